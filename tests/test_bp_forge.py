"""The forger of tests/bp_forge.py against both oracle verifiers, without a GPU: what "well-formed but invalid" means for the
inputs of tests/test_gpu_bp_batch_check.py.  Envelopes come from the C oracle's provers, at every bit width."""
import ctypes

import numpy as np
import pytest

import bp_forge as F
from util import P, U64

WIDTHS = (8, 16, 32, 64)


def _env(oracle_c, fn, *args):
    out = ctypes.create_string_buffer(8192)
    ln = ctypes.c_uint32()
    assert fn(*args, out, 8192, ctypes.byref(ln)) == 0
    return out.raw[:ln.value]


def range_env(oracle_c, v, mn, mx, bits, seed):
    return _env(oracle_c, oracle_c.zkp_oracle_prove_range, U64(v), U64(mn), U64(mx), ctypes.c_uint32(bits), seed)


def threshold_env(oracle_c, values, thr, bits, seed):
    arr = (ctypes.c_uint64 * len(values))(*values)
    return _env(oracle_c, oracle_c.zkp_oracle_prove_threshold, arr, ctypes.c_uint32(len(values)), U64(thr), ctypes.c_uint32(bits), seed)


def consistency_env(oracle_c, data, seed):
    arr = (ctypes.c_uint64 * len(data))(*data)
    return _env(oracle_c, oracle_c.zkp_oracle_prove_consistency, arr, ctypes.c_uint32(len(data)), seed)


c_verify = F.c_verify


def seed(i):
    return bytes([i]) * 32


def make(oracle_c, scheme, bits):
    """(envelope, donor of the same shape for another value, bounds)"""
    if scheme == 1:
        mn, mx = 1000, 1000 + min(2**bits - 1, 2**40)
        return range_env(oracle_c, mn + 77, mn, mx, bits, seed(bits)), range_env(oracle_c, mn + 78, mn, mx, bits, seed(bits + 1)), (mn, mx)
    if scheme == 3:
        return threshold_env(oracle_c, [40, 50, 60], 100, bits, seed(bits + 2)), threshold_env(oracle_c, [40, 50, 61], 100, bits, seed(bits + 3)), (100,)
    return consistency_env(oracle_c, [5, 9, 9], seed(200)), consistency_env(oracle_c, [5, 8, 30], seed(201)), ()


def expected_field_forgeries(n_proofs, lg, n_commitments):
    """per inner proof 4 + 2 lg n points and 5 scalars, plus the commitments; three mutations of a point, two of a scalar"""
    return n_proofs * ((4 + 2 * lg) * len(F.POINT_MUTATIONS) + 5 * len(F.SCALAR_MUTATIONS)) + n_commitments * len(F.POINT_MUTATIONS)


def test_the_forger_covers_every_slot(oracle_c):
    env, donor, _ = make(oracle_c, 1, 64)
    assert len(env) == 1478
    got = F.field_forgeries(env)
    assert len(got) == 2 * (16 * 3 + 5 * 2) + 3 * 3 == 125 == expected_field_forgeries(2, 6, 3)
    names = [f.name for f in got]
    assert len(set(names)) == len(names) and len({f.env for f in got}) == len(got)
    for proof in ("rp_min", "rp_max"):
        for slot in ["A", "S", "T1", "T2"] + ["L%d" % j for j in range(6)] + ["R%d" % j for j in range(6)]:
            assert ["%s.%s:%s" % (proof, slot, m) in names for m in F.POINT_MUTATIONS] == [True] * 3
        for slot in F.SCALAR_NAMES:
            assert ["%s.%s:%s" % (proof, slot, m) in names for m in F.SCALAR_MUTATIONS] == [True] * 2
    for c in ("c_min", "c_max", "value_commitment"):
        assert ["%s:%s" % (c, m) in names for m in F.POINT_MUTATIONS] == [True] * 3
    assert [f.name for f in F.transplant_forgeries(env, donor)] == ["rp_min_and_rp_max_swapped", "proofs_of_another_envelope", "commitments_shifted_by_B"]
    for bits, lg, size in ((8, 3, 1094), (16, 4, 1222), (32, 5, 1350)):
        e = make(oracle_c, 1, bits)[0]
        assert len(e) == size and len(F.field_forgeries(e)) == expected_field_forgeries(2, lg, 3)
    assert len(F.field_forgeries(make(oracle_c, 3, 64)[0])) == expected_field_forgeries(1, 6, 2) == 64
    assert len(F.field_forgeries(make(oracle_c, 6, 64)[0])) == expected_field_forgeries(2, 6, 3 + 2) == 131
    # every forgery differs from the envelope in exactly the fields its name says: a field forgery in one 32-byte field
    for f in got:
        diff = [i for i in range(len(env)) if env[i] != f.env[i]]
        assert diff and diff[-1] - diff[0] < 32 and len(f.env) == len(env)


CASES = [(1, b) for b in WIDTHS] + [(3, b) for b in WIDTHS] + [(6, 64)]


@pytest.mark.parametrize("scheme,bits", CASES)
def test_forgeries_are_well_formed_and_rejected_by_both_oracles(oracle_c, scheme, bits):
    env, donor, bounds = make(oracle_c, scheme, bits)
    assert F.layout(env).n_bits == bits
    for e in (env, donor):
        assert F.well_formed(e) and F.rejection_stage(e, *bounds) == "accepted" and c_verify(oracle_c, e, *bounds)
    forged = F.forgeries(env, donor)
    for _, plus, minus in F.opposite_pairs(env):
        forged += [F.Forgery("pair", plus, "equation"), F.Forgery("pair", minus, "equation")]
    assert len(forged) >= len(F.field_forgeries(env)) + 2 + 12
    stages = set()
    for f in forged:
        assert f.env != env and len(f.env) == len(env), f.name
        assert F.well_formed(f.env), f.name
        assert not c_verify(oracle_c, f.env, *bounds), f.name
        assert F.rejection_stage(f.env, *bounds) == f.stage, f.name      # rejected by the Python verifier, and where
        stages.add(f.stage)
    assert stages == {"equation", "rule"}


@pytest.mark.parametrize("scheme,bits", CASES)
def test_excluded_envelopes_fail_before_any_equation(oracle_c, scheme, bits):
    env, _, bounds = make(oracle_c, scheme, bits)
    lay = F.layout(env)
    ex = F.excluded(env)
    n_points = sum(f.kind == "point" for f in lay.proof_fields) + len(lay.commitments)
    assert len(ex) == 5 * len(lay.proofs) + 3 * n_points
    for name, e in ex:
        assert len(e) == len(env) and e != env, name
        assert not F.well_formed(e), name
        assert F.rejection_stage(e, *bounds) == "rule", name
        assert not c_verify(oracle_c, e, *bounds), name
