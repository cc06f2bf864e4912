"""One prover workspace reused across shrinking and regrowing shapes in one process (prover_plan.h: the plan and binder of the range /
threshold / consistency prover and of the Groth16 prover).  The size tests only ever grow a workspace; here a larger call's layout is still
in the buffer when a smaller one is bound over it, the any-failed word is read after a shrink, and a narrower bit width may raise the chunk
count under an existing workspace.  Bytes against the C oracle, Groth16 rows against the trapdoor reference."""
import ctypes
import os

import numpy as np
import pytest

from oracle.py import groth16 as g
from util import P, PROOF, U64, oracle_prove, outputs, workload

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SS = bytes(range(32))


@pytest.fixture(scope="module")
def hip():
    from libzkp_amd import _native
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        blob = open(os.path.join(GOLD, name), "rb").read()
        assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0
    return L


def prove_range(hip, oracle_c, n, seed, bad=None):
    """one 64-bit call of n ops; op `bad` (if any) has value > max: refused alone, every other op's bytes are the oracle's"""
    v, mn, mx, seeds = workload(n, seed)
    if bad is not None:
        v[bad] = mx[bad] + 1
    out, lens, st = outputs(n)
    rc = hip.zkp_hip_prove_range_batch(n, P(v), P(mn), P(mx), 64, P(seeds), P(out), PROOF, P(lens), P(st))
    good = [i for i in range(n) if i != bad]
    assert rc == (0 if bad is None else 1), (n, rc)
    assert [int(st[i]) for i in good] == [0] * len(good) and [int(lens[i]) for i in good] == [PROOF] * len(good)
    if bad is not None:
        assert st[bad] == 1 and lens[bad] == 0 and (out[bad] == 0).all()
    rc2, ref, _, _ = oracle_prove(oracle_c, v[good].copy(), mn[good].copy(), mx[good].copy(), seeds.reshape(n, 32)[good].ravel().copy())
    assert rc2 == 0 and (out[good] == ref).all(), n


def test_range_shrinks_regrows_and_changes_width(hip, oracle_c):
    for n, bad in ((65, None), (2, 1), (33, 17), (1, None), (65, None)):      # the calls around a refused op return 0: the flag is read after a shrink
        prove_range(hip, oracle_c, n, 700 + n, bad)
    # another bit width is another family of launches: its chunk counts may exceed those the workspace was sized for
    n, bits = 3, 8
    v, mn, mx, seeds = workload(n, 708, 0, 255)
    stride = int(hip.zkp_hip_range_proof_bytes(bits))
    out, lens, st = outputs(n, stride)
    ref, rlens, rst = outputs(n, stride)
    assert hip.zkp_hip_prove_range_batch(n, P(v), P(mn), P(mx), bits, P(seeds), P(out), stride, P(lens), P(st)) == 0
    assert oracle_c.zkp_oracle_prove_range_batch(U64(n), P(v), P(mn), P(mx), bits, P(seeds), P(ref), U64(stride), P(rlens), P(rst), 4) == 0
    assert (st == 0).all() and (lens == rlens).all() and (lens == stride).all() and (out == ref).all()


def _flat(lists):
    return np.array([x for l in lists for x in l], dtype=np.uint64), np.array([len(l) for l in lists], dtype=np.uint32)


def test_threshold_consistency_range_on_one_workspace(hip, oracle_c):
    ref, ol = ctypes.create_string_buffer(4096), ctypes.c_uint32()
    # threshold: one job per op and no commitment task
    lists = [[50], [10, 20, 30], [7], [1, 2, 3], [2**63]]
    thr = np.array([50, 45, 0, 6, 1], dtype=np.uint64)
    flat, counts = _flat(lists)
    n = len(lists)
    seeds = (np.arange(32 * n, dtype=np.uint32) * 5 + 3).astype(np.uint8)
    out, lens, st = outputs(n, 800)
    assert hip.zkp_hip_prove_threshold_batch(n, P(flat), P(counts), P(thr), 64, P(seeds), P(out), 800, P(lens), P(st)) == 0
    assert (st == 0).all() and (lens == 762).all()
    for i in range(n):
        vals = (ctypes.c_uint64 * len(lists[i]))(*lists[i])
        assert oracle_c.zkp_oracle_prove_threshold(vals, len(lists[i]), U64(int(thr[i])), 64, seeds[32 * i: 32 * i + 32].tobytes(), ref, 4096, ctypes.byref(ol)) == 0
        assert ol.value == 762 and out[i, :762].tobytes() == ref.raw[:762] and (out[i, 762:] == 0).all(), i
    # consistency: k - 1 jobs and k commitment tasks per op
    lists = [[10, 20], [1, 2, 3, 4], [0, 2**64 - 1], [5, 5, 5, 9]]
    flat, counts = _flat(lists)
    n = len(lists)
    stride = max(int(hip.zkp_hip_consistency_proof_bytes(len(l))) for l in lists)
    seeds = (np.arange(32 * n, dtype=np.uint32) * 7 + 1).astype(np.uint8)
    out, lens, st = outputs(n, stride)
    assert hip.zkp_hip_prove_consistency_batch(n, P(flat), P(counts), P(seeds), P(out), stride, P(lens), P(st)) == 0 and (st == 0).all()
    for i in range(n):
        d = (ctypes.c_uint64 * len(lists[i]))(*lists[i])
        assert oracle_c.zkp_oracle_prove_consistency(d, len(lists[i]), seeds[32 * i: 32 * i + 32].tobytes(), ref, 4096, ctypes.byref(ol)) == 0
        assert lens[i] == ol.value and out[i, : lens[i]].tobytes() == ref.raw[: ol.value], i
    # range: two jobs and one task per op
    prove_range(hip, oracle_c, 2, 731)


def test_equality_workspace_shrinks_and_regrows(hip):
    """(the trapdoor key is derived once per process by oracle.py.groth16 and shared with test_gpu_sizes.py: seconds on first use)"""
    for n in (65, 1, 33):
        rng = np.random.default_rng(740 + n)
        v = rng.integers(0, 2**63, n, dtype=np.uint64)
        seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
        out, lens, st = outputs(n, 298)
        assert hip.zkp_hip_prove_equality_batch(n, P(v), P(v), P(seeds), P(out), 298, P(lens), P(st)) == 0 and (lens == 298).all()
        for i in sorted({0, n - 1}):
            sd = seeds[32 * i:32 * i + 32].tobytes()
            cm = g.commit_value_snark(int(v[i]))
            cs = g.equality_circuit(int(v[i]), int(v[i]), int.from_bytes(cm, "little"))
            want = g.envelope(2, g.prove_with_trapdoor(g.equality_key(SS), cs, g.draw_fr(sd, 0x47313600, 0), g.draw_fr(sd, 0x47313600, 1)), cm)
            assert out[i].tobytes() == want, (n, i)
        ok = np.zeros(n, dtype=np.uint8)
        assert hip.zkp_hip_verify_equality_batch(n, P(out), 298, P(lens), P(ok)) == 0 and (ok == 1).all()


def test_membership_workspace_shrinks(hip):
    for n in (4, 1):
        rng = np.random.default_rng(750 + n)
        sets = rng.integers(0, 2**32, (n, 5), dtype=np.uint64)
        v = sets[np.arange(n), np.arange(n) % 5].copy()
        cnt = np.full(n, 5, dtype=np.uint32); flat = sets.ravel().copy()
        seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
        stride = 10 + 4 + 8 * 5 + 256 + 32
        out, lens, st = outputs(n, stride)
        assert hip.zkp_hip_prove_membership_batch(n, P(v), P(flat), P(cnt), P(seeds), P(out), stride, P(lens), P(st)) == 0 and (lens == stride).all()
        for i in sorted({0, n - 1}):
            assert g.verify_membership(out[i].tobytes(), [int(x) for x in sets[i]], SS), (n, i)
