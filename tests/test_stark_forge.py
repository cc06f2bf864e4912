"""The STARK forger (tests/stark_forge.py) validated against the oracle's verifier, and its envelopes through the device verifier's own
code compiled for the host (stark_verify_envelope of libzkp_amd/csrc/stark_steps.h in tests/emul/emul_stark.cpp).  No GPU.

Self-validation: each forgery is refused by the oracle, accepted by the oracle without the ONE check the forgery names, and refused without
any other single check -- so a forgery that the device verifier accepted would mean that this check is missing there.  Host leg: the device
verifier's verdict on every forgery and every grammar-aware mutation equals the oracle's."""
import collections
import ctypes
import os
import re

import pytest

import stark_forge as F
from oracle.py import stark as s


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_stark.so"))
    L.emul_stark_verify.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64]
    return L


@pytest.fixture(scope="module")
def cases():
    return F.corpus()


def test_the_honest_restatement_is_the_oracles_prover():
    assert len(F.PAIRS) >= 3 and (0, 1) in F.PAIRS and (2**64 - 2, 2**64 - 1) in F.PAIRS
    for (old, new), count in F.PAIRS.items():
        d = {}
        assert F.forge(old, new, detail=d) == s.prove(old, new)
        assert len(d["positions"]) == count
        assert F.envelope(old, new, F.forge(old, new)) == s.prove_improvement(old, new)
    assert len(set(F.PAIRS.values())) >= 5                         # the openings' shapes differ


def test_every_forgery_is_refused_by_its_check_alone():
    seen = collections.Counter()
    with F.memoised_hash():
        for old, new in F.PAIRS:
            for f in F.forgeries(old, new):
                proof = f.env[26:-32]
                nq = proof[28]                                     # the forgery's own count of opened positions
                assert f.env == F.envelope(old, new, proof) and f.old == old
                assert not s.verify_improvement(f.env, old), f.name
                assert not s.verify(proof, old, new), f.name
                assert s.verify(proof, old, new, skip={f.check}), (f.name, old, new)
                name = f.check if isinstance(f.check, str) else "deep"
                for other in s.SKIPPABLE:
                    assert s.verify(proof, old, new, skip={other}) == (other == name), (f.name, other, old, new)
                if name == "deep":
                    k = f.check[1]
                    assert k == (0 if f.name.endswith("first") else nq - 1 if f.name.endswith("last") else k) and 0 <= k < nq
                    assert f.name.endswith("middle") == (0 < k < nq - 1)
                    for j in range(nq):
                        assert s.verify(proof, old, new, skip={("deep", j)}) == (j == k), (f.name, j, k)
                seen[f.name] += 1
    pairs = len(F.PAIRS)
    assert set(seen) == {"h_shift", "bent_trace", "wrong_first_row", "wrong_last_row", "fake_rem_commit", "padded_queries", "fake_t_root",
                         "fake_h_root"} | set(F.LEAF_FAMILIES)
    assert all(n == pairs for n in seen.values())


def test_layout_names_every_byte():
    for old, new in F.PAIRS:
        env = s.prove_improvement(old, new)
        L = F.layout(env)
        covered = sorted(v for k, v in L.items() if not re.search(r"\.(block|opening|list\d+)$", k))          # without the fields that span others
        assert covered[0][0] == 0 and sum(covered[-1]) == len(env)
        assert all(a[0] + a[1] == b[0] for a, b in zip(covered, covered[1:]))          # no gap, no overlap
        assert len(F.element_fields(L)) == 2 * F.PAIRS[(old, new)] + 11
        for w in range(1, 10):
            assert s.read_vint(F.vint_w(100, w) + b"\xff", 0) == (100, w) and F.vint_width(F.vint_w(100, w), 0) == w
        assert F.vint_w(416, 2) == s.vint(416) and F.vint_w(2**63, 9) == s.vint(2**63)


def test_the_oracle_on_the_mutations(cases):
    """what the mutations are, by the oracle: the re-encoded length prefixes stay valid; wrong prefix values, non-canonical elements and bent
    structure or framing do not"""
    kinds = collections.Counter(c.kind for c in cases)
    assert kinds["forgery"] == 14 * len(F.PAIRS) and kinds["vint_form"] == 2 * 44 and kinds["vint_value"] == 2 * 18
    assert kinds["element"] == 3 * (2 * F.PAIRS[F.MUTATED_IN_FULL] + 11) and kinds["structure"] == 2 * 26 and kinds["framing"] == 2 * 14
    assert kinds["honest"] >= len(cases) // 4 - 1
    for c in cases:
        assert c.want == (c.kind in ("honest", "vint_form")), c.name
    widths = {c.name.split(":")[1].split("(")[0] for c in cases if c.kind == "vint_form"}
    assert widths == {"%d_bytes" % w for w in range(2, 10)}        # (one byte is what the list counts have to begin with)


def host_verdicts(lib, cases):
    return [bool(lib.emul_stark_verify(c.env, len(c.env), c.old)) for c in cases]


def test_host_leg_forgeries_are_rejected(lib, cases):
    """a forgery accepted here names the check that stark_verify_envelope lacks"""
    got = host_verdicts(lib, cases)
    accepted = [c.name for c, ok in zip(cases, got) if c.kind == "forgery" and ok]
    assert not accepted, accepted
    assert all(ok for c, ok in zip(cases, got) if c.kind == "honest")


def test_host_leg_vint_forms_are_accepted(lib, cases):
    """Every width of a length prefix that winter-utils' read_usize takes.  Before StarkReader::vint read the 5- to 9-byte forms, 60 of the 88
    re-encodings here (all those of 5 to 9 bytes) were refused."""
    got = host_verdicts(lib, cases)
    refused = [c.name for c, ok in zip(cases, got) if c.kind == "vint_form" and not ok]
    assert not refused, refused


def test_host_leg_verdicts_equal_the_oracle(lib, cases):
    got = host_verdicts(lib, cases)
    differ = [(c.name, ok, c.want) for c, ok in zip(cases, got) if ok != c.want]
    assert not differ, differ
    assert 400 <= len(cases) <= 800
    assert all(c.old == int.from_bytes(c.env[10:18], "little") for c in cases)         # the mixed verifier takes `old` from the envelope
