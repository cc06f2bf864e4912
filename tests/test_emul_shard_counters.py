"""The shards' counter table on the host (no GPU): libzkp_amd/csrc/shard_counters.h compiled from the header the library uses
(tests/emul/emul_shard_counters.cpp) -- the family table against the exports' declarations under include/, the read that sums one family
over the shards, the tally's two counting rules, the Bulletproofs verifiers' one failed check."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = ctypes.c_uint64
# family (in the order emul_ctr_family_ids names them) -> the header that declares its export, the export
EXPORT = (("g16_verify", "libzkp_hip.h", "zkp_hip_profile_read_kernel"), ("batch_self_check", "libzkp_hip.h", "zkp_hip_profile_read_kernel"),
          ("verify_fanout", "libzkp_hip.h", "zkp_hip_profile_read_kernel"), ("verify_mixed", "libzkp_hip.h", "zkp_hip_profile_read_kernel"),
          ("bp_localise", "libzkp_hip_bp_localise.h", "zkp_hip_bp_localise_counters"), ("composites", "libzkp_hip_composites.h", "zkp_hip_composites_counters"),
          ("seal", "libzkp_hip_seal.h", "libzkp_seal_counters"), ("statements", "libzkp_hip_statements.h", "zkp_stmt_counters"),
          ("key_check", "libzkp_hip_keycheck.h", "zkpkeycheck_counters"))
ID_BASED = {"g16_verify": "ZKP_HIP_COUNTER_G16_VERIFY", "batch_self_check": "ZKP_HIP_COUNTER_BATCH_SELF_CHECK", "verify_fanout": "ZKP_HIP_COUNTER_VERIFY_FANOUT",
            "verify_mixed": "ZKP_HIP_COUNTER_VERIFY_MIXED"}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_shard_counters.so"))
    for f in (L.emul_ctr_families, L.emul_ctr_max_fields, L.emul_ctr_fields):
        f.restype = ctypes.c_uint32
    L.emul_ctr_fields.argtypes = [ctypes.c_uint32]
    L.emul_ctr_family_ids.argtypes = [ctypes.c_void_p]
    L.emul_ctr_read.argtypes = [ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.POINTER(U64)),
                                ctypes.c_uint32]
    L.emul_ctr_read.restype = None
    L.emul_ctr_tally.argtypes = [ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_ctr_tally.restype = ctypes.c_int
    L.emul_ctr_bp_localise.argtypes = [ctypes.c_uint32, U64, U64, ctypes.c_void_p]
    L.emul_ctr_bp_localise.restype = None
    return L


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def family_ids(L):
    ids = np.zeros(len(EXPORT), dtype=np.uint32)
    L.emul_ctr_family_ids(P(ids))
    return {name: int(i) for (name, _, _), i in zip(EXPORT, ids)}


def declaration(header, export):
    text = open(os.path.join(ROOT, "include", header)).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % re.escape(export), text)
    assert m, (header, export)
    return [p.strip() for p in m.group(1).split(",")]


def test_field_counts_are_the_exports_uint64_parameters(lib):
    ids = family_ids(lib)
    assert lib.emul_ctr_families() == len(EXPORT) == 9 and sorted(ids.values()) == list(range(9))
    for name, header, export in EXPORT:
        params = declaration(header, export)
        counts = [p for p in params if re.match(r"uint64_t\s*\*", p)]
        assert params[-1] == "int reset" and any(re.match(r"double\s*\*\s*ms$", p) for p in params)
        assert lib.emul_ctr_fields(ids[name]) == len(counts) <= lib.emul_ctr_max_fields(), name
        assert len(counts) == (2 if name in ID_BASED else {"bp_localise": 3, "composites": 3, "seal": 4, "statements": 4, "key_check": 3}[name])
    assert lib.emul_ctr_fields(9) == 0


def test_id_based_families_sit_at_which_minus_the_first_counter_id(lib):
    ids = family_ids(lib)
    text = open(os.path.join(ROOT, "include", "libzkp_hip.h")).read()
    value = {c: int(re.search(r"\b%s\s*=\s*(\d+)" % c, text).group(1)) for c in ID_BASED.values()}
    for name, const in ID_BASED.items():
        assert ids[name] == value[const] - value["ZKP_HIP_COUNTER_G16_VERIFY"]


def tables(shards, families, fields):
    ms = (np.arange(shards * families, dtype=np.float64) + 1) * 0.25                  # sums of these are exact in a double
    v = (np.arange(shards * families * fields, dtype=np.uint64) * 1000 + 7).reshape(shards, families, fields)
    return ms.reshape(shards, families), v


def read(L, ms, v, family, reset, nouts, null=()):
    got_ms = ctypes.c_double(-1.0)
    got = [U64(2**64 - 1) for _ in range(nouts)]
    outs = (ctypes.POINTER(U64) * nouts)(*[None if k in null else ctypes.pointer(got[k]) for k in range(nouts)])
    L.emul_ctr_read(ms.shape[0], P(ms), P(v), family, 1 if reset else 0, ctypes.byref(got_ms), outs, nouts)
    return got_ms.value, [g.value for g in got]


@pytest.mark.parametrize("shards", (1, 2, 64))
def test_read_sums_one_family_over_the_shards_and_resets_only_it(lib, shards):
    F, K = lib.emul_ctr_families(), lib.emul_ctr_max_fields()
    for family in range(F):
        n = lib.emul_ctr_fields(family)
        for reset in (False, True):
            ms, v = tables(shards, F, K)
            ms0, v0 = ms.copy(), v.copy()
            got_ms, got = read(lib, ms, v, family, reset, n)
            assert got_ms == ms0[:, family].sum() and got == [int(x) for x in v0[:, family, :n].sum(axis=0)]
            want_ms, want_v = ms0.copy(), v0.copy()
            if reset:
                want_ms[:, family] = 0
                want_v[:, family, :] = 0                                               # every shard's, and no other family's
            assert (ms == want_ms).all() and (v == want_v).all()


def test_null_outs_are_skipped_and_the_others_overwritten(lib):
    F, K = lib.emul_ctr_families(), lib.emul_ctr_max_fields()
    for family in range(F):
        n = lib.emul_ctr_fields(family)
        for null in range(n):
            ms, v = tables(3, F, K)
            _, got = read(lib, ms, v, family, False, n, null=(null,))
            want = [int(x) for x in v[:, family, :n].sum(axis=0)]
            want[null] = 2**64 - 1                                                     # what the test put there: nothing was written through a null out
            assert got == want                                                         # the others held 2^64 - 1 too: overwritten, not added to
        ms, v = tables(3, F, K)
        want = [int(x) for x in v[:, family, :n].sum(axis=0)]
        got = [U64(2**64 - 1) for _ in range(n)]
        outs = (ctypes.POINTER(U64) * n)(*[ctypes.pointer(g) for g in got])
        lib.emul_ctr_read(3, P(ms), P(v), family, 0, None, outs, n)                    # a null ms beside outs that are not: they are still written
        assert [g.value for g in got] == want
        lib.emul_ctr_read(3, P(ms), P(v), family, 1, None, (ctypes.POINTER(U64) * n)(), n)      # every out null, ms too: the reset still happens
        assert (v[:, family, :] == 0).all() and (ms[:, family] == 0).all()


def tally(L, family, rule, early, fields):
    v = np.zeros((L.emul_ctr_families(), L.emul_ctr_max_fields()), dtype=np.uint64)
    s = np.asarray(fields, dtype=np.uint64)
    assert L.emul_ctr_tally(family, rule, 1 if early else 0, P(s), P(v)) == 1          # ms: >= 0 in this family, 0 in every other
    return v


def test_a_tally_adds_once_whichever_way_its_scope_ends(lib):
    for family in range(lib.emul_ctr_families()):
        for early in (False, True):
            v = tally(lib, family, 0, early, [3, 5, 7, 11])
            want = np.zeros_like(v)
            want[family] = [3, 5, 7, 11]
            assert (v == want).all()


def test_a_committed_only_tally_adds_at_commit_and_never_otherwise(lib):
    for family in range(lib.emul_ctr_families()):
        v = tally(lib, family, 1, False, [3, 5, 7, 11])                                # committed before the end
        want = np.zeros_like(v)
        want[family] = [3, 5, 7, 11]
        assert (v == want).all()
        assert not tally(lib, family, 1, True, [3, 5, 7, 11]).any()                    # an early return before the commit
        assert not tally(lib, family, 2, False, [3, 5, 7, 11]).any()                   # never committed


def test_the_bp_localise_tally_counts_one_failed_check(lib):
    v = np.zeros(lib.emul_ctr_max_fields(), dtype=np.uint64)
    lib.emul_ctr_bp_localise(0, 0, 0, P(v))                                            # made after the failed check, the call returns at once
    assert v.tolist() == [1, 0, 0, 0]
    lib.emul_ctr_bp_localise(2, 16, 40, P(v))
    assert v.tolist() == [1, 32, 80, 0]

