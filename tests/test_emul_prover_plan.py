"""The workspace plans of the two provers' host paths on the host (no GPU): bp_prove_plan, bp_prove_bind, g16_prove_plan and g16_prove_bind of
libzkp_amd/csrc/prover_plan.h, compiled from the header the library uses (tests/emul/emul_prover_plan.cpp), against a model written here from
the header's comment block (the regions of each block in take order, their byte formulas) and, for what every array needs, from the field
comments of JobBuf, BpView, CtView, MsmView, ReduceView (bp_steps.h) and G16View (g16_steps.h).  A wrong size or a forgotten region in a plan
is an out-of-bounds device write; nothing but a GPU fault showed one before."""
import ctypes
import itertools
import os

import numpy as np
import pytest

TAPE_SLOTS, P1_NSLOTS, P2_NSLOTS, PR_NSLOTS, SC_NUM, DIGW, GE_W = 132, 260, 4, 130, 9, 13, 40
G1_JAC_W, G2_JAC_W, G16_CPARTS = 30, 60, 4
EQUALITY, MEMBERSHIP = (334, 512), (653, 1024)                                                      # (nv, m) of the shipped circuits
BP_WORDS, G16_WORDS, WS_WORDS, G16_VIEW_WORDS = 35, 11, 55, 25

MS, CS, MAX_CHUNKS, CT_CHUNKS = (1, 2, 3, 130, 8192), (1, 2, 65, 4096), (1, 3, 50), (1, 2)           # includes the range shape M = 2C and M != 2C
ROWS, DIGWS, CIRCUITS, G16_CHUNKS = (1, 65, 4096), (8, 13, 16), (EQUALITY, MEMBERSHIP, (7, 8)), (1, 7, 40)

JOB_FIELDS = ("v", "seed_ix", "proof_ix", "bl_plus", "bl_minus", "kind", "proof_off", "commit_off", "ct_v", "ct_seed_ix", "ct_bl_ix", "ct_off")
WORK_FIELDS = ("tape", "gamma", "d1", "d2", "dr", "yinvpow", "ypq", "r0", "r1", "pp", "ab", "gh", "scal", "tstate", "enc")
WS_FIELDS = (tuple("J." + f for f in JOB_FIELDS)
             + tuple("V." + f for f in ("M", "n", "lg", "wbits", "v", "seed_ix", "proof_ix", "bl_plus", "bl_minus", "kind", "seeds", "proof_off", "commit_off", "out") + WORK_FIELDS)
             + tuple("T." + f for f in ("C", "v", "seed_ix", "bl_ix", "seeds", "digits", "wbits"))
             + ("partial", "ct_partial", "ct_enc", "sums", "ct_sums", "ct_off", "flag"))
# Ws field -> region: the job arrays (and the views' read-only aliases of them), the work arrays, the launchers' arrays
WS_BOUND = dict([("J." + f, f) for f in JOB_FIELDS] + [("V." + f, f) for f in JOB_FIELDS[:8]] + [("V." + f, f) for f in WORK_FIELDS]
                + [("T.v", "ct_v"), ("T.seed_ix", "ct_seed_ix"), ("T.bl_ix", "ct_bl_ix"), ("T.digits", "ct_digits")]
                + [(f, f) for f in ("partial", "ct_partial", "ct_enc", "sums", "ct_sums", "ct_off", "flag")])
G16_VIEW_FIELDS = ("rows", "kind", "rx.wbits", "rx.digw", "n_inst", "n_wit", "nv", "m", "value", "set_vals", "set_len", "seeds", "mimc_c", "z", "sdig", "rs", "qap_evals",
                   "out", "stride", "p1", "p1c", "p2", "s1", "s2", "t1")
G16_BOUND = {"z": "z", "sdig": "sdig", "rs": "rs", "qap_evals": "qe", "p1": "p1", "p1c": "p1c", "p2": "p2", "s1": "s1", "s2": "s2", "t1": "t1"}


def pad256(x):
    return (x + 255) & ~255


# ---- the model: the header's comment, region by region
def bp_regions(M, C, max_chunks, ct_chunks):
    S, D = 32 * M, DIGW * 4 * M
    return [("flag", 256),
            ("v", 8 * M), ("seed_ix", 4 * M), ("proof_ix", 4 * M), ("bl_plus", 4 * M), ("bl_minus", 4 * M), ("kind", M), ("proof_off", 8 * M), ("commit_off", 8 * M),
            ("ct_v", 8 * C), ("ct_seed_ix", 4 * C), ("ct_bl_ix", 4 * C), ("ct_off", 8 * C),
            ("tape", S * TAPE_SLOTS), ("gamma", S), ("d1", D * P1_NSLOTS), ("d2", D * P2_NSLOTS), ("dr", D * PR_NSLOTS), ("yinvpow", S * 64), ("ypq", S * 32), ("r0", S * 64),
            ("r1", S * 64), ("pp", S * 192), ("ab", S * 256), ("gh", S * 128), ("scal", S * SC_NUM), ("tstate", 4 * 52 * M), ("enc", S * 3),
            ("partial", max_chunks * GE_W * 4 * M), ("sums", 3 * GE_W * 4 * M),
            ("ct_digits", 2 * DIGW * 4 * C), ("ct_partial", ct_chunks * GE_W * 4 * C), ("ct_enc", 32 * C), ("ct_sums", GE_W * 4 * C)]


def g16_regions(rows, nv, m, digw, nchunks_ab, nchunks_c, nchunks_g2):
    nsc = nv + m + 3
    return [("z", 32 * rows * nv), ("sdig", digw * 4 * rows * nsc), ("rs", 32 * rows * 2), ("p1", nchunks_ab * G1_JAC_W * 4 * rows), ("p1c", nchunks_c * G1_JAC_W * 4 * rows),
            ("p2", nchunks_g2 * G2_JAC_W * 4 * rows), ("s1", 3 * G1_JAC_W * 4 * rows), ("s2", G2_JAC_W * 4 * rows), ("t1", G16_CPARTS * G1_JAC_W * 4 * rows),
            ("qe", 3 * 36 * m * rows)]


def lay_out(regions):
    """offsets and the total of a block whose regions are taken in order, each padded to 256 bytes"""
    off, lay = 0, {}
    for name, size in regions:
        lay[name] = off
        off += pad256(size)
    return lay, off


# ---- what every array needs: the views' field comments, in bytes
def bp_needs(M, C, max_chunks, ct_chunks):
    words = 4
    sc = 8 * M * words                                                                            # "[..][8][M] words unless noted"
    return {"flag": 4,
            "v": 8 * M, "seed_ix": 4 * M, "proof_ix": 4 * M, "bl_plus": 4 * M, "bl_minus": 4 * M, "kind": M, "proof_off": 8 * M, "commit_off": 8 * M,      # [M] of u64, u32, u32, i32, i32, u8, u64, u64
            "ct_v": 8 * C, "ct_seed_ix": 4 * C, "ct_bl_ix": 4 * C, "ct_off": 8 * C,                # [C] of u64, u32, u32, u64
            "tape": 132 * sc, "gamma": sc,
            "d1": 260 * 13 * M * words, "d2": 4 * 13 * M * words, "dr": 130 * 13 * M * words,     # [260], [4], [130] packed digits: [slots][digit words][M]
            "yinvpow": 64 * sc, "ypq": 32 * sc, "r0": 64 * sc, "r1": 64 * sc, "pp": 3 * 64 * sc, "ab": 2 * 2 * 64 * sc, "gh": 2 * 64 * sc, "scal": 9 * sc,
            "tstate": 52 * M * words, "enc": 3 * sc,                                              # [52][M], [3][8][M]
            "partial": max_chunks * 40 * M * words, "sums": 3 * 40 * M * words,                   # [nchunks][40][rows]; three targets [3][40][M]
            "ct_digits": 2 * 13 * C * words, "ct_partial": ct_chunks * 40 * C * words,            # [2][DIGW][C], [nchunks][40][rows]
            "ct_enc": 8 * C * words, "ct_sums": 40 * C * words}                                   # one target: [1][8][C], [1][40][C]


def g16_needs(rows, nv, m, digw, nchunks_ab, nchunks_c, nchunks_g2):
    words = 4
    return {"z": nv * 8 * rows * words, "sdig": (nv + m + 3) * digw * rows * words, "rs": 2 * 8 * rows * words,      # [nv][8][rows], [nscalars][rx.digw][rows], [2][8][rows]
            "qe": 3 * m * 9 * rows * words,                                                        # [3][m][9][rows]
            "p1": nchunks_ab * 30 * rows * words, "p1c": nchunks_c * 30 * rows * words, "p2": nchunks_g2 * 60 * rows * words,      # [nchunks][ACC_W][rows]
            "s1": 3 * 30 * rows * words, "s2": 60 * rows * words, "t1": 4 * 30 * rows * words}        # [3][G1_JAC_W][rows], [1][G2_JAC_W][rows], [G16_CPARTS][G1_JAC_W][rows]


def check_block(lay, total, regions, needs):
    """the plan is the model's; every region 256-aligned, inside [0, total), as large as its array needs, disjoint from the others"""
    m_lay, m_total = lay_out(regions)
    assert lay == m_lay and total == m_total == sum(pad256(size) for _, size in regions)
    assert set(needs) == set(lay)
    end = 0
    for off, padded, name in sorted((lay[name], pad256(size), name) for name, size in regions):
        assert off % 256 == 0 and off >= end and off + padded <= total, (name, off, end, total)
        assert padded >= needs[name], (name, padded, needs[name])
        end = off + padded


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_prover_plan.so"))
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_pp_constants.argtypes = [vp]
    L.emul_pp_bp_plan.argtypes = [u32, u32, u32, u32, vp]
    L.emul_pp_g16_plan.argtypes = [u32] * 7 + [vp]
    L.emul_pp_bp_bind.argtypes = [u64] + [u32] * 7 + [u64, vp]
    L.emul_pp_g16_bind.argtypes = [u64] + [u32] * 7 + [u64, vp]
    c = np.zeros(18, dtype=np.uint32)
    L.emul_pp_constants(c.ctypes.data)
    assert c.tolist() == [TAPE_SLOTS, P1_NSLOTS, P2_NSLOTS, PR_NSLOTS, SC_NUM, DIGW, GE_W, G1_JAC_W, G2_JAC_W, G16_CPARTS, *EQUALITY, *MEMBERSHIP,
                          BP_WORDS, G16_WORDS, WS_WORDS, G16_VIEW_WORDS]
    return L


def words(call, count, *args):
    out = np.full(count + 1, 0x5151, dtype=np.uint64)
    call(*args, out.ctypes.data)
    assert out[count] == 0x5151
    return [int(x) for x in out[:count]]


def bp_plan(L, *shape):
    w = words(L.emul_pp_bp_plan, BP_WORDS, *shape)
    return dict(zip((name for name, _ in bp_regions(*shape)), w)), w[-1]


def g16_plan(L, *shape):
    w = words(L.emul_pp_g16_plan, G16_WORDS, *shape)
    return dict(zip((name for name, _ in g16_regions(*shape)), w)), w[-1]


def test_range_prover_plan(lib):
    for shape in itertools.product(MS, CS, MAX_CHUNKS, CT_CHUNKS):
        lay, total = bp_plan(lib, *shape)
        assert lay["flag"] == 0                                                                     # whatever the sizes
        check_block(lay, total, bp_regions(*shape), bp_needs(*shape))


def test_groth16_prover_plan(lib):
    for rows, digw, (nv, m), a, c, g2 in itertools.product(ROWS, DIGWS, CIRCUITS, G16_CHUNKS, G16_CHUNKS, G16_CHUNKS):
        shape = (rows, nv, m, digw, a, c, g2)
        lay, total = g16_plan(lib, *shape)
        check_block(lay, total, g16_regions(*shape), g16_needs(*shape))


def test_the_abi_limit_shape_has_no_32_bit_product(lib):
    """2^22 ops per call (ZKP_MAX_BATCH_OPS): the range shape M = 2 * 2^22, C = 2^22; the model's integers are Python's"""
    shape = (2 << 22, 1 << 22, 50, 2)
    lay, total = bp_plan(lib, *shape)
    check_block(lay, total, bp_regions(*shape), bp_needs(*shape))
    for nv, m in (EQUALITY, MEMBERSHIP):
        shape = (1 << 22, nv, m, 16, 40, 40, 40)
        lay, total = g16_plan(lib, *shape)
        check_block(lay, total, g16_regions(*shape), g16_needs(*shape))


def test_range_prover_binder(lib):
    base, marker, wbits = 0x7E0000000000, 0x1100, 16
    # (planned M, C) -> (bound M, C): the range shape, a host job list, and the lists without jobs or without tasks, planned for one
    for (pm, pc), (M, C) in (((130, 65), (130, 65)), ((3, 4096), (3, 4096)), ((1, 5), (0, 5)), ((7, 1), (7, 0))):
        for max_chunks, ct_chunks in itertools.product(MAX_CHUNKS, CT_CHUNKS):
            got = dict(zip(WS_FIELDS, words(lib.emul_pp_bp_bind, WS_WORDS, base, pm, pc, max_chunks, ct_chunks, M, C, wbits, marker)))
            lay, _ = lay_out(bp_regions(pm, pc, max_chunks, ct_chunks))
            for i, field in enumerate(WS_FIELDS):
                if field in WS_BOUND:
                    assert got[field] == base + lay[WS_BOUND[field]], field
                elif field in ("V.M", "T.C"):
                    assert got[field] == (M if field == "V.M" else C)                                # the true counts, not the planned ones
                elif field in ("V.wbits", "T.wbits"):
                    assert got[field] == wbits
                else:
                    assert field in ("V.n", "V.lg", "V.seeds", "V.out", "T.seeds") and got[field] == marker + i, field      # the caller's
            assert got["V.r1"] != got["V.r0"] and len({got[f] for f in WS_BOUND if f.startswith("V.") and f[2:] in WORK_FIELDS}) == len(WORK_FIELDS)


def test_groth16_prover_binder(lib):
    base, marker = 0x7E0000000000, 0x2200
    for rows, digw, (nv, m), (a, c, g2) in itertools.product(ROWS, DIGWS, CIRCUITS, ((1, 7, 40), (40, 1, 7))):
        shape = (rows, nv, m, digw, a, c, g2)
        got = dict(zip(G16_VIEW_FIELDS, words(lib.emul_pp_g16_bind, G16_VIEW_WORDS, base, *shape, marker)))
        lay, _ = lay_out(g16_regions(*shape))
        for i, field in enumerate(G16_VIEW_FIELDS):
            if field in G16_BOUND:
                assert got[field] == base + lay[G16_BOUND[field]], field
            else:
                assert got[field] == marker + i, field                                              # shape, inputs, out and stride: not the binder's
