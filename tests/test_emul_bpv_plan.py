"""The workspace plan of the Bulletproofs verifier's host path on the host (no GPU): bpv_plan_jobs, bpv_plan_batch, bpv_plan_segments,
bpv_plan_compact and bpv_bind_jobs of libzkp_amd/csrc/bpv_plan.h, compiled from the header the library uses (tests/emul/emul_bpv_plan.cpp),
against a model written here from the header's comment block (the regions of every block in take order, their byte formulas) and, for what
every array needs, from the field comments of VfyView, RlcView (bp_verify.h) and ReduceView (bp_steps.h).  A wrong size or a forgotten
region in the plan is an out-of-bounds device write; nothing but a GPU fault showed one before."""
import ctypes
import itertools
import os

import numpy as np
import pytest

VP_NUM, VS_NUM, NBASE, DIGW, GE_W = 17, 17, 130, 13, 40
RLC_NWIN, RLC_NBUCKET, RLC_NSEG, RLC_NIELS_W = 24, 1024, 32, 32
JOB_WORDS = 18
JOB_NAMES = ("poff", "voff", "kind", "lgn", "bad", "pts", "scal", "digits", "vscal", "partial", "sums", "enc", "tcb")          # take order
CHECK_NAMES = ("rho", "fterm", "count", "niels", "dig", "start", "cursor", "sorted", "bucket", "seg", "dig1", "part1", "sum1", "result")
VIEW_FIELDS = ("M", "in", "proof_off", "venc_off", "kind", "lgn", "bad", "pts", "scal", "digits", "vscal", "partial", "var_chunk0", "table", "wbits", "rho", "fterm",
               "job_base", "env_bad")
BOUND = {"proof_off": "poff", "venc_off": "voff", "kind": "kind", "lgn": "lgn", "bad": "bad", "pts": "pts", "scal": "scal", "digits": "digits", "vscal": "vscal",
         "partial": "partial"}                                                                                                 # view field -> region

NS, MS, NCHUNKS, NCHUNKS1, COUNTS = (1, 3, 2048), (0, 1, 2, 17, 4095, 4096), (1, 3, 50), (1, 7), (1, 13, 1024)


def pad256(x):
    return (x + 255) & ~255


# ---- the model: the header's comment, region by region
def job_regions(M, nchunks):
    return [("poff", 8 * M), ("voff", 8 * M), ("kind", M), ("lgn", M), ("bad", 4 * M), ("pts", VP_NUM * GE_W * 4 * M), ("scal", VS_NUM * 32 * M),
            ("digits", NBASE * DIGW * 4 * M), ("vscal", VP_NUM * 32 * M), ("partial", (nchunks + VP_NUM) * GE_W * 4 * M), ("sums", GE_W * 4 * M), ("enc", 32 * M), ("tcb", 4)]


def batch_regions(n, Mw, nchunks, batch_mode, nchunks1):
    N = VP_NUM * Mw
    regions = [("job_base", 4 * (n + 1)), ("env_bad", 4 * n)] + job_regions(Mw, nchunks)
    if batch_mode:
        regions += [("rho", 32 * Mw), ("fterm", NBASE * 32 * Mw), ("count", RLC_NWIN * (RLC_NBUCKET + 1) * 4), ("niels", N * RLC_NIELS_W * 4), ("dig", RLC_NWIN * N * 2),
                    ("start", RLC_NWIN * (RLC_NBUCKET + 2) * 4), ("cursor", RLC_NWIN * (RLC_NBUCKET + 1) * 4), ("sorted", RLC_NWIN * N * 4),
                    ("bucket", RLC_NWIN * RLC_NBUCKET * GE_W * 4), ("seg", RLC_NWIN * RLC_NSEG * GE_W * 4), ("dig1", NBASE * DIGW * 4), ("part1", nchunks1 * GE_W * 4),
                    ("sum1", GE_W * 4), ("result", 64)]
    return regions


def segment_regions(count, nchunks):
    return [("dig", NBASE * DIGW * 4 * count), ("part", nchunks * GE_W * 4 * count), ("gen", GE_W * 4 * count), ("win", count * RLC_NWIN * GE_W * 4), ("suspect", count)]


def compact_regions(count, Mc, nchunks):
    return [("suspect", count), ("off", 4 * (count + 1))] + job_regions(Mc, nchunks)


def lay_out(regions):
    """offsets and the total of a block whose regions are taken in order, each padded to 256 bytes"""
    off, lay = 0, {}
    for name, size in regions:
        lay[name] = off
        off += pad256(size)
    return lay, off


# ---- what every array needs: the views' field comments, in bytes
def job_needs(M, nchunks):
    words = 4
    return {"poff": 8 * M, "voff": 8 * M, "kind": M, "lgn": M, "bad": 4 * M,                        # [M] of u64, u64, u8, u8, i32
            "pts": 17 * 40 * M * words, "scal": VS_NUM * 8 * M * words,                           # [17][40][M], [VS_NUM][8][M]
            "digits": 130 * DIGW * M * words, "vscal": 17 * 8 * M * words,                        # [130][DIGW][M], [17][8][M]
            "partial": (nchunks + 17) * 40 * M * words,                                           # the layout's chunks, then chunks var_chunk0 + p for 17 points: [40][M] each
            "sums": 40 * M * words, "enc": 8 * M * words, "tcb": 2 * 2}                           # one target: [1][40][rows], [1][8][rows], [1 + 1] of u16


def batch_needs(n, Mw, nchunks, batch_mode, nchunks1):
    needs = dict(job_needs(Mw, nchunks), job_base=4 * (n + 1), env_bad=4 * n)                     # [n + 1], [n]
    if batch_mode:
        N, words = 17 * Mw, 4
        needs.update(rho=8 * Mw * words, fterm=130 * 8 * Mw * words,                              # [8][M], [130][8][M]
                     niels=N * 32 * words, dig=RLC_NWIN * N * 2, count=RLC_NWIN * (RLC_NBUCKET + 1) * words, start=RLC_NWIN * (RLC_NBUCKET + 2) * words,
                     cursor=RLC_NWIN * (RLC_NBUCKET + 1) * words, sorted=RLC_NWIN * N * words, bucket=RLC_NWIN * RLC_NBUCKET * 40 * words,
                     seg=RLC_NWIN * RLC_NSEG * 40 * words,
                     dig1=130 * DIGW * words, part1=nchunks1 * 40 * words, sum1=40 * words, result=9 * words)          # one row; result: [8] and the flag [8]
    return needs


def segment_needs(count, nchunks):
    return {"dig": 130 * DIGW * count * 4, "part": nchunks * 40 * count * 4, "gen": 40 * count * 4, "win": count * RLC_NWIN * 40 * 4, "suspect": count}


def check_block(lay, total, regions, needs, zeroed=()):
    """every region 256-aligned, inside [0, total), as large as its array needs, disjoint from the others; total = the sum of the padded
    sizes; every (lo, hi, names) of `zeroed` is exactly the union of its regions, contiguous, and touches no other region"""
    m_lay, m_total = lay_out(regions)
    assert {name: lay[name] for name in m_lay} == m_lay and total == m_total == sum(pad256(size) for _, size in regions)
    spans = sorted((lay[name], pad256(size), name) for name, size in regions)
    end = 0
    for off, padded, name in spans:
        assert off % 256 == 0 and off >= end and off + padded <= total, (name, off, end, total)
        assert padded >= needs[name], (name, padded, needs[name])
        end = off + padded
    for lo, hi, names in zeroed:
        inside = [s for s in spans if s[0] < hi and s[0] + s[1] > lo]
        assert sorted(s[2] for s in inside) == sorted(names) and lo == inside[0][0] and hi == inside[-1][0] + inside[-1][1], (lo, hi, inside)
        assert all(a[0] + a[1] == b[0] for a, b in zip(inside, inside[1:]))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_bpv_plan.so"))
    u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    L.emul_bpv_constants.argtypes = [vp]
    L.emul_bpv_plan_batch.argtypes = [u64, u32, u32, ctypes.c_int, u32, vp]
    L.emul_bpv_plan_segments.argtypes = [u32, u32, vp]
    L.emul_bpv_plan_compact.argtypes = [u32, u32, u32, vp]
    L.emul_bpv_bind.argtypes = [u64, u64, u32, u32, u64, vp, vp]
    c = np.zeros(10, dtype=np.uint32)
    L.emul_bpv_constants(c.ctypes.data)
    assert c.tolist() == [VP_NUM, VS_NUM, NBASE, DIGW, GE_W, RLC_NWIN, RLC_NBUCKET, RLC_NSEG, RLC_NIELS_W, JOB_WORDS]
    return L


def words(call, count, *args):
    out = np.full(count + 1, 0x5151, dtype=np.uint64)
    call(*args, out.ctypes.data)
    assert out[count] == 0x5151
    return [int(x) for x in out[:count]]


def jobs_of(w):
    """a job-array plan's words -> (nchunks, chunk table, offsets by region, the zeroed range)"""
    names = ("poff", "voff", "kind", "lgn", "bad", "pts", "scal", "zero0", "digits", "vscal", "zero1", "partial", "sums", "enc", "tcb")
    lay = dict(zip(names, w[3:]))
    return w[0], w[1:3], lay, (lay.pop("zero0"), lay.pop("zero1"))


def plan_batch(L, n, Mw, nchunks, batch_mode, nchunks1):
    w = words(L.emul_bpv_plan_batch, 2 + JOB_WORDS + 16, n, Mw, nchunks, int(batch_mode), nchunks1)
    nch, table, lay, zero = jobs_of(w[2:2 + JOB_WORDS])
    lay.update(job_base=w[0], env_bad=w[1])
    check = dict(zip(("rho", "fterm", "count", "rzero1", "niels", "dig", "start", "cursor", "sorted", "bucket", "seg", "dig1", "part1", "sum1", "result", "total"), w[2 + JOB_WORDS:]))
    return nch, table, lay, zero, check


def plan_compact(L, count, Mc, nchunks):
    w = words(L.emul_bpv_plan_compact, 2 + JOB_WORDS + 1, count, Mc, nchunks)
    nch, table, lay, zero = jobs_of(w[2:2 + JOB_WORDS])
    lay.update(suspect=w[0], off=w[1])
    return nch, table, lay, zero, w[-1]


@pytest.mark.parametrize("batch_mode", (False, True))
def test_batch_block(lib, batch_mode):
    for n, M, nchunks, nchunks1 in itertools.product(NS, MS, NCHUNKS, NCHUNKS1):
        Mw = max(M, 1)                                                                              # the M == 0 call still lays out one job
        nch, table, lay, zero, check = plan_batch(lib, n, Mw, nchunks, batch_mode, nchunks1)
        assert nch == nchunks and table == [0, nchunks + VP_NUM]                                    # the per-job sum: the fixed chunks and the 17 proof-point products
        total = check.pop("total")
        rzero1 = check.pop("rzero1")
        zeroed = [(zero[0], zero[1], ("digits", "vscal"))]
        if batch_mode:
            lay.update(check)
            zeroed.append((check["fterm"], rzero1, ("fterm", "count")))
        else:
            assert not any(check.values()) and rzero1 == 0                                          # the check's regions take no space ...
            assert total == lay_out(batch_regions(n, Mw, nchunks, False, nchunks1))[1]              # ... (the total is that of the other regions)
        check_block(lay, total, batch_regions(n, Mw, nchunks, batch_mode, nchunks1), batch_needs(n, Mw, nchunks, batch_mode, nchunks1), zeroed)


def test_localisation_block_both_shapes(lib):
    for count, nchunks in itertools.product(COUNTS, NCHUNKS):
        w = words(lib.emul_bpv_plan_segments, 6, count, nchunks)
        seg_lay, seg_total = dict(zip(("dig", "part", "gen", "win", "suspect"), w)), w[5]
        check_block(seg_lay, seg_total, segment_regions(count, nchunks), segment_needs(count, nchunks))
        for M, cchunks in itertools.product(MS, NCHUNKS):
            for Mc in sorted({1, 16, M - 1} - {0, -1}):
                nch, table, lay, zero, total = plan_compact(lib, count, Mc, cchunks)
                assert nch == cchunks and table == [0, cchunks + VP_NUM]
                needs = dict(job_needs(Mc, cchunks), suspect=count, off=4 * (count + 1))                # [count], [count + 1]
                check_block(lay, total, compact_regions(count, Mc, cchunks), needs, [(zero[0], zero[1], ("digits", "vscal"))])
                # both shapes lie over the same buffer from offset 0: the buffer needed is the larger total, and it holds either shape
                assert min(seg_lay.values()) == 0 and min(lay.values()) == 0
                need = max(seg_total, total)
                assert need == max(lay_out(segment_regions(count, nchunks))[1], lay_out(compact_regions(count, Mc, cchunks))[1])
                assert all(seg_lay[name] + size <= need for name, size in segment_regions(count, nchunks))
                assert all(lay[name] + size <= need for name, size in compact_regions(count, Mc, cchunks))


def test_compact_job_arrays_have_the_batch_blocks_sizes(lib):
    """the same function carves both: for the same (M, nchunks) every job array of the compact shape is as large as the batch block's"""
    def sizes(lay, total):
        order = sorted(JOB_NAMES, key=lambda name: lay[name])
        assert order == list(JOB_NAMES)
        return [(lay[b] if b else total) - lay[a] for a, b in zip(order, order[1:] + [None])]
    for M, nchunks in itertools.product(MS[1:], NCHUNKS):
        _, _, blay, _, check = plan_batch(lib, 3, M, nchunks, False, 1)
        _, _, clay, _, ctotal = plan_compact(lib, 13, M, nchunks)
        assert sizes(blay, check["total"]) == sizes(clay, ctotal) == [pad256(size) for _, size in job_regions(M, nchunks)]


def test_binder(lib):
    base, marker = 0x7E0000000000, 0x1100
    for M, nchunks, lead in itertools.product(MS[1:], NCHUNKS, (0, 1, 4096)):
        plan = np.zeros(JOB_WORDS, dtype=np.uint64)
        view = np.full(len(VIEW_FIELDS) + 1, 0x5151, dtype=np.uint64)
        lib.emul_bpv_bind(base, lead, M, nchunks, marker, plan.ctypes.data, view.ctypes.data)
        assert view[len(VIEW_FIELDS)] == 0x5151
        nch, _, lay, _ = jobs_of([int(x) for x in plan])
        assert lay == {name: off + pad256(lead) for name, off in lay_out(job_regions(M, nchunks))[0].items()}
        got = dict(zip(VIEW_FIELDS, (int(x) for x in view)))
        for i, field in enumerate(VIEW_FIELDS):
            if field in BOUND:
                assert got[field] == base + lay[BOUND[field]], field
            elif field == "var_chunk0":
                assert got[field] == nchunks == nch
            else:
                assert got[field] == marker + i, field                                              # M, in, table, wbits, rho, fterm, job_base, env_bad: not the binder's
