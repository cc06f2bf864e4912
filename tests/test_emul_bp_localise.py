"""The Bulletproofs batch verifier's localisation pass on the host (no GPU), compiled from the header the kernels use (bp_localise.h):
the planning -- segment bounds in envelopes and in jobs for one, two and a varying number of jobs per envelope, the cap on the number of
segments, suspect flags -> compaction offsets, gather / scatter, the half-of-the-batch rule -- the segment kernel's per-lane steps run one
lane after the other against bigint arithmetic (oracle/py/ristretto.py), and the algebra the pass rests on: the batch-mode steps under
fixed weights, summed per segment, accept the clean segments and refuse exactly those that hold a forged envelope."""
import ctypes
import os
import random

import numpy as np
import pytest

import bp_forge as F
from oracle.py import ristretto as R
from util import P, U64, outputs, workload

QUANTUM, MINIMUM, CAP, TILE_JOBS = 16, 32, 1024, 64                      # pinned: BP_LOC_SEGMENT_QUANTUM, _SEGMENT_MIN, _MAX_SEGMENTS, BP_LOC_TILE_JOBS
SIZES = (64, 2048, 2077, 16384, 65536, 1 << 22)
WANTS = (0, 1, 4, 16, 128)


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build_emul()
    d = os.path.join(ge.EMUL_DIR, "_build")
    loc = ctypes.CDLL(os.path.join(d, "libemul_bp_localise.so"))
    for f in (loc.emul_bp_loc_default_size, loc.emul_bp_loc_segment_of, loc.emul_bp_loc_offsets):
        f.restype = ctypes.c_uint32
    return loc, ctypes.CDLL(os.path.join(d, "libemul_bp.so"))


def _segments(loc, n, want):
    out = (ctypes.c_uint32 * 2)()
    loc.emul_bp_loc_segments(n, want, out)
    return int(out[0]), int(out[1])


def _bounds(loc, n, want, jobs_per, job_base=None):
    size, count = _segments(loc, n, want)
    a = [np.zeros(count, dtype=np.uint32) for _ in range(4)]
    loc.emul_bp_loc_bounds(n, want, jobs_per, P(job_base) if job_base is not None else None, *(P(x) for x in a))
    return (size, count) + tuple(x.astype(np.int64) for x in a)


def test_the_constants_are_the_pinned_ones(libs):
    loc, _ = libs
    c = (ctypes.c_uint32 * 6)()
    loc.emul_bp_loc_constants(c)
    assert list(c) == [CAP, QUANTUM, MINIMUM, TILE_JOBS, 17 * TILE_JOBS, 64] and CAP <= 8192
    # default: about n / 256, a multiple of the quantum, at least the minimum
    assert [loc.emul_bp_loc_default_size(n) for n in (1, 64, 2048, 8192, 8193, 16384, 100000)] == [32, 32, 32, 32, 48, 64, 400]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want", WANTS)
def test_every_envelope_lies_in_exactly_one_segment_and_the_cap_holds(libs, n, want):
    loc, _ = libs
    size, count, lo, hi, jlo, jhi = _bounds(loc, n, want, 2)
    asked = want or loc.emul_bp_loc_default_size(n)
    assert count <= CAP and count == -(-n // size) and size == max(asked, -(-n // CAP))
    assert lo[0] == 0 and hi[-1] == n and (lo[1:] == hi[:-1]).all() and (hi > lo).all()          # a partition of [0, n), in order, none empty
    assert (hi[:-1] - lo[:-1] == size).all() and 0 < hi[-1] - lo[-1] <= size                      # only the last one may be partial
    assert (jlo == 2 * lo).all() and (jhi == 2 * hi).all()                                        # range: two jobs per envelope
    _, _, _, _, tlo, thi = _bounds(loc, n, want, 1)
    assert (tlo == lo).all() and (thi == hi).all()                                                # threshold: one
    for e in (0, 1, min(size, n) - 1, min(size, n - 1), n // 2, n - 2, n - 1):
        s = loc.emul_bp_loc_segment_of(n, want, e)
        assert lo[s] <= e < hi[s]
    if want == 0:
        assert asked % QUANTUM == 0 and asked >= MINIMUM and asked >= n / 256


def test_partial_last_segment_and_the_raised_size(libs):
    loc, _ = libs
    size, count, lo, hi, jlo, jhi = _bounds(loc, 2077, 16, 2)
    assert (size, count) == (16, 130) and (lo[-1], hi[-1], jlo[-1], jhi[-1]) == (2064, 2077, 4128, 4154)
    assert _segments(loc, 1 << 22, 16) == (4096, 1024) and _segments(loc, 1025, 1) == (2, 513) and _segments(loc, 1024, 1) == (1, 1024)


def _consistency_base(n, seed):
    """job_base of n envelopes with k - 1 = 0..7 jobs, zero-job envelopes first and last in segments of 4 among them"""
    rnd = random.Random(seed)
    counts = [rnd.randrange(0, 8) for _ in range(n)]
    for e in (0, 3, 4, 7, 8, 9, 10, 11, n - 1):                               # segment 2 of four has no job at all
        counts[e] = 0
    return np.concatenate(([0], np.cumsum(counts))).astype(np.uint32), counts


def test_job_ranges_with_a_varying_number_of_jobs(libs):
    loc, _ = libs
    n = 203
    base, counts = _consistency_base(n, 5)
    size, count, lo, hi, jlo, jhi = _bounds(loc, n, 4, 1, base)
    assert (size, count) == (4, 51)
    for s in range(count):
        assert jlo[s] == sum(counts[:lo[s]]) and jhi[s] == sum(counts[:hi[s]])
    assert jlo[0] == 0 and jhi[-1] == base[-1] and (jlo[1:] == jhi[:-1]).all()                     # the jobs are partitioned too
    assert jlo[2] == jhi[2]                                                                        # a segment without a job
    assert jhi[0] - jlo[0] == counts[1] + counts[2]                                                # zero-job envelopes at both edges


@pytest.mark.parametrize("kind", ("range", "threshold", "consistency"))
def test_compaction_plan_is_dense_and_order_preserving_and_scatter_inverts_gather(libs, kind):
    loc, _ = libs
    n, want = 2077, 16
    base, jobs_per = None, {"range": 2, "threshold": 1, "consistency": 1}[kind]
    if kind == "consistency":
        n, want = 203, 4
        base, _ = _consistency_base(n, 6)
    size, count, lo, hi, jlo, jhi = _bounds(loc, n, want, jobs_per, base)
    M = int(jhi[-1])
    pb = P(base) if base is not None else None
    rnd = random.Random(n)
    for pattern in ("none", "first", "last", "first+last", "random", "all"):
        sus = np.zeros(count, dtype=np.uint8)
        if pattern in ("first", "first+last"):
            sus[0] = 1
        if pattern in ("last", "first+last"):
            sus[-1] = 1
        if pattern == "random":
            sus[rnd.sample(range(count), max(1, count // 7))] = 1
        if pattern == "all":
            sus[:] = 1
        off = np.zeros(count + 1, dtype=np.uint32)
        m = loc.emul_bp_loc_offsets(n, want, jobs_per, pb, P(sus), P(off))
        lens = np.where(sus == 1, jhi - jlo, 0)
        assert m == lens.sum() == off[-1]
        assert (off[:-1] == np.concatenate(([0], np.cumsum(lens)[:-1]))).all()                     # dense
        batch = np.arange(1000, 1000 + M, dtype=np.uint32)
        compact = np.full(m + 1, 0xFFFFFFFF, dtype=np.uint32)                                     # one word past the end: must stay untouched
        loc.emul_bp_loc_gather(n, want, jobs_per, pb, P(sus), P(off), P(batch), P(compact))
        chosen = np.concatenate([batch[jlo[s]:jhi[s]] for s in range(count) if sus[s]] or [np.zeros(0, dtype=np.uint32)])
        assert (compact[:m] == chosen).all() and compact[m] == 0xFFFFFFFF                          # every suspect job once, in the batch's order
        back = np.zeros(M, dtype=np.uint32)
        loc.emul_bp_loc_scatter(n, want, jobs_per, pb, P(sus), P(off), P(compact), P(back))
        inside = np.repeat(sus, jhi - jlo).astype(bool)
        assert (back[inside] == batch[inside]).all() and not back[~inside].any()                   # the inverse of gather, and nothing else is touched


@pytest.mark.parametrize("M", (128, 4096, 4154, 32768))
def test_half_of_the_batch_rule_at_the_boundary(libs, M):
    loc, _ = libs
    assert loc.emul_bp_loc_whole_batch(M // 2 - 1, M) == 0
    assert loc.emul_bp_loc_whole_batch(M // 2, M) == 1
    assert loc.emul_bp_loc_whole_batch(M, M) == 1 and loc.emul_bp_loc_whole_batch(0, M) == 0
    assert loc.emul_bp_loc_whole_batch(2077, 4153) == 1 and loc.emul_bp_loc_whole_batch(2076, 4153) == 0      # odd M: 2 m >= M


# ---------------------------------------------------------------------------------------------- the kernel's steps, lane by lane
POOL_JOBS = 70


@pytest.fixture(scope="module")
def pool(libs):
    """17 * 70 points k_i B with their Niels rows (index p * 70 + job), k_i known: sum d_i P_i = (sum d_i k_i) B"""
    loc, _ = libs
    n = 17 * POOL_JOBS
    k0, step = 0x1234567 * 2**200 + 99, 2**130 + 12345
    ks, rows = [], np.zeros((n, 32), dtype=np.uint32)
    pt, sb = k0 * R.BASEPOINT, step * R.BASEPOINT
    for i in range(n):
        ks.append((k0 + i * step) % R.L)
        enc = np.frombuffer(pt.encode(), dtype=np.uint32).copy()
        assert loc.emul_bp_loc_niels(P(enc), P(rows[i])) == 1
        pt = pt + sb
    assert (rows[:, 30:] == 0).all() and rows[:, :30].any(axis=1).all()
    return ks, rows


def _window_sum(loc, pool, dig, j_lo, j_hi):
    ks, rows = pool
    enc, run = np.zeros(8, dtype=np.uint32), ctypes.c_uint32(0)
    d = np.array(dig, dtype=np.int16)
    loc.emul_bp_loc_window_sum(POOL_JOBS, P(rows), P(d), j_lo, j_hi, P(enc), ctypes.byref(run))
    want = 0
    for p in range(17):
        for j in range(j_lo, j_hi):
            want += int(dig[p * POOL_JOBS + j]) * ks[p * POOL_JOBS + j]
    assert enc.tobytes() == ((want % R.L) * R.BASEPOINT).encode()
    return run.value


EDGE_DIGITS = (0, 1, -1, 31, -31, 32, -32, 1023, -1023, 1024, -1024, 33, -992, 2, 512)


@pytest.mark.parametrize("jobs", (1, 2, TILE_JOBS - 1, TILE_JOBS, TILE_JOBS + 1, POOL_JOBS))
def test_window_sum_of_a_segment_equals_the_bigint_sum(libs, pool, jobs):
    """segments of one job, one below, at and one above the tile's capacity; digits outside [j_lo, j_hi) belong to other segments"""
    loc, _ = libs
    rnd = random.Random(jobs)
    dig = [rnd.choice(EDGE_DIGITS) if rnd.random() < 0.3 else rnd.randrange(-1024, 1025) for _ in range(17 * POOL_JOBS)]
    j_lo = 0 if jobs == POOL_JOBS else 3
    run = _window_sum(loc, pool, dig, j_lo, j_lo + jobs)
    assert 0 < run <= 17 * min(jobs, TILE_JOBS)


@pytest.mark.parametrize("d", [x for x in EDGE_DIGITS if x])
def test_window_sum_of_a_lone_point_and_of_one_digit_everywhere(libs, pool, d):
    loc, _ = libs
    lone = [0] * (17 * POOL_JOBS)
    lone[5 * POOL_JOBS + 9] = d
    lone[5 * POOL_JOBS + 8] = lone[5 * POOL_JOBS + 10] = 77                  # the neighbours' digits, outside the segment
    assert _window_sum(loc, pool, lone, 9, 10) == 1
    same = [d] * (17 * POOL_JOBS)                                             # every point in the same one or two runs
    assert _window_sum(loc, pool, same, 0, TILE_JOBS + 1) == 17 * TILE_JOBS


def test_window_sum_of_nothing_is_the_identity(libs, pool):
    loc, _ = libs
    assert _window_sum(loc, pool, [0] * (17 * POOL_JOBS), 0, POOL_JOBS) == 0
    assert _window_sum(loc, pool, [5] * (17 * POOL_JOBS), 7, 7) == 0           # a segment without a job


# ---------------------------------------------------------------------------------------------- the algebra
def test_segment_checks_under_the_batch_s_weights_refuse_exactly_the_segments_with_a_forged_envelope(libs):
    loc, bp = libs
    n, size = 13, 4                                                           # segments [0,4) [4,8) [8,12) [12,13): the last one partial
    v, mn, mx, seeds = workload(n, 41)
    out, lens, st = outputs(n)
    assert bp.emul_prove_range_batch(U64(n), P(v), P(mn), P(mx), P(seeds), P(out), U64(1478), P(lens), P(st), 128) == 0
    envs = [out[i].tobytes() for i in range(n)]
    rnd = random.Random(7)
    weights = np.frombuffer(bytes(rnd.randrange(1, 256) for _ in range(16 * 2 * n)), dtype=np.uint8).copy()

    def checks(batch):
        buf = np.frombuffer(b"".join(batch), dtype=np.uint8).reshape(n, 1478).copy()
        seg, whole = np.zeros(4, dtype=np.uint8), ctypes.c_uint8(7)
        assert loc.emul_bp_loc_range_checks(U64(n), P(buf), U64(1478), P(lens), P(mn), P(mx), P(weights), size, P(seg), ctypes.byref(whole)) == 4
        return list(seg), whole.value

    assert checks(envs) == ([1, 1, 1, 1], 1)
    forge = lambda i, name: [f for f in F.field_forgeries(envs[i]) if f.name == name][0].env      # noqa: E731
    more = list(envs)
    more[5] = forge(5, "rp_min.a:plus_1")
    more[6] = forge(6, "rp_max.S:plus_B")                                     # a second one in the same segment
    more[12] = forge(12, "rp_max.t_x:neg")                                    # and one in the partial segment
    assert checks(more) == ([1, 0, 1, 0], 0)
    # opposite errors in two copies of one envelope, in one segment and in two: the weights differ per job, nothing cancels; beside them a
    # rule-refused envelope (an identity point), which never enters a sum: its segment stands
    name, plus, minus = F.opposite_pairs(envs[9])[0]
    pair = list(envs); pair[9], pair[10] = plus, minus
    pair[0] = forge(0, "rp_min.A:identity")
    assert checks(pair) == ([1, 1, 0, 1], 0)
    pair = list(envs); pair[9], pair[2] = plus, minus
    same_bounds = mn[9] == mn[2] and mx[9] == mx[2]
    assert same_bounds and checks(pair) == ([0, 1, 0, 1], 0)
