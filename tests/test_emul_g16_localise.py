"""The Groth16 batch verifier's localisation pass on the host (no GPU): the planning of g16_localise.h -- segment bounds, the cap on the
number of segments, suspect flags -> compaction offsets, the half-of-the-batch rule -- compiled from the header the kernels use, and the
algebra it rests on: the batch check of g16_rlc.h over a sub-range, under the batch's own weights, accepts a segment of valid envelopes and
refuses exactly the segments that hold a tampered one."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle.py import groth16 as g

SIZES = (8193, 8237, 16384, 65536, 1 << 22)
SEGMENTS = (64, 256, 1024)


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build_emul()
    d = os.path.join(ge.EMUL_DIR, "_build")
    loc = ctypes.CDLL(os.path.join(d, "libemul_g16_localise.so"))
    for f in (loc.emul_g16_loc_default_size, loc.emul_g16_loc_max_segments, loc.emul_g16_loc_segment_of, loc.emul_g16_loc_offsets):
        f.restype = ctypes.c_uint32
    return loc, ctypes.CDLL(os.path.join(d, "libemul_g16.so"))


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _vk_args(pk):
    """a key's verifying part as raw little-endian words: alpha, beta, gamma, delta, n_ic, ic (the arguments of emul_g16_rlc)"""
    words = lambda vals: [(v >> (32 * i)) & 0xFFFFFFFF for v in vals for i in range(8)]  # noqa: E731
    g1w = lambda pt: words(pt)  # noqa: E731
    g2w = lambda pt: words((pt[0][0], pt[0][1], pt[1][0], pt[1][1]))  # noqa: E731
    A = lambda ws: (ctypes.c_uint32 * len(ws))(*ws)  # noqa: E731
    ic = sum((g1w(p) for p in pk.gamma_abc_g1), [])
    return A(g1w(pk.alpha_g1)), A(g2w(pk.beta_g2)), A(g2w(pk.gamma_g2)), A(g2w(pk.delta_g2)), len(pk.gamma_abc_g1), A(ic)


def _segments(loc, n, want):
    out = (ctypes.c_uint32 * 2)()
    loc.emul_g16_loc_segments(n, want, out)
    return int(out[0]), int(out[1])


def _bounds(loc, n, want):
    size, count = _segments(loc, n, want)
    lo, hi = np.zeros(count, dtype=np.uint32), np.zeros(count, dtype=np.uint32)
    loc.emul_g16_loc_bounds(n, want, P(lo), P(hi))
    return size, count, lo.astype(np.int64), hi.astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want", SEGMENTS + (0,))
def test_every_envelope_lies_in_exactly_one_segment_and_there_are_at_most_8192(libs, n, want):
    loc, _ = libs
    cap = loc.emul_g16_loc_max_segments()
    assert cap == 8192
    size, count, lo, hi = _bounds(loc, n, want)
    asked = want or loc.emul_g16_loc_default_size(n)
    assert count <= cap and count == -(-n // size)
    # the size is the one asked for unless that would make more than 8192 segments; then it is the least size that does not
    assert size == max(asked, -(-n // cap))
    assert lo[0] == 0 and hi[-1] == n and (lo[1:] == hi[:-1]).all() and (hi > lo).all()          # contiguous, in order, none empty: a partition of [0, n)
    assert (hi[:-1] - lo[:-1] == size).all() and 0 < hi[-1] - lo[-1] <= size                      # only the last one may be partial
    for j in (0, 1, size - 1, size, n // 2, n - 2, n - 1):
        s = loc.emul_g16_loc_segment_of(n, want, j)
        assert lo[s] <= j < hi[s]
    if want == 0:
        assert asked % 64 == 0 and asked >= 64 and asked >= n / 256


def test_partial_last_segment(libs):
    loc, _ = libs
    size, count, lo, hi = _bounds(loc, 8237, 64)
    assert (size, count) == (64, 129) and (lo[-1], hi[-1]) == (8192, 8237)
    assert _segments(loc, 1 << 22, 64) == (512, 8192)
    assert _segments(loc, 16384, 64) == (64, 256) and _segments(loc, 16384, 1024) == (1024, 16)


@pytest.mark.parametrize("n,want", [(8237, 64), (16384, 256), (65536, 1024), (8193, 64)])
def test_compaction_plan_is_dense_and_order_preserving_and_scatter_inverts_gather(libs, n, want):
    loc, _ = libs
    size, count, lo, hi = _bounds(loc, n, want)
    rnd = random.Random(n + want)
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
        m = loc.emul_g16_loc_offsets(n, want, P(sus), P(off))
        lens = np.where(sus == 1, hi - lo, 0)
        assert m == lens.sum() == off[-1]
        assert (off[:-1] == np.concatenate(([0], np.cumsum(lens)[:-1]))).all()                     # dense: each suspect segment starts where the one before ended
        batch = np.arange(1000, 1000 + n, dtype=np.uint32)
        compact = np.full(m + 1, 0xFFFFFFFF, dtype=np.uint32)                                     # one word past the end: must stay untouched
        loc.emul_g16_loc_gather(n, want, P(sus), P(off), P(batch), P(compact))
        chosen = np.concatenate([batch[lo[s]:hi[s]] for s in range(count) if sus[s]] or [np.zeros(0, dtype=np.uint32)])
        assert (compact[:m] == chosen).all() and compact[m] == 0xFFFFFFFF                          # every suspect envelope once, in the batch's order
        back = np.zeros(n, dtype=np.uint32)
        loc.emul_g16_loc_scatter(n, want, P(sus), P(off), P(compact), P(back))
        inside = np.repeat(sus, hi - lo).astype(bool)
        assert (back[inside] == batch[inside]).all() and not back[~inside].any()                   # scatter is the inverse of gather and touches nothing else


@pytest.mark.parametrize("n", (8194, 16384, 65536))
def test_half_of_the_batch_rule_at_the_boundary(libs, n):
    loc, _ = libs
    assert loc.emul_g16_loc_whole_batch(n // 2 - 1, n) == 0
    assert loc.emul_g16_loc_whole_batch(n // 2, n) == 1
    assert loc.emul_g16_loc_whole_batch(n, n) == 1
    assert loc.emul_g16_loc_whole_batch(0, n) == 0
    assert loc.emul_g16_loc_whole_batch(4119, 8237) == 1 and loc.emul_g16_loc_whole_batch(4118, 8237) == 0          # odd n: 2 m >= n


def test_segment_checks_under_the_batch_s_weights_refuse_exactly_the_segments_with_a_tampered_envelope(libs):
    """g16_rlc_check (the lane-per-chain form of what the kernels compute) over sub-ranges of one batch, each with its own slice of the batch's
    weights: the all-valid segments are accepted, the segments that hold an envelope under another envelope's commitment are refused, and so is
    the batch as a whole -- a segment's check involves only its own weights, so the weights of the failed batch check serve again."""
    _, lib = libs
    SS = bytes(range(32))
    rnd = random.Random(17)
    pk = g.equality_key(SS)
    va = _vk_args(pk)
    distinct = []
    for k in range(3):
        seed = bytes([k + 11]) * 32
        v = rnd.randrange(2**64)
        cm = g.commit_value_snark(v)
        distinct.append(g.envelope(2, g.prove_with_trapdoor(pk, g.equality_circuit(v, v, int.from_bytes(cm, "little")), g.draw_fr(seed, 0x47313600, 0), g.draw_fr(seed, 0x47313600, 1)), cm))
    n, size = 14, 4                                                                                # segments [0,4) [4,8) [8,12) [12,14): the last one partial
    envs = [distinct[i % 3] for i in range(n)]
    bad = (5, 12, 13)                                                                              # one in segment 1, two in the partial segment 3
    for i in bad:
        envs[i] = envs[i][:266] + envs[i + 1 if i + 1 < n else 0][266:]                            # a valid proof under its neighbour's commitment
        assert envs[i][266:] != distinct[i % 3][266:]
    buf = np.frombuffer(b"".join(envs), dtype=np.uint8).copy()
    lens = np.full(n, 298, dtype=np.uint32)
    rho = np.array([rnd.randrange(1, 2**32) for _ in range(4 * n)], dtype=np.uint32)

    def check(lo, hi):
        return lib.emul_g16_rlc(0, hi - lo, P(buf[298 * lo:]), 298, P(lens[lo:]), P(rho[4 * lo:]), *va)

    assert check(0, n) == 0
    verdicts = [check(lo, min(lo + size, n)) for lo in range(0, n, size)]
    assert verdicts == [1, 0, 1, 0]
    assert [s for s, v in enumerate(verdicts) if v == 0] == sorted({i // size for i in bad})
    assert check(0, 5) == 1 and check(0, 6) == 0 and check(6, 12) == 1                             # ranges need not be aligned to anything
