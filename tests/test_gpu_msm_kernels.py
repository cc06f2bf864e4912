"""k_msm_gather<G1Msm | G2Msm | EdGather | EdGatherPrio> and k_sum_t<G1Msm | G2Msm | EdMsm> driven directly through the product's own launchers
(g16_launch_msm, g16_launch_sum, edg_launch_msm in its plain and its raised form, edg_launch_sum; tests/devtier/devtier.hip builds the synthetic views and validates them on the host before anything is launched), at the smallest shapes at
which the kernels can still be wrong, against

    partial(c, row) = acc_init + sum over the steps t of chunk c of sign(d_t) * E[steps[t].x + |d_t| - 1]

in bigint curve arithmetic.  Table entries are distinct known multiples of the generator, so a swapped, late or early entry changes the answer;
every point of a case is therefore a known multiple too and the reference is a sum of small integers looked up in a table of multiples.  The
lazy BN254 additions have no exceptional cases, so before a launch it is asserted -- nothing is filtered -- that no prefix sum of any lane is
the neutral element or +- the entry it is about to take.  The ed25519 formulas are complete: there the same lists run unconditioned, and one
case walks its lanes through the neutral element, acc = entry and acc = -entry on purpose.  Needs no zkp_hip_init, no keys and no generator tables."""
import ctypes

import numpy as np
import pytest

import devtier_cases as DC
from oracle.py import bn254 as BN
from oracle.py import ristretto as RIS

pytestmark = pytest.mark.gpu

NMULT = 4200
ACC_K = 2000              # acc_init = ACC_K * G: with entries <= 300 G and at most 7 steps no prefix sum comes near 0 or an entry


@pytest.fixture(scope="module")
def lib():
    return DC.load()


G1, G2, ED, ED_RAISED = 0, 1, 2, 3        # the `kind` of devtier_msm / devtier_sum; ED_RAISED: the gather instantiation with raised issue priority


class Group:
    """one of the three groups: multiples of its generator by repeated addition (index k = k G; negative k through negation), affine words"""

    def __init__(self, kind):
        self.kind, self.w, self.lazy, self._words = kind, (33 if kind == G2 else 17), kind in (G1, G2), {}
        if kind in (G1, G2):
            c, gen, t = (BN.G2C if kind == G2 else BN.G1C), (BN.G2 if kind == G2 else BN.G1), [None]
            for _ in range(NMULT):
                t.append(c.add_pts(t[-1], gen))
            self.neg = c.neg_pt
        else:
            t = [RIS.IDENTITY]
            for _ in range(NMULT):
                t.append(t[-1] + RIS.BASEPOINT)
            self.neg = lambda p: -p
        self.t = t

    def words(self, k):
        """canonical affine words of k G and the neutral flag"""
        if k not in self._words:
            p = self.t[k] if k >= 0 else self.neg(self.t[-k])
            if self.kind in (G1, G2):
                comps = None if p is None else [p[0][0], p[0][1], p[1][0], p[1][1]] if self.kind == G2 else [p[0], p[1]]
            else:
                zi = pow(p.Z, RIS.P - 2, RIS.P)
                comps = [p.X * zi % RIS.P, p.Y * zi % RIS.P]
                comps = None if comps == [0, 1] else comps
            self._words[k] = [0] * (self.w - 1) + [1] if comps is None else [(x >> (32 * i)) & 0xFFFFFFFF for x in comps for i in range(8)] + [0]
        return self._words[k]


_GROUPS = {}


def group(kind):
    kind = min(kind, ED)
    if kind not in _GROUPS:
        _GROUPS[kind] = Group(kind)
    return _GROUPS[kind]


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def gather(lib, kind, rows, chunk_lens, win_x, table_entries, digit, layout="halves", acc=True, expect_rc=0):
    """One launch.  Step t (global) walks window t % len(win_x), whose first entry is win_x[.]; digit(row, t) is the lane's digit there.
    layout "halves": steps 2j, 2j + 1 share digit-word row j (low half, high half); "rows": a word row per step, the half alternating in
    threes, the other half holding another valid digit so that a read of the wrong half changes the answer and stays inside the table."""
    G = group(kind)
    nsteps = sum(chunk_lens)
    step0 = np.cumsum([0] + list(chunk_lens)).astype(np.uint32)
    place = [(t // 2, t % 2) if layout == "halves" else (t, (t // 3) % 2) for t in range(nsteps)]
    digit_rows = max([p[0] for p in place], default=0) + 1
    steps = np.array([[win_x[t % len(win_x)], (place[t][0] << 1) | place[t][1]] for t in range(nsteps)], dtype=np.uint32).reshape(-1, 2)
    d = np.array([[digit(r, t) for r in range(rows)] for t in range(nsteps)], dtype=np.int64).reshape(nsteps, rows)
    dig16 = np.zeros((digit_rows, 2, rows), dtype=np.int64)
    dig16[:, :, :] = 1                                                     # the unused halves: entry 0 of a window, always populated below
    for t in range(nsteps):
        dig16[place[t][0], place[t][1]] = d[t]
    words = ((dig16[:, 0] & 0xFFFF) | ((dig16[:, 1] & 0xFFFF) << 16)).astype(np.uint32)
    # the populated entries: what the digits select, and entry 0 of every window for the filler halves; each a distinct multiple of G
    used = sorted({int(steps[t, 0]) + abs(int(x)) - 1 for t in range(nsteps) for x in d[t] if x} | {int(x) for x in win_x})
    mult = {slot: 1 + i for i, slot in enumerate(used)}
    if expect_rc:
        used = [s for s in used if s < table_entries]                      # a view meant to be refused: only what fits is populated
    assert len(used) <= 300 and all(0 <= s < table_entries for s in used)
    # the reference, and the condition under which the lazy additions are exact: asserted over every lane, nothing skipped
    k0 = ACC_K if acc else 0
    mult_of = lambda slot: mult.get(slot, 1)  # noqa: E731
    want = np.zeros((len(chunk_lens), rows), dtype=np.int64)
    for c in range(len(chunk_lens)):
        for r in range(rows):
            k = k0
            for t in range(step0[c], step0[c + 1]):
                x = int(d[t, r])
                if x:
                    e = mult_of(int(steps[t, 0]) + abs(x) - 1)
                    assert not G.lazy or (k != 0 and k != e and k != -e), "a prefix sum meets +- the entry or the neutral element"
                    k += e if x > 0 else -e
                    assert not G.lazy or k != 0
            want[c, r] = k
    pts = np.array([G.words(mult[s])[:-1] for s in used], dtype=np.uint32)
    slots = np.array(used, dtype=np.uint64)
    acc_w = np.array(G.words(ACC_K)[:-1], dtype=np.uint32) if acc else None
    out = np.zeros((len(chunk_lens), rows, G.w), dtype=np.uint32)
    lib.devtier_msm.restype = ctypes.c_int
    rc = lib.devtier_msm(ctypes.c_int(kind), ctypes.c_uint32(rows), ctypes.c_uint32(len(chunk_lens)), ctypes.c_uint32(nsteps), ptr(steps), ptr(step0),
                               ptr(words), ctypes.c_uint32(digit_rows), ptr(pts), ptr(slots), ctypes.c_uint32(len(used)), ctypes.c_uint64(table_entries), ptr(acc_w), ptr(out))
    assert rc == expect_rc, "devtier_msm returned %d" % rc
    if rc:
        return
    cache = {}
    for c in range(len(chunk_lens)):
        for r in range(rows):
            k = int(want[c, r])
            if k not in cache:
                cache[k] = G.words(k)
            assert out[c, r].tolist() == cache[k], "chunk %d (%d steps) row %d: not %d G" % (c, chunk_lens[c], r, k)


def lanes_differ(nent):
    return lambda r, t: ((r * 5 + t * 3) % (2 * nent + 1)) - nent           # every digit of [-nent, nent], zero included, neighbours different


KINDS = [pytest.param(G1, id="G1"), pytest.param(G2, id="G2"), pytest.param(ED, id="Ed"), pytest.param(ED_RAISED, id="EdRaised")]
SUM_KINDS = KINDS[:3]
TINY = dict(win_x=[4 * w for w in range(6)], table_entries=24)             # nent = 4, six windows


@pytest.mark.parametrize("kind", KINDS)
def test_chunk_lengths_against_the_lead_and_the_look_ahead(lib, kind):
    """0, 1, 2, 3, 4, 5 and 7 steps in one launch: prologue only, prologue = lead, lead + 1, lead + 2 (the digit-word look-ahead), steady
    state with tail; the 0-step chunk stores acc_init"""
    gather(lib, kind, 65, [0, 1, 2, 3, 4, 5, 7], digit=lanes_differ(4), **TINY)
    gather(lib, kind, 65, [7, 5, 4, 3, 2, 1, 0], digit=lanes_differ(4), layout="rows", **TINY)


@pytest.mark.parametrize("kind", KINDS)
def test_zero_step_chunks_without_acc_init_store_the_neutral_element(lib, kind):
    gather(lib, kind, 65, [0, 0, 0], digit=lambda r, t: 0, acc=False, **TINY)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nchunks", [1, 3, 8, 9])
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 255, 256, 257])
def test_rows_and_groups(lib, kind, rows, nchunks):
    """one and two row groups, the last one a lane wide; 2, 6, 16 and 18 workgroups at two groups: the `linear >= nblocks` exit and the
    per-XCD mapping (a workgroup that took another's chunk or group stores another lane's sum)"""
    gather(lib, kind, rows, [3 + (c % 3) for c in range(nchunks)], digit=lanes_differ(4), **TINY)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["all_zero", "zero_every_other", "plus_nent", "minus_nent", "halves", "row_per_step"])
def test_digit_patterns(lib, kind, name):
    digit = {"all_zero": lambda r, t: 0,
             "zero_every_other": lambda r, t: 0 if (t + r) % 2 else 1 + (r + t) % 4,      # skipped fetches rotate through the prefetch slots
             "plus_nent": lambda r, t: 4, "minus_nent": lambda r, t: -4,
             "halves": lanes_differ(4), "row_per_step": lanes_differ(4)}[name]
    gather(lib, kind, 65, [5, 7, 3], digit=digit, layout="rows" if name == "row_per_step" else "halves", **TINY)


@pytest.mark.parametrize("kind", [KINDS[0], KINDS[2]])
def test_the_most_negative_digit_selects_the_last_entry_of_a_window(lib, kind):
    """int16 -32768 at nent = 32768: entry nent - 1 (one G1 case, one EdGather case)"""
    nent = 32768
    digit = lambda r, t: -32768 if (r + t) % 3 == 0 else (32767 if (r + t) % 3 == 1 else -1 - (r % 5))  # noqa: E731
    gather(lib, kind, 65, [4, 3], win_x=[0, nent], table_entries=2 * nent, digit=digit)


@pytest.mark.parametrize("kind", KINDS)
def test_byte_offsets_into_the_table_beyond_4_gib(lib, kind):
    """a table allocation just over 4 GiB, never cleared; windows in its first and its last slots"""
    entries = (1 << (26 if kind == G1 else 25)) + 8          # 64-byte entries for G1, 128-byte slots for G2 and ed25519
    gather(lib, kind, 65, [4, 3], win_x=[0, entries - 4], table_entries=entries, digit=lanes_differ(4))


@pytest.mark.parametrize("kind", KINDS[2:])
def test_ed25519_chunks_pass_through_the_neutral_element_and_through_acc_equal_to_plus_or_minus_the_entry(lib, kind):
    """no acc_init, one window: a lane's digits d, -d, d, d, -d, -d, -d take it from the neutral element to E, back to it (acc = E takes -E),
    to E, to 2E (acc = E takes E), and down through the neutral element to -E; the complete formulas must give every one of them"""
    seq = [1, -1, 1, 1, -1, -1, -1]
    digit = lambda r, t: seq[t % 7] * (1 + r % 4)  # noqa: E731
    gather(lib, kind, 65, [7, 2, 3, 5], win_x=[0], table_entries=4, digit=digit, acc=False)
    gather(lib, kind, 65, [7, 2, 3, 5], win_x=[0], table_entries=4, digit=digit, acc=False, layout="rows")


def test_a_view_that_leaves_the_table_or_the_digit_buffer_is_refused_before_launch(lib):
    gather(lib, G1, 3, [2], win_x=[22], table_entries=24, digit=lambda r, t: 4, expect_rc=-5)       # entry 25 of 24
    gather(lib, ED, 3, [2], win_x=[22], table_entries=24, digit=lambda r, t: 4, expect_rc=-5)
    G = group(G1)
    one = np.array(G.words(1)[:-1], dtype=np.uint32)
    slot, out = np.array([0], dtype=np.uint64), np.zeros((1, 1, 17), dtype=np.uint32)
    steps, step0, words = np.array([[0, 5 << 1]], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.ones((2, 1), dtype=np.uint32)
    rc = lib.devtier_msm(0, 1, 1, 1, ptr(steps), ptr(step0), ptr(words), 2, ptr(one), ptr(slot), 1, ctypes.c_uint64(4), ptr(one), ptr(out))
    assert rc == -4                                                                                    # digit-word row 5 of 2


# ------------------------------------------------------------------------------------------------ k_sum_t
def partial_k(c, r):
    """the multiple of G that partial (chunk c, row r) holds: small, of either sign, neutral now and then, and in row 0 two equal and two
    opposite partials where the tree (and the slice loop of a long target) joins them"""
    if (c * (r + 2)) % 11 == 3:
        return 0
    k = 1 + (c * 7 + r * 3) % 37
    return -k if (c + r) % 5 == 0 else k


def sums(lib, kind, rows, begin, end, nchunks, corr, special=()):
    G = group(kind)
    ks = np.array([[partial_k(c, r) for r in range(rows)] for c in range(nchunks)], dtype=np.int64)
    for c, r, k in special:
        ks[c, r] = k
    part = np.array([[G.words(int(ks[c, r])) for r in range(rows)] for c in range(nchunks)], dtype=np.uint32)
    nt = len(begin) - 1
    ck = [(-3 - 2 * t) if t % 3 else 0 for t in range(nt)] if corr else None     # a neutral correction among them
    cw = np.array([G.words(k) for k in ck], dtype=np.uint32) if corr else None
    b16 = np.array(begin, dtype=np.uint16)
    e16 = np.array(end, dtype=np.uint16) if end is not None else None
    out = np.zeros((nt, rows, G.w), dtype=np.uint32)
    lib.devtier_sum.restype = ctypes.c_int
    rc = lib.devtier_sum(ctypes.c_int(kind), ctypes.c_uint32(rows), ctypes.c_uint32(nchunks), ctypes.c_uint32(nt), ptr(b16), ptr(e16), ptr(part), ptr(cw), ptr(out))
    assert rc == 0, "devtier_sum returned %d" % rc
    for t in range(nt):
        c1 = end[t] if end is not None else begin[t + 1]
        for r in range(rows):
            k = int(ks[begin[t]:c1, r].sum()) + (ck[t] if corr else 0)
            assert out[t, r].tolist() == G.words(k), "target %d (chunks %d..%d) row %d: not %d G" % (t, begin[t], c1, r, k)


# chunks per target against the slices per row (32 for BN254, 8 for ed25519): fewer chunks than slices, one fewer, exactly as many, one more,
# two rounds and one
CHUNKS_PER_TARGET = {G1: [1, 2, 31, 32, 33, 65], G2: [1, 2, 31, 32, 33, 65], ED: [1, 7, 8, 9, 17]}


@pytest.mark.parametrize("kind", SUM_KINDS)
@pytest.mark.parametrize("corr", [False, True], ids=["no_corr", "corr"])
@pytest.mark.parametrize("rows", [1, 7, 8, 9, 33])
def test_sum_over_tiling_targets(lib, kind, rows, corr):
    per = CHUNKS_PER_TARGET[kind]
    begin = np.cumsum([0] + per).tolist()
    slices = 8 if kind == ED else 32
    full, long = begin[per.index(slices)], begin[len(per) - 1]      # the target with one chunk per slice; the longest target
    special = [(full + 0, 0, 9), (full + slices // 2, 0, 9),            # equal partials meet in the tree's first level: the doubling branch, 2P
               (full + 1, 0, 12), (full + 1 + slices // 2, 0, -12),     # opposite partials: the infinity branch, O, which the next level then takes as an operand
               (long + 0, 0, 5), (long + slices, 0, 5)]                 # equal partials in one slice's loop
    if kind != ED:
        special += [(begin[1], 0, 4), (begin[1] + 1, 0, -4)]            # a target whose two chunks cancel: the sum is the neutral element
    sums(lib, kind, rows, begin, None, begin[-1], corr, special)


@pytest.mark.parametrize("kind", SUM_KINDS)
def test_sum_over_overlapping_target_ranges(lib, kind):
    """target_chunk_end: ranges that overlap, one inside another, an empty one, one that ends at the last chunk"""
    begin, end = [0, 0, 10, 5, 40, 7, 0], [40, 33, 75, 6, 75, 7]
    sums(lib, kind, 9, begin, end, 75, True)
    sums(lib, kind, 9, begin, end, 75, False)
