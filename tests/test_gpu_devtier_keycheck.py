"""The Groth16 key check's kernels on the device (tests/devtier/devtier_keycheck.hip): k_g16_check_table through the product's
g16_launch_check_table over tables the product's g16_launch_build_table made, k_g16_subgroup, and the twin sums.  No zkp_hip_init, no keys.

Tables (base points as in tests/devtier_g16_cases.py), G1 and G2 each, at the smallest shapes at which the check can go wrong:
  packed 2^8         a window (128 entries) shorter than the builder's 512-entry segment, and than the check's 256-lane workgroup
  packed 2^11        two builder segments per window; entry 512 is the seam
  packed 2^14 uneven windows 16 (twice the entries) and 17 (from bit 239, 25 088 entries); two slots
  plain 2^10         the verifier's gamma_abc_g1 form, G1 only
The clean table reports nothing.  After ONE change the reported set of (slot, window) pairs is exactly the expected one and the first bad
location is the expected one; a broken join of two windows is reported at entry 0 of the upper window.  A packed or plain coordinate
replaced by the same value plus p is the same coordinate and is not reported.  The kernel writes nothing but its documented output words."""
import ctypes
import os

import numpy as np
import pytest

import devtier_g16_cases as GC
from oracle.py import bn254 as bn

pytestmark = pytest.mark.gpu
P = bn.P
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    L = ctypes.CDLL(ge.build_devtier_keycheck())
    L.devtier_kc_entry_words.restype = ctypes.c_uint32
    return L


ptr = GC.ptr
# (g2, packed, wbits, uneven, slots)
TABLES = [(g2, 1, w, u, n) for g2 in (0, 1) for w, u, n in ((8, 0, 3), (11, 0, 3), (14, 1, 2))] + [(0, 0, 10, 0, 3)]
IDS = ["%s-%s-w%d%s" % ("G2" if t[0] else "G1", "packed" if t[1] else "plain", t[2], "u" if t[3] else "") for t in TABLES]
_BUILT = {}


def bases_of(g2, nslots):
    return np.array([GC.pt_words(g2, GC.base_point(g2, s)) for s in range(nslots)], dtype=np.uint32)


def built(lib, t):
    """the table of one form, built once by the product's builder and never changed: [slots][slot_ent][entry words]"""
    if t not in _BUILT:
        g2, packed, wbits, uneven, nslots = t
        g = GC.geom(wbits, bool(uneven))
        ow = lib.devtier_kc_entry_words(g2, packed)
        assert ow == (4 if g2 else 2) * (8 if packed else 10)
        geo = np.zeros(3, dtype=np.uint32)
        assert lib.devtier_kc_geom(wbits, uneven, ptr(geo)) == 0 and geo.tolist() == [g.nwin, g.ent[0], g.slot_ent]
        raw = np.zeros((nslots, g.slot_ent, ow), dtype=np.uint32)
        rc = lib.devtier_kc_build(g2, packed, wbits, uneven, ptr(bases_of(g2, nslots)), nslots, ptr(raw))
        assert rc == 0, "devtier_kc_build returned %d" % rc
        raw.setflags(write=False)
        _BUILT[t] = raw
    return _BUILT[t]


def check(lib, t, raw):
    g2, packed, wbits, uneven, nslots = t
    g = GC.geom(wbits, bool(uneven))
    pairs, out, written = np.zeros((nslots, g.nwin), dtype=np.uint32), np.zeros(4, dtype=np.uint32), np.full(3, 99, dtype=np.uint32)
    raw = np.ascontiguousarray(raw)
    rc = lib.devtier_kc_check(g2, packed, wbits, uneven, ptr(bases_of(g2, nslots)), nslots, ptr(raw), ptr(pairs), ptr(out), ptr(written))
    assert rc == 0, "devtier_kc_check returned %d" % rc
    assert written.tolist() == [0, 0, 0], "words written outside the kernel's outputs: table and the guard behind it %d, around pair_bad %d, around the output words %d" % tuple(written)
    bad = {(s, w) for s, w in np.argwhere(pairs != 0).tolist()}
    key = int(out[3]) << 32 | int(out[2])
    first = None if key == (1 << 64) - 1 else (key >> 40, (key >> 32) & 0xFF, key & 0xFFFFFFFF)
    assert int(out[0]) == len(bad) and int(out[1]) == int(pairs.sum()), "the counts do not add up: %r against %r" % (out.tolist(), pairs.tolist())
    assert (first is None) == (not bad)
    return bad, first, pairs


# ---- the stored integer of a coordinate and back (packed: eight 32-bit words; plain: ten 26-bit limbs)
def coord_get(entry, k, packed):
    if packed:
        return sum(int(w) << (32 * i) for i, w in enumerate(entry[8 * k:8 * k + 8]))
    return sum(int(w) << (26 * i) for i, w in enumerate(entry[10 * k:10 * k + 10]))


def coord_put(entry, k, packed, v):
    if packed:
        assert 0 <= v < 1 << 256
        entry[8 * k:8 * k + 8] = [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    else:
        entry[10 * k:10 * k + 10] = [(v >> (26 * i)) & 0x3FFFFFF for i in range(9)] + [v >> 234]


def expect(lib, t, raw, pairs, first, what):
    bad, got_first, _ = check(lib, t, raw)
    assert bad == set(pairs), "%s: reported pairs %r, expected %r" % (what, sorted(bad), sorted(pairs))
    assert got_first == first, "%s: first bad location %r, expected %r" % (what, got_first, first)


@pytest.mark.parametrize("t", TABLES, ids=IDS)
def test_clean_table_reports_nothing(lib, t):
    bad, first, pairs = check(lib, t, built(lib, t))
    assert not bad and first is None and not pairs.any()


@pytest.mark.parametrize("t", TABLES, ids=IDS)
def test_one_changed_word_is_found_where_it_is(lib, t):
    g2, packed, wbits, uneven, nslots = t
    g = GC.geom(wbits, bool(uneven))
    base = built(lib, t)
    s, top = nslots - 1, g.nwin - 1
    wm = g.nwin // 2

    def flipped(slot, w, e, word=0):
        raw = base.copy()
        raw[slot, g.off[w] + e, word] ^= 1
        return raw

    ow = base.shape[2]
    # the anchor: entry 0 of window 0 is no longer P, and nothing of window 0 follows from it
    expect(lib, t, flipped(s, 0, 0), {(s, 0)}, (s, 0, 0), "anchor")
    # entry 0 of a middle window: the join from the window below (reported here, at entry 0) and every entry of the window
    expect(lib, t, flipped(0, wm, 0, ow - 1), {(0, wm)}, (0, wm, 0), "entry 0 of a middle window")
    _, _, pairs = check(lib, t, flipped(0, wm, 0))
    assert int(pairs[0, wm]) == g.ent[wm], "every entry of a window depends on its entry 0"
    # the last entry of a window: that entry, and the join into the next window
    last = g.ent[wm] - 1
    expect(lib, t, flipped(0, wm, last), {(0, wm), (0, wm + 1)}, (0, wm, last), "last entry of a window")
    _, _, pairs = check(lib, t, flipped(0, wm, last))
    assert (int(pairs[0, wm]), int(pairs[0, wm + 1])) == (1, 1)
    # the very last entry of the top window has no window above it
    expect(lib, t, flipped(s, top, g.ent[top] - 1, ow // 2), {(s, top)}, (s, top, g.ent[top] - 1), "last entry of the top window")
    # an entry in the middle: it does not follow from its neighbour, and its right neighbour does not follow from it
    e = g.ent[1] // 2 + 1
    expect(lib, t, flipped(1, 1, e), {(1, 1)}, (1, 1, e), "a middle entry")
    _, _, pairs = check(lib, t, flipped(1, 1, e))
    assert int(pairs[1, 1]) == 2
    if g.ent[0] > 512:                                     # the seam of the builder's two segments
        expect(lib, t, flipped(1, 2, 512), {(1, 2)}, (1, 2, 512), "entry 512")
        expect(lib, t, flipped(1, 2, 511), {(1, 2)}, (1, 2, 511), "entry 511")
    if uneven:
        # windows 16 (twice the entries) and 17 (from bit 239)
        expect(lib, t, flipped(1, 16, g.ent[16] - 1), {(1, 16), (1, 17)}, (1, 16, g.ent[16] - 1), "last entry of window 16")
        expect(lib, t, flipped(0, 16, 0), {(0, 16)}, (0, 16, 0), "entry 0 of window 16")
        expect(lib, t, flipped(0, 17, 0), {(0, 17)}, (0, 17, 0), "entry 0 of window 17")
        expect(lib, t, flipped(0, 16, g.ent[0]), {(0, 16)}, (0, 16, g.ent[0]), "the first entry of window 16's second half")


@pytest.mark.parametrize("t", TABLES, ids=IDS)
def test_negated_swapped_and_plus_p(lib, t):
    g2, packed, wbits, uneven, nslots = t
    g = GC.geom(wbits, bool(uneven))
    base = built(lib, t)
    nc = 4 if g2 else 2
    w, e = 2, g.ent[2] // 2 - 3
    # an entry replaced by its negative: on the curve, in the group, and wrong
    raw = base.copy()
    ent = raw[1, g.off[w] + e]
    for k in range(nc // 2, nc):
        coord_put(ent, k, packed, -coord_get(ent, k, packed) % P)
    expect(lib, t, raw, {(1, w)}, (1, w, e), "a negated entry")
    # two adjacent entries swapped
    raw = base.copy()
    raw[0, [g.off[w] + e, g.off[w] + e + 1]] = raw[0, [g.off[w] + e + 1, g.off[w] + e]]
    expect(lib, t, raw, {(0, w)}, (0, w, e), "two swapped entries")
    _, _, pairs = check(lib, t, raw)
    assert int(pairs[0, w]) == 3                           # e, e + 1, and e + 2, which no longer follows from its left neighbour
    # the same value plus p stays inside the stored form's bound (2.4 p packed, 2 p plain) and is the same coordinate: NOT reported
    bound = 24 * P // 10 if packed else 2 * P
    raw, moved = base.copy(), 0
    for slot, ww, ee in ((0, 0, 0), (0, 0, 1), (1, w, e), (nslots - 1, g.nwin - 1, g.ent[g.nwin - 1] - 1), (1, w, g.ent[w] - 1), (1, w + 1, 0)):
        ent = raw[slot, g.off[ww] + ee]
        for k in range(nc):
            v = coord_get(ent, k, packed)
            if v + P < bound:
                coord_put(ent, k, packed, v + P)
                moved += 1
    assert moved >= 6 and (raw != base).any()
    expect(lib, t, raw, set(), None, "coordinates plus p")
    # ... and one more than that is reported
    ent = raw[1, g.off[w] + e]
    coord_put(ent, 0, packed, coord_get(ent, 0, packed) + 1)
    expect(lib, t, raw, {(1, w)}, (1, w, e), "a coordinate plus p plus 1")


def test_subgroup_lanes(lib):
    """one lane per G2 point: multiples of the generator are inside; the same points moved by a point of the twist's cofactor part are not"""
    from test_emul_g16_keycheck import cofactor_point
    cof = cofactor_point()
    inside = [GC.base_point(1, s) for s in range(3)] + [bn.G2C.mul_pt(bn.G2, k) for k in (2, 3, bn.R - 1)]
    pts = inside + [bn.G2C.add_pts(p, cof) for p in inside] + [cof] + [inside[0]] * 60          # 73 lanes: more than one wave
    words = np.array([GC.pt_words(1, p) for p in pts], dtype=np.uint32)
    ok = np.full(len(pts) + 8, 0x5A, dtype=np.uint8)
    assert lib.devtier_kc_subgroup(ptr(words), len(pts), ptr(ok)) == 0
    assert ok[:len(pts)].tolist() == [1] * 6 + [0] * 7 + [1] * 60 and (ok[len(pts):] == 0x5A).all()


@pytest.mark.parametrize("g2", [0, 1], ids=["G1", "G2"])
def test_twin_sums(lib, g2):
    """sum rho_i P_i over 70 points (more than a wave, more than the sum tree's 32 slices) with 128-bit weights, against bigints"""
    import random
    rnd = random.Random(99 + g2)
    c, gen = GC.curve(g2)
    ks = [rnd.randrange(1, bn.R) for _ in range(70)]
    pts = [c.mul_pt(gen, k) for k in ks]
    rho = [rnd.randrange(1 << 128) for _ in range(70)]
    rho[0], rho[1], rho[2] = (1 << 128) - 1, 1, 1 << 127          # every digit at its largest, the smallest weight, the top bit alone
    want = c.mul_pt(gen, sum(r * k for r, k in zip(rho, ks)))
    words = np.array([GC.pt_words(g2, p) for p in pts], dtype=np.uint32)
    rw = np.array([[(r >> (32 * i)) & 0xFFFFFFFF for i in range(4)] for r in rho], dtype=np.uint32)
    out = np.zeros(33 if g2 else 17, dtype=np.uint32)
    assert lib.devtier_kc_twin_sum(g2, ptr(words), ptr(rw), 70, ptr(out)) == 0
    assert out.tolist() == GC.pt_words(g2, want).tolist() + [0]
    # weights that cancel: the sum is the point at infinity
    words2 = np.array([GC.pt_words(g2, pts[0]), GC.pt_words(g2, c.neg_pt(pts[0]))], dtype=np.uint32)
    rw2 = np.array([rw[3], rw[3]], dtype=np.uint32)
    assert lib.devtier_kc_twin_sum(g2, ptr(words2), ptr(rw2), 2, ptr(out)) == 0
    assert int(out[-1]) == 1
