"""The Groth16 key check's step functions (libzkp_amd/csrc/g16_keycheck.h) and its view of a key blob (g16_keyblob.h) on the CPU, against
bigint entries from oracle/py/bn254.py.

Stored forms, as the table builder writes them (g16_kernels.hip: k_g16_build_table):
  packed   a coordinate x is the integer x * 2^261 mod p plus a multiple of p, below 2.4 p, as eight 32-bit words
  plain    the integer x * 2^260 mod p plus a multiple of p, below 2 p, as ten 26-bit limbs (the last takes what is left)
The predicates compare modulo p: x and x + p are the same coordinate, x + 1 is not."""
import ctypes
import os
import random

import numpy as np
import pytest

from oracle.py import bn254 as bn
import devtier_g16_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = bn.P, bn.R
KINDS = {0: "equality_mimc_pk.bin", 1: "membership_mimc_pk.bin"}
# the finite G2 points of the golden keys: the finite b_g2_query points and beta, gamma, delta
G2_FINITE = {0: (224, 221), 1: (416, 413)}
B2_INF = {0: (113, 334), 1: (240, 653)}          # b_g2_query points at infinity, of how many


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_g16_keycheck.so"))
    L.emul_kc_points.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p]
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ stored forms from bigints
def coords(g2, pt):
    return (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) if g2 else tuple(pt)


def stored(g2, fmt9, pt, add_p=(), bump=None):
    """the entry words of an affine point; add_p: coordinates stored as value + p; bump = (coordinate, d): that coordinate's stored integer + d"""
    out = []
    for c, x in enumerate(coords(g2, pt)):
        v = x * (1 << (261 if fmt9 else 260)) % P
        if c in add_p:
            v += P                                      # v < p, so v + p < 2 p: below 2.4 p (packed) and below 2 p (plain)
        if bump and bump[0] == c:
            v += bump[1]
        if fmt9:
            assert v < 1 << 256
            out += [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]
        else:
            out += [(v >> (26 * k)) & 0x3FFFFFF for k in range(9)] + [v >> 234]
    return np.array(out, dtype=np.uint32)


def follows(lib, g2, fmt9, prev, first, ent):
    return lib.emul_kc_entry_follows(int(g2), int(fmt9), ptr(prev), ptr(first), ptr(ent))


FORMS = [(False, True), (False, False), (True, True), (True, False)]
IDS = ["g1-packed", "g1-plain", "g2-packed", "g2-plain"]


def window_points(g2, bit, upto):
    c, _ = G.curve(g2)
    q = c.mul_pt(G.base_point(g2, 1), 1 << bit)
    pts, e = [], q
    for _ in range(upto):
        pts.append(e)
        e = c.add_pts(e, q)
    return pts


@pytest.mark.parametrize("g2,fmt9", FORMS, ids=IDS)
def test_entry_words(lib, g2, fmt9):
    assert lib.emul_kc_entry_words(int(g2), int(fmt9)) == (4 if g2 else 2) * (8 if fmt9 else 10)


@pytest.mark.parametrize("g2,fmt9", FORMS, ids=IDS)
def test_rule_b_on_correct_and_wrong_triples(lib, g2, fmt9):
    c, _ = G.curve(g2)
    pts = window_points(g2, 28, 6)          # entries 0 .. 5 of a window that starts at bit 28
    S = lambda pt, **kw: stored(g2, fmt9, pt, **kw)      # noqa: E731
    first = S(pts[0])
    for e in range(1, 6):                   # e = 1 is the doubling entry[0] + entry[0]
        assert follows(lib, g2, fmt9, S(pts[e - 1]), first, S(pts[e])) == 1, "entry %d" % e
    # the entry after the next, the previous one, the negative (on the curve, in the group, and still wrong)
    assert follows(lib, g2, fmt9, S(pts[2]), first, S(pts[4])) == 0
    assert follows(lib, g2, fmt9, S(pts[2]), first, S(pts[2])) == 0
    assert follows(lib, g2, fmt9, S(pts[2]), first, S(c.neg_pt(pts[3]))) == 0
    assert follows(lib, g2, fmt9, S(pts[0]), first, S(c.neg_pt(pts[1]))) == 0          # the doubling's negative
    # prev == -first: the sum is the point at infinity, which no entry is
    assert follows(lib, g2, fmt9, S(c.neg_pt(pts[0])), first, S(pts[1])) == 0
    nc = 4 if g2 else 2
    for k in range(nc):
        assert follows(lib, g2, fmt9, S(pts[2]), first, S(pts[3], bump=(k, 1))) == 0, "coordinate %d + 1 passes" % k
        assert follows(lib, g2, fmt9, S(pts[2], bump=(k, 1)), first, S(pts[3])) == 0
        assert follows(lib, g2, fmt9, S(pts[2]), S(pts[0], bump=(k, 1)), S(pts[3])) == 0


@pytest.mark.parametrize("g2,fmt9", FORMS, ids=IDS)
def test_a_coordinate_and_the_same_plus_p_pass_both_ways(lib, g2, fmt9):
    """a stored value v < p and v + p (< 2 p: inside both stored forms' bounds) are the same coordinate, in the entry and in its operands"""
    pts = window_points(g2, 13, 4)
    S = lambda pt, **kw: stored(g2, fmt9, pt, **kw)      # noqa: E731
    for e in (1, 2, 3):                     # e = 1: the doubling is recognised although prev and first differ by p as integers
        for k in range(4 if g2 else 2):
            assert follows(lib, g2, fmt9, S(pts[e - 1]), S(pts[0]), S(pts[e])) == 1
            assert follows(lib, g2, fmt9, S(pts[e - 1]), S(pts[0]), S(pts[e], add_p=(k,))) == 1, (e, k)
            assert follows(lib, g2, fmt9, S(pts[e - 1], add_p=(k,)), S(pts[0]), S(pts[e])) == 1, (e, k)
            assert follows(lib, g2, fmt9, S(pts[e - 1]), S(pts[0], add_p=(k,)), S(pts[e])) == 1, (e, k)
            assert follows(lib, g2, fmt9, S(pts[e - 1]), S(pts[0]), S(pts[e], add_p=(k,), bump=(k, 1))) == 0, (e, k)


@pytest.mark.parametrize("g2,fmt9", FORMS, ids=IDS)
def test_rule_a_anchor(lib, g2, fmt9):
    c, _ = G.curve(g2)
    p = G.base_point(g2, 2)
    base = stored(g2, False, p)
    assert lib.emul_kc_same_point(int(g2), int(fmt9), ptr(base), ptr(stored(g2, fmt9, p))) == 1
    assert lib.emul_kc_same_point(int(g2), int(fmt9), ptr(base), ptr(stored(g2, fmt9, c.neg_pt(p)))) == 0
    assert lib.emul_kc_same_point(int(g2), int(fmt9), ptr(base), ptr(stored(g2, fmt9, c.double(p)))) == 0
    assert lib.emul_kc_same_point(int(g2), int(fmt9), ptr(base), ptr(stored(g2, fmt9, p, bump=(1, 1)))) == 0


def geometry(lib, wbits, uneven):
    out, win = np.zeros(2, dtype=np.uint32), np.zeros(3 * 40, dtype=np.uint32)
    assert lib.emul_kc_geom(wbits, int(uneven), ptr(out), ptr(win)) == 0
    nwin = int(out[0])
    return nwin, int(out[1]), win[:3 * nwin].reshape(nwin, 3).tolist()


@pytest.mark.parametrize("wbits,uneven", [(w, False) for w in range(8, 16)] + [(14, True)])
def test_the_walk_covers_the_reference_geometry(lib, wbits, uneven):
    """g16_win_off / _ent / _bit and the lane mapping against tests/devtier_g16_cases.py's geometry, which is derived from DESIGN.md"""
    g = G.geom(wbits, uneven)
    nwin, slot_ent, win = geometry(lib, wbits, uneven)
    assert (nwin, slot_ent) == (g.nwin, g.slot_ent)
    assert win == [[g.off[w], g.ent[w], g.bit[w]] for w in range(g.nwin)]
    assert all(e % 64 == 0 for e in g.ent)          # a wave of 64 adjacent lanes stays inside one window
    out = np.zeros(2, dtype=np.uint32)
    for w in range(g.nwin):
        for e in (0, 1, g.ent[w] - 1):
            lib.emul_kc_window_of(wbits, int(uneven), g.off[w] + e, ptr(out))
            assert out.tolist() == [w, e]


@pytest.mark.parametrize("g2,fmt9", FORMS, ids=IDS)
def test_window_joins_of_the_uneven_form(lib, g2, fmt9):
    """2 * (last entry of window w) == entry 0 of window w + 1 for 15 -> 16 and 16 -> 17 of the uneven 2^14 form; window 17 built from bit
    238 (one bit early: where the 15-bit window 16 ends if it is taken for a 14-bit one) fails"""
    c, _ = G.curve(g2)
    _, _, win = geometry(lib, 14, True)
    p = G.base_point(g2, 1)
    joins = lambda a, b: lib.emul_kc_window_joins(int(g2), int(fmt9), ptr(stored(g2, fmt9, a)), ptr(stored(g2, fmt9, b)))      # noqa: E731
    for w in (15, 16):
        ent, bit = win[w][1], win[w][2]
        last = c.mul_pt(p, ent << bit)                     # entry ent - 1 is ent * 2^bit * P
        nxt = c.mul_pt(p, 1 << win[w + 1][2])
        assert joins(last, nxt) == 1, "windows %d -> %d" % (w, w + 1)
        assert joins(last, c.neg_pt(nxt)) == 0
        assert joins(last, last) == 0
    assert win[17][2] == 239
    last16 = c.mul_pt(p, win[16][1] << win[16][2])
    assert joins(last16, c.mul_pt(p, 1 << 238)) == 0       # window 17 started one bit early
    assert joins(last16, c.mul_pt(p, 1 << 240)) == 0


def test_the_whole_lane_on_a_small_host_table(lib):
    """kc_table_entry_ok over a two-slot packed G1 table at radix 2^8 built from bigints: every entry passes; a change to entry 0 of window
    1 fails the join there and every later entry of that window, and nothing else"""
    g = G.geom(8)
    tab = np.zeros((2, g.slot_ent, 16), dtype=np.uint32)
    sub = 3                                               # windows built per slot (the table is addressed by offsets, the rest stays zero)
    for s in range(2):
        for w in range(sub):
            for e, pt in enumerate(window_points_of(s, g.bit[w], g.ent[w])):
                tab[s, g.off[w] + e] = stored(False, True, pt)
    bases = np.array([stored(False, False, G.base_point(False, s)) for s in range(2)], dtype=np.uint32)
    ok = lambda s, w, e: lib.emul_kc_table_entry_ok(0, 1, 8, 0, ptr(tab), ptr(bases), 2, s, w, e)      # noqa: E731
    for s in range(2):
        for w in range(sub):
            for e in (0, 1, 2, 63, 64, g.ent[w] - 1):
                assert ok(s, w, e) == 1, (s, w, e)
    tab[1, g.off[1]] = stored(False, True, G.BN.G1C.double(G.base_point(False, 1)))
    assert ok(1, 1, 0) == 0 and all(ok(1, 1, e) == 0 for e in (1, 2, g.ent[1] - 1))
    assert ok(1, 0, g.ent[0] - 1) == 1 and ok(1, 2, 0) == 1 and ok(0, 1, 0) == 1


def window_points_of(slot, bit, n):
    c = G.BN.G1C
    q = c.mul_pt(G.base_point(False, slot), 1 << bit)
    e, out = q, []
    for _ in range(n):
        out.append(e)
        e = c.add_pts(e, q)
    return out


# ------------------------------------------------------------------------------------------------ the blob side (POINTS without a device)
def pk_blob(kind):
    with open(os.path.join(ROOT, "tests", "golden", KINDS[kind]), "rb") as f:
        return f.read()


def points(lib, kind, blob):
    out = np.zeros(8, dtype=np.uint32)
    rc = lib.emul_kc_points(kind, blob, len(blob), ptr(out))
    return rc, dict(zip(("format", "g2_checked", "g2_outside", "first", "twins", "inf_mismatches", "b1_inf", "b2_inf"), (int(x) for x in out)))


def b_g2_offset(blob, j):
    """byte offset of b_g2_query[j] in an ark-serialize uncompressed ProvingKey<Bn254>"""
    n_ic = int.from_bytes(blob[448:456], "little")
    at = 456 + 64 * n_ic + 128                              # vk | beta_g1, delta_g1
    na = int.from_bytes(blob[at:at + 8], "little"); at += 8 + 64 * na
    nb1 = int.from_bytes(blob[at:at + 8], "little"); at += 8 + 64 * nb1
    nb2 = int.from_bytes(blob[at:at + 8], "little")
    assert j < nb2
    return at + 8 + 128 * j


def b_g1_offset(blob, j):
    n_ic = int.from_bytes(blob[448:456], "little")
    at = 456 + 64 * n_ic + 128
    na = int.from_bytes(blob[at:at + 8], "little"); at += 8 + 64 * na
    assert j < int.from_bytes(blob[at:at + 8], "little")
    return at + 8 + 64 * j


def cofactor_point():
    """a point of the twist's cofactor part, as tests/test_gpu_verify.py builds one: a random twist point times R"""
    from test_gpu_verify import _f2_sqrt
    rr = random.Random(9)
    while True:
        x = (rr.randrange(P), rr.randrange(P))
        y = _f2_sqrt(bn, bn.f2_add(bn.f2_mul(bn.f2_sq(x), x), bn.B2))
        if y is not None:
            break
    cof = bn.G2C.mul_pt((x, y), R, reduce=False)
    assert cof is not None and bn.G2C.is_on_curve(cof)
    return cof


def moved_g2(blob, off):
    okb, pt = bn.de_g2(blob[off:off + 128])
    assert okb and pt is not None
    out = bytearray(blob)
    out[off:off + 128] = bn.ser_g2(bn.G2C.add_pts(pt, cofactor_point()))
    return bytes(out)


def finite_b_g2(blob, start=0):
    j = start
    while blob[b_g2_offset(blob, j) + 127] & 0x40:
        j += 1
    return j


@pytest.mark.parametrize("kind", KINDS)
def test_golden_keys_are_sound(lib, kind):
    blob = pk_blob(kind)
    rc, r = points(lib, kind, blob)
    total, query = G2_FINITE[kind]
    inf, of = B2_INF[kind]
    assert rc == 0 and r["format"] == 0
    assert (r["g2_checked"], r["g2_outside"], r["first"]) == (total, 0, 0xFFFFFFFF) and total == query + 3 and query == of - inf
    assert (r["b1_inf"], r["b2_inf"], r["inf_mismatches"], r["twins"]) == (inf, inf, 0, query)
    # its verifying key alone: the three points of the head
    n_ic = int.from_bytes(blob[448:456], "little")
    rc, r = points(lib, kind, blob[:456 + 64 * n_ic])
    assert rc == 0 and (r["format"], r["g2_checked"], r["g2_outside"], r["twins"]) == (1, 3, 0, 0)


def test_a_b_g2_query_point_outside_the_subgroup_is_reported_by_its_file_index(lib):
    blob = pk_blob(0)
    j = finite_b_g2(blob, 17)
    assert j > 17 or not blob[b_g2_offset(blob, 17) + 127] & 0x40          # (points at infinity before j are skipped, the index still counts them)
    rc, r = points(lib, 0, moved_g2(blob, b_g2_offset(blob, j)))
    assert rc == 0 and (r["g2_checked"], r["g2_outside"], r["first"]) == (224, 1, 3 + j)
    name = ctypes.create_string_buffer(48)
    lib.emul_kc_point_name(3 + j, name, 48)
    assert name.value.decode() == "b_g2_query[%d]" % j


def test_gamma_g2_outside_the_subgroup_is_index_1(lib):
    blob = pk_blob(0)
    rc, r = points(lib, 0, moved_g2(blob, 64 + 128))
    assert rc == 0 and (r["g2_outside"], r["first"]) == (1, 1)
    name = ctypes.create_string_buffer(48)
    lib.emul_kc_point_name(1, name, 48)
    assert name.value.decode() == "gamma_g2"
    n_ic = int.from_bytes(blob[448:456], "little")
    rc, r = points(lib, 0, moved_g2(blob, 64 + 128)[:456 + 64 * n_ic])      # the same in a verifying key alone
    assert rc == 0 and (r["format"], r["g2_checked"], r["g2_outside"], r["first"]) == (1, 3, 1, 1)


def test_an_infinity_flag_on_one_twin_only_is_counted(lib):
    blob = bytearray(pk_blob(0))
    j = finite_b_g2(blob)
    off = b_g1_offset(blob, j)
    blob[off:off + 64] = bytes(63) + b"\x40"
    rc, r = points(lib, 0, bytes(blob))
    assert rc == 0 and (r["inf_mismatches"], r["twins"], r["g2_outside"]) == (1, 220, 0)
