"""Cases and bigint references of the device tier's Groth16 entry points (tests/devtier/devtier_g16.h): the key tables k_g16_build_table
writes, the digit recodings that index them, and the launch in which builder, recoder and planner meet.  Shared by the host tests
(tests/test_devtier_g16.py) and the device tests (tests/test_gpu_devtier_g16.py).

Everything here is derived from DESIGN.md 6b, not from g16_radix: a key point's block is, window by window, the multiples
(i + 1) * 2^bit(w) * P; an even radix 2^w has ceil(255 / w) windows of w bits (254 scalar bits and the recoding's carry) with 2^(w-1)
entries each; the uneven form of 2^14 is sixteen 14-bit windows, one 15-bit window with 16 384 entries, and the top 15 bits from bit 239
as an unsigned digit with as many 512-entry segments as the largest digit of a scalar below r needs."""
import ctypes
import functools
import random

import numpy as np

import devtier_cases as DC
from oracle.py import bn254 as BN
from oracle.py import ristretto as RIS

R, L = BN.R, RIS.L
SEG = 512                                                   # the builder's segment: one thread walks at most this many entries
DIGW_MAX = 16
FILL = 0xA5A5A5A5


# ------------------------------------------------------------------------------------------------ geometry
class Geom:
    """windows of one radix form: first bit, width, entry count and first entry of each"""

    def __init__(self, wbits, uneven=False, modulus=R):
        self.wbits, self.uneven, self.q = wbits, uneven, modulus
        bits = (modulus - 1).bit_length()
        if uneven:
            assert wbits == 14 and modulus == R
            self.width = [14] * 16 + [15, 15]
            top = ((modulus - 1) >> 239) + 1                # the largest top digit: the top bits of r - 1 and a carry from below
            self.ent = [1 << 13] * 16 + [1 << 14, -(-top // SEG) * SEG]
        else:
            nwin = -(-(bits + 1) // wbits)                  # the scalar's bits and the carry of the signed recoding
            self.width, self.ent = [wbits] * nwin, [1 << (wbits - 1)] * nwin
        self.nwin = len(self.width)
        self.bit = [sum(self.width[:w]) for w in range(self.nwin)]
        self.off = [sum(self.ent[:w]) for w in range(self.nwin)]
        self.slot_ent = sum(self.ent)
        self.digw = (self.nwin + 1) // 2
        self.nwin_u64 = -(-65 // wbits)                     # 64 bits and the carry
        self.seg = min(SEG, self.ent[0])

    @property
    def id(self):
        return "w%d%s" % (self.wbits, "u" if self.uneven else "")


@functools.lru_cache(maxsize=None)
def geom(wbits, uneven=False):
    return Geom(wbits, uneven)


def recode(x, g):
    """signed digits of x at the form's windows: a digit above half the radix borrows from the window above; the top
    window of the uneven form keeps its digit unsigned.  Returns the digits and the carry that leaves the top window."""
    out, carry = [], 0
    for j in range(g.nwin):
        d = ((x >> g.bit[j]) & ((1 << g.width[j]) - 1)) + carry
        carry = 1 if d > (1 << (g.width[j] - 1)) and not (g.uneven and j == g.nwin - 1) else 0
        out.append(d - (carry << g.width[j]))
    return out, carry


class Form:
    """one recoding the harness runs: its id in G16DigCase, its windows, the modulus its scalars stay below"""

    def __init__(self, opid, name, g):
        self.opid, self.name, self.g = opid, name, g

    @property
    def id(self):
        return self.name


FORMS = [Form(w - 8, "g16_recode_w%d" % w, geom(w)) for w in range(8, 16)] + [Form(8, "g16_recode_w14_uneven", geom(14, True))]
FORMS += [Form(9 + w - 11, "sc_recode_signed_rt_w%d" % w, Geom(w, False, L)) for w in range(11, 16)]
N_RANDOM = 2000


def pinned(g):
    """the fixed scalars of one form, all below its modulus"""
    q = g.q
    out = [0, 1, 2, q - 1, q - 2, (q + 1) // 2, (q - 1) // 2]
    for k in sorted(set(g.bit[1:]) | {32 * i for i in range(1, 8)} | {g.bit[-1] + g.width[-1]}):      # window and word boundaries: every straddle position
        out += [(1 << k) - 1, 1 << k]
    for j in range(g.nwin):
        half = 1 << (g.width[j] - 1)
        out += [half << g.bit[j], (half + 1) << g.bit[j]]   # exactly half the radix stays positive with no carry; one more carries
    k = (q - 1).bit_length() - 1
    out += [(1 << k) - 1, (1 << k) - 2, (1 << k) - (1 << g.bit[1])]      # every window at 2^wb - 1 (all ones below the modulus): the carry ripples to the top
    out += [(1 << 64) - 1, 1 << 63, (1 << 63) + 1, (1 << 64) - (1 << g.bit[1])]
    return [x for x in out if 0 <= x < q]


@functools.lru_cache(maxsize=None)
def scalars_of(form_id):
    fm = next(f for f in FORMS if f.id == form_id)
    rnd = random.Random(sum(form_id.encode()))
    out = pinned(fm.g)
    out += [rnd.randrange(fm.g.q) for _ in range(N_RANDOM)]
    out += [rnd.randrange(1 << 64) for _ in range(200)]
    return out


def to_words(xs):
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype=np.uint32).reshape(len(xs), 8).copy()


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def run_digits(lib, fm, xs, on_device):
    w = to_words(xs)
    out = np.zeros((len(xs), DIGW_MAX), dtype=np.uint32)
    lib.devtier_g16_digits.restype = ctypes.c_int
    rc = lib.devtier_g16_digits(ctypes.c_int(fm.opid), ctypes.c_uint32(len(xs)), ptr(w), ptr(out), ctypes.c_int(on_device))
    assert rc == 0, "devtier_g16_digits(%s) returned %d" % (fm.id, rc)
    return out


def decode(words, nwin):
    """digits as the gather kernel decodes them: (int16_t) of the half of the word the window selects"""
    d = [(int(words[j >> 1]) >> (16 * (j & 1))) & 0xFFFF for j in range(nwin)]
    return [x - 65536 if x >= 32768 else x for x in d]


def check_reference_caps(fm, xs):
    """what the callers rely on, about the reference alone: no carry leaves the top window, every digit is inside its window's entries"""
    g, top = fm.g, 0
    for x in xs:
        d, carry = recode(x, g)
        assert carry == 0, (fm.id, "the reference carries out of its top window", hex(x))
        assert all(abs(v) <= e for v, e in zip(d, g.ent)), (fm.id, hex(x), d)
        assert sum(v << b for v, b in zip(d, g.bit)) == x
        top = max(top, d[-1])
    return top


def check_digits(fm, xs, out):
    g = fm.g
    for x, o in zip(xs, out):
        tag = (fm.id, hex(x))
        assert all(int(w) == FILL for w in o[g.digw:]), tag + ("words past the form's digit words were written",)
        d = decode(o, g.nwin)
        assert sum(v << b for v, b in zip(d, g.bit)) == x, tag + ("digits do not sum to the scalar", d)
        for j, v in enumerate(d):
            signed = not (g.uneven and j == g.nwin - 1)
            lo, hi = (-((1 << (g.width[j] - 1)) - 1), 1 << (g.width[j] - 1)) if signed else (0, g.ent[j])
            assert lo <= v <= hi, tag + ("window %d: digit %d outside [%d, %d]" % (j, v, lo, hi),)
            assert abs(v) <= g.ent[j], tag + ("window %d: digit %d selects an entry past the window's %d" % (j, v, g.ent[j]),)
        if g.nwin & 1:
            assert int(o[g.digw - 1]) >> 16 == 0, tag + ("the unused half of the last digit word is not zero",)
        if x < 1 << 64:
            assert all(v == 0 for v in d[g.nwin_u64:]), tag + ("a 64-bit value reaches past window %d" % g.nwin_u64, d)
        assert d == recode(x, g)[0], tag + ("not the reference's digits", d)


# ------------------------------------------------------------------------------------------------ points and tables
def curve(g2):
    return (BN.G2C, BN.G2) if g2 else (BN.G1C, BN.G1)


def pt_bytes(g2, pt):
    comps = (pt[0][0], pt[0][1], pt[1][0], pt[1][1]) if g2 else pt
    return b"".join(c.to_bytes(32, "little") for c in comps)


def pt_words(g2, pt):
    return np.frombuffer(pt_bytes(g2, pt), dtype=np.uint32).copy()


@functools.lru_cache(maxsize=None)
def base_mult(slot):
    """slot 0 is the generator; the others are seeded full-width multiples of it"""
    return 1 if slot == 0 else random.Random(7700 + slot).randrange(1 << 250, R)


@functools.lru_cache(maxsize=None)
def base_point(g2, slot):
    c, gen = curve(g2)
    return c.mul_pt(gen, base_mult(slot))


@functools.lru_cache(maxsize=8)
def slot_reference(g2, slot, wbits, uneven):
    """every entry of one point's block, [slot_ent][16 | 32] canonical words: window w starts from Q = 2^bit(w) P and entry i + 1 is entry
    i + Q, one affine addition per entry (the first of them is the doubling Q + Q)"""
    g, (c, _) = geom(wbits, uneven), curve(g2)
    q, at, buf = base_point(g2, slot), 0, []
    for w in range(g.nwin):
        for _ in range(g.bit[w] - at):
            q = c.double(q)
        at = g.bit[w]
        e = q
        for _ in range(g.ent[w]):
            buf.append(pt_bytes(g2, e))
            e = c.add_pts(e, q)
    out = np.frombuffer(b"".join(buf), dtype=np.uint32).reshape(g.slot_ent, -1)
    assert out.shape[1] == (32 if g2 else 16)
    return out


def sample_indices(g, seed):
    """entries of a block checked where it is sampled: the first, second, eighth, ninth and last of every builder segment of every window
    (the ladder's landing point, the first batch of eight and the step into the second, the segment's end), and 256 seeded others"""
    rnd = random.Random(seed)
    idx = set()
    for w in range(g.nwin):
        for s0 in range(0, g.ent[w], g.seg):
            idx |= {(w, s0 + o) for o in (0, 1, 7, 8, g.seg - 1)}
    while len(idx) < sum(g.ent[w] // g.seg for w in range(g.nwin)) * 5 + 256:
        w = rnd.randrange(g.nwin)
        idx.add((w, rnd.randrange(g.ent[w])))
    return sorted(idx)


def sample_reference(g2, slot, g, idx):
    """the sampled entries by another route than the chain: per window Q = 2^bit(w) P, per segment k the point (k seg) Q by repeated
    addition of seg Q, and entry k seg + o as that plus (o + 1) Q; the seeded ones as (i + 1) Q by double-and-add"""
    c, _ = curve(g2)
    q, at, want = base_point(g2, slot), 0, {}
    by_win = {}
    for w, i in idx:
        by_win.setdefault(w, []).append(i)
    for w in range(g.nwin):
        for _ in range(g.bit[w] - at):
            q = c.double(q)
        at = g.bit[w]
        small = {o: c.mul_pt(q, o + 1, reduce=False) for o in (0, 1, 7, 8, g.seg - 1)}
        seg_q, base, bases = small[g.seg - 1], None, []
        for _ in range(g.ent[w] // g.seg):
            bases.append(base)
            base = c.add_pts(base, seg_q)
        for i in by_win.get(w, []):
            k, o = divmod(i, g.seg)
            want[(w, i)] = c.add_pts(bases[k], small[o]) if o in small else c.mul_pt(q, i + 1, reduce=False)
    return np.array([pt_words(g2, want[k]) for k in idx], dtype=np.uint32)


def run_table(lib, g2, msm_form, wbits, uneven, nslots, expect_rc=0):
    g = geom(wbits, uneven) if 8 <= wbits <= 15 and (not uneven or wbits == 14) else None
    aw = 32 if g2 else 16
    ow = aw if msm_form else (40 if g2 else 20)
    n = g.slot_ent if g and 1 <= nslots <= 4 else 1
    bases = np.array([pt_words(g2, base_point(g2, s)) for s in range(max(1, min(nslots, 4)))], dtype=np.uint32)
    raw, aff = np.zeros((max(nslots, 1), n, ow), dtype=np.uint32), np.zeros((max(nslots, 1), n, aw), dtype=np.uint32)
    guard = np.full(3, 99, dtype=np.uint32)
    lib.devtier_g16_table.restype = ctypes.c_int
    rc = lib.devtier_g16_table(ctypes.c_int(g2), ctypes.c_int(msm_form), ctypes.c_uint32(wbits), ctypes.c_uint32(uneven), ptr(bases), ctypes.c_uint32(nslots),
                               ptr(raw), ptr(aff), ptr(guard))
    assert rc == expect_rc, "devtier_g16_table returned %d" % rc
    return raw, aff, guard


def words_below(arr, bound):
    """value of the eight little-endian words < bound, for every row of arr[..., 8]"""
    b = [(bound >> (32 * i)) & 0xFFFFFFFF for i in range(8)]
    lt, eq = np.zeros(arr.shape[:-1], dtype=bool), np.ones(arr.shape[:-1], dtype=bool)
    for i in reversed(range(8)):
        lt |= eq & (arr[..., i] < b[i])
        eq &= arr[..., i] == b[i]
    return lt


def packed_bound(g2):
    """exclusive bound of a packed coordinate, from the interval proof: what the builder's conversion yields for G1 (the "< 2.4 p" of the
    kernel's comment), the entry class of g2_mmadd9 for G2"""
    num, den = (DC.FQB.G2_MMADD9_BOUNDS["q"]) if g2 else (DC.FQB.KEY_ENTRY_BOUND.numerator, DC.FQB.KEY_ENTRY_BOUND.denominator)
    return -(-num * DC.PQ // den)


def check_stored_form(g2, msm_form, raw):
    """raw: [..., words of one entry]"""
    nc = 4 if g2 else 2
    if msm_form:
        co = raw.reshape(raw.shape[:-1] + (nc, 8))
        w64 = co.astype(np.uint64)
        for i in range(9):                                  # the nine limbs as fq9_unpack8 takes them out of the eight words
            wd, sh = (29 * i) >> 5, (29 * i) & 31
            x = w64[..., wd] >> np.uint64(sh)
            if sh + 29 > 32 and wd + 1 < 8:
                x = x | (w64[..., wd + 1] << np.uint64(32 - sh))
            if i < 8:
                x = x & np.uint64((1 << 29) - 1)
            assert (x < np.uint64(1 << 29)).all(), "limb %d of a packed coordinate is not below 2^29" % i
        bad = np.argwhere(~words_below(co, packed_bound(g2)))
        assert bad.size == 0, "a packed coordinate leaves the entry class of the MSM loop, first at %r" % (bad[0].tolist(),)
        return
    co = raw.reshape(raw.shape[:-1] + (nc, 10))
    assert (co[..., :9] < (1 << 26)).all(), "a plain coordinate is not carried"
    flat = co.reshape(-1, 10)
    lim = DC.FQB.CANON.val * DC.PQ // 1000                  # the class g16_verify.h reads the entries as: carried, below 2p
    for row in flat:
        assert DC.val(row, DC.FQ_OFF) < lim, "a plain coordinate is not below 2p"


def check_table(g2, msm_form, wbits, uneven, nslots, raw, aff, guard, full_slots):
    """guard, stale entries, stored form, and every entry (full_slots) or the segment-boundary sample (the other slots) against the reference"""
    g = geom(wbits, uneven)
    assert int(guard[0]) == 0, "%d words behind the table were written" % guard[0]
    _check_entries(g2, g, nslots, aff, full_slots)           # first: a wrong entry is named by slot, window, segment and place in its batch
    assert int(guard[1]) == 0, "%d entries were never written" % guard[1]
    if msm_form:
        assert int(guard[2]) == 1, "BnG1::entry / BnG2::entry is not the builder's packed form of entry 1 of window 0"
    check_stored_form(g2, msm_form, raw)


def _check_entries(g2, g, nslots, aff, full_slots):
    wbits, uneven = g.wbits, g.uneven
    for s in range(nslots):
        if s in full_slots:
            ref = slot_reference(g2, s, wbits, uneven)
            bad = np.nonzero((aff[s] != ref).any(axis=1))[0]
            where = None
            if bad.size:
                w = max(j for j in range(g.nwin) if g.off[j] <= bad[0])
                where = "slot %d window %d entry %d (segment %d, position %d of its batch of eight)" % (s, w, bad[0] - g.off[w], (bad[0] - g.off[w]) // g.seg, (bad[0] - g.off[w]) % 8)
            assert bad.size == 0, "%d entries of slot %d differ from (i + 1) 2^bit(w) P, first: %s" % (bad.size, s, where)
        else:
            idx = sample_indices(g, 100 * wbits + s)
            ref = sample_reference(g2, s, g, idx)
            got = aff[s][[g.off[w] + i for w, i in idx]]
            bad = np.nonzero((got != ref).any(axis=1))[0]
            assert bad.size == 0, "%d sampled entries of slot %d differ, first: window %d entry %d" % (bad.size, s, idx[bad[0]][0] if bad.size else -1, idx[bad[0]][1] if bad.size else -1)


# ------------------------------------------------------------------------------------------------ builder, recoder and planner in one launch
ROWS = 70
ACC_K = random.Random(2024).randrange(1 << 200, R)          # acc_init = ACC_K * G; the lists below are asserted clear of every exceptional case


def plan(lib, g, chunks, expect_rc=None):
    steps, step0 = np.zeros((2 * g.nwin, 2), dtype=np.uint32), np.zeros(chunks + 1, dtype=np.uint32)
    lib.devtier_g16_plan.restype = ctypes.c_int
    rc = lib.devtier_g16_plan(ctypes.c_uint32(g.wbits), ctypes.c_uint32(g.uneven), ctypes.c_uint32(chunks), ptr(steps), ptr(step0))
    assert rc == (chunks if expect_rc is None else expect_rc), "devtier_g16_plan returned %d" % rc
    return steps, step0


def walk_of(g, steps, step0):
    """the planner's steps read against the geometry: (slot, window) per step; every (slot, window) once, in chunks that tile the list"""
    out = []
    for first, ds in steps.tolist():
        slot, off = divmod(first, g.slot_ent)
        assert slot < 2 and off in g.off, "step starts at entry %d, which begins no window" % first
        w = g.off.index(off)
        assert ds == ((slot * g.digw + w // 2) << 1 | (w & 1)), "step of slot %d window %d reads digit word %d half %d" % (slot, w, ds >> 1, ds & 1)
        out.append((slot, w))
    assert sorted(out) == [(s, w) for s in range(2) for w in range(g.nwin)]
    assert step0[0] == 0 and step0[-1] == len(out) and all(a < b for a, b in zip(step0, step0[1:]))
    return out


def row_pairs(fm):
    """scalar pairs (s_0, s_1) of the rows: every pinned scalar of the form in either column, filled with seeded ones to whole launches"""
    p = pinned(fm.g)
    rnd = random.Random(31 + fm.opid)
    pairs = [(p[i], p[len(p) - 1 - i]) for i in range(len(p))]
    while len(pairs) % ROWS:
        pairs.append((rnd.randrange(R), rnd.randrange(R)))
    return pairs


def assert_no_exceptional_case(g, walk, step0, pairs, mults):
    """integer arithmetic mod r over every lane and chunk: no prefix sum is 0 or +- the entry about to be added (the lazy additions' contract)"""
    for s0, s1 in pairs:
        d = (recode(s0, g)[0], recode(s1, g)[0])
        total = ACC_K
        for c in range(len(step0) - 1):
            k = ACC_K
            for slot, w in walk[step0[c]:step0[c + 1]]:
                v = d[slot][w]
                if v:
                    e = abs(v) * (1 << g.bit[w]) * mults[slot] % R
                    assert k % R not in (0, e, R - e), "a prefix sum meets +- the entry or the neutral element"
                    k += e if v > 0 else -e
            assert k % R
            total += k - ACC_K
        assert total % R == (ACC_K + s0 * mults[0] + s1 * mults[1]) % R


_MUL_CACHE = {}


def mul_gen(g2, k):
    k %= R
    if (g2, k) not in _MUL_CACHE:
        c, gen = curve(g2)
        _MUL_CACHE[(g2, k)] = c.mul_pt(gen, k)
    return _MUL_CACHE[(g2, k)]


def run_fixed_mul(lib, g2, fm, chunks, pairs):
    g, aw = fm.g, 32 if g2 else 16
    mults = (base_mult(0), base_mult(1))
    steps, step0 = plan(lib, g, chunks)
    assert_no_exceptional_case(g, walk_of(g, steps, step0), step0.tolist(), pairs, mults)
    bases = np.array([pt_words(g2, base_point(g2, s)) for s in range(2)], dtype=np.uint32)
    acc = pt_words(g2, mul_gen(g2, ACC_K))
    corr = pt_words(g2, mul_gen(g2, -(chunks - 1) * ACC_K)) if chunks > 1 else None
    lib.devtier_g16_fixed_mul.restype = ctypes.c_int
    for at in range(0, len(pairs), ROWS):
        rows = pairs[at:at + ROWS]
        sc = to_words([x for pr in rows for x in pr])
        out = np.zeros((len(rows), aw + 1), dtype=np.uint32)
        rc = lib.devtier_g16_fixed_mul(ctypes.c_int(g2), ctypes.c_uint32(g.wbits), ctypes.c_uint32(g.uneven), ptr(bases), ptr(sc), ctypes.c_uint32(len(rows)),
                                       ctypes.c_uint32(chunks), ptr(acc), ptr(corr), ptr(out))
        assert rc == 0, "devtier_g16_fixed_mul returned %d" % rc
        for r, (s0, s1) in enumerate(rows):
            want = mul_gen(g2, ACC_K + s0 * mults[0] + s1 * mults[1])
            assert want is not None and out[r].tolist() == pt_words(g2, want).tolist() + [0], \
                "%s %s chunks %d row %d: not acc_init + s_0 P_0 + s_1 P_1 for s = (%x, %x)" % ("G2" if g2 else "G1", fm.id, chunks, at + r, s0, s1)
