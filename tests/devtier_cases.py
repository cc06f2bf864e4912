"""Case generators and plain bigint references of the device tier (tests/devtier/devtier.hip), shared by its host leg
(tests/test_devtier_math.py) and its device leg (tests/test_gpu_devtier_math.py).

An operand is a vector of RAW LIMBS in the type's own layout.  The reference of an op is the integer the limbs denote, sum limb_i * 2^off_i,
pushed through the operation modulo the prime, compared exactly.  The limb and value bounds of every operand class are imported from the two
interval proofs (tests/test_fe_bounds.py, tests/test_fq_bounds.py) so that the proof and the run cannot drift apart: where the proof has a
checking function for an op (mul, sq, sub_k, mul_add2, reduce_weak, carry) the class is pushed through it when the op table is built, and the
bound it returns is the bound the result limbs are held to."""
import ctypes
import os
import random
import sys
from fractions import Fraction

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_fe_bounds as FEB  # noqa: E402
import test_fq_bounds as FQB  # noqa: E402
from oracle.py import bn254 as BN  # noqa: E402
from oracle.py import ristretto as RIS  # noqa: E402

N_RANDOM = 200

# ------------------------------------------------------------------------------------------------ primes and layouts
P25519 = 2**255 - 19
PQ = FQB.P
PR = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
P128 = 2**128 - 45 * 2**40 + 1
FE_OFF = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
FQ_OFF = [26 * i for i in range(10)]
N9_OFF = [29 * i for i in range(9)]
W8_OFF = [32 * i for i in range(8)]
R260, R261 = 1 << 260, 1 << 261


def val(limbs, off):
    return sum(int(x) << o for x, o in zip(limbs, off))


def canon(x, off):
    """x sliced at the layout's boundaries; the top limb holds the rest"""
    out = [(x >> off[i]) & ((1 << (off[i + 1] - off[i])) - 1) for i in range(len(off) - 1)]
    return out + [x >> off[-1]]


class Cls:
    """An operand class: inclusive limb maxima, the layout, an inclusive value maximum (None: the limbs alone bound it)"""

    def __init__(self, name, limbs, off, vmax=None):
        self.name, self.l, self.off = name, [int(x) for x in limbs], off
        full = val(self.l, off)
        self.vmax = full if vmax is None else min(int(vmax), full)

    def admits(self, limbs):
        return len(limbs) == len(self.l) and all(0 <= x <= m for x, m in zip(limbs, self.l)) and val(limbs, self.off) <= self.vmax

    def largest(self, zero=None):
        """the largest pattern inside both bounds (limb `zero` held at 0): from the top limb down, each limb as large as both allow"""
        rem, out = self.vmax, [0] * len(self.l)
        for i in reversed(range(len(self.l))):
            if i == zero:
                continue
            out[i] = min(self.l[i], rem >> self.off[i])
            rem -= out[i] << self.off[i]
        return out

    def single(self, i):
        out = [0] * len(self.l)
        out[i] = min(self.l[i], self.vmax >> self.off[i])
        return out

    def random(self, rnd):
        """uniform limbs; where the value bound is missed the top limbs are drawn again below what is left of it"""
        out = [rnd.randint(0, m) for m in self.l]
        if val(out, self.off) <= self.vmax:
            return out
        rem = rnd.randint(0, self.vmax)
        for i in reversed(range(len(self.l))):
            out[i] = min(out[i], rem >> self.off[i]) if i else min(self.l[0], rem)
            if i and rnd.random() < 0.5:
                out[i] = min(self.l[i], rem >> self.off[i])
            rem -= out[i] << self.off[i]
        return out


def edges(cls, p):
    """the fixed patterns of one operand class (every one inside the class; nothing is filtered at run time, the list is built once).
    "Each single limb at its maximum with the others zero, and the same with the others at maximum" is read as: limb i at its maximum
    and the rest zero (`single`), then limb i singled out the other way round, zero among limbs at their maximum (`largest(zero=i)`); every
    limb at its maximum together is the first pattern."""
    n, off = len(cls.l), cls.off
    out = [cls.largest()]
    out += [cls.single(i) for i in range(n)]
    out += [cls.largest(zero=i) for i in range(n)]
    cand = [canon(x, off) for x in (0, 1, 2, p - 1, p - 2, (p + 1) // 2, (p - 1) // 2, p, p + 1, 2 * p - 1)]
    for k in off[1:]:
        cand += [canon(1 << k, off), canon((1 << k) - 1, off)]
        i = off.index(k)
        unc = [0] * n
        unc[i - 1] = 1 << (k - off[i - 1])                   # 2^k left in the limb below its boundary: a carry that is still to come
        cand.append(unc)
    out += [c for c in cand if cls.admits(c)]
    assert all(cls.admits(c) for c in out), cls.name
    return out


class Op:
    """One op of one family: its id in the library's switch, the operand classes of the arrays a, b, c in order (an int n stands for a flag
    word with values 0..n-1), the reference on the operands' integer values, and how the result is held to it."""

    def __init__(self, fam, name, opid, arrays, ref, **kw):
        self.fam, self.name, self.opid, self.arrays, self.ref = fam, name, opid, arrays, ref
        self.exact = kw.get("exact", False)                 # the raw result's integer equals the reference (not only modulo the prime)
        self.out_l = kw.get("out_l")                        # inclusive limb maxima the header promises for the result
        self.out_v = kw.get("out_v")                        # inclusive value maximum
        self.extra = kw.get("extra", [])                    # further cases: tuples of operands
        self.kind = kw.get("kind")                          # family-specific result handling
        self.flat = [c for arr in arrays for c in arr]

    @property
    def id(self):
        return "%s.%s" % (self.fam, self.name)

    @property
    def out_words(self):
        return OUT_WORDS[self.fam]

    def pack(self, cases):
        return pack(self, cases)

    def build_cases(self):
        return build_cases(self, PRIME[self.fam], sum(self.id.encode()))


def build_cases(op, p, seed):
    """every operand through its fixed patterns with the others at their largest; the patterns against each other; the op's own pairs; 200
    seeded random draws inside the classes"""
    rnd = random.Random(seed)
    k = len(op.flat)
    E = [list(range(c)) if isinstance(c, int) else edges(c, p) for c in op.flat]
    top = [c - 1 if isinstance(c, int) else c.largest() for c in op.flat]
    cases = []
    for i in range(k):
        for e in E[i]:
            cases.append(tuple(e if j == i else top[j] for j in range(k)))
    for t in range(max(len(e) for e in E)):
        cases.append(tuple(E[j][(t * (2 * j + 1) + 3 * j) % len(E[j])] for j in range(k)))
    cases += [tuple(c) for c in op.extra]
    for _ in range(N_RANDOM):
        cases.append(tuple(rnd.randrange(c) if isinstance(c, int) else c.random(rnd) for c in op.flat))
    for c in cases:
        assert all((0 <= x < cl) if isinstance(cl, int) else cl.admits(x) for x, cl in zip(c, op.flat)), op.id
    return cases


def values(op, case):
    return [x if isinstance(cl, int) else val(x, cl.off) for x, cl in zip(case, op.flat)]


def pack(op, cases):
    """the three operand arrays of a case list as uint32 matrices (None for an unused array)"""
    arrs, at = [], 0
    for arr in op.arrays:
        if not arr:
            arrs.append(None)
            continue
        rows = []
        for c in cases:
            row = []
            for j in range(len(arr)):
                x = c[at + j]
                row += [x] if isinstance(x, int) else list(x)
            rows.append(row)
        arrs.append(np.array(rows, dtype=np.uint32))
        at += len(arr)
    while len(arrs) < 3:
        arrs.append(None)
    return arrs


OUT_WORDS = {"fe": 19, "fq": 18, "fq9": 18, "fr9": 17, "f128": 4, "sc": 16, "fp": 16}


def run(lib, op, cases, on_device):
    """one call of the op's family entry point over a case list; how the cases become the three operand arrays is the op's own business"""
    a, b, c = op.pack(cases)
    out = np.zeros((len(cases), op.out_words), dtype=np.uint32)
    ptr = lambda x: None if x is None else x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    fn = getattr(lib, "devtier_" + op.fam)
    fn.restype = ctypes.c_int
    rc = fn(ctypes.c_int(op.opid), ctypes.c_uint32(len(cases)), ptr(a), ptr(b), ptr(c), ptr(out), ctypes.c_int(on_device))
    assert rc == 0, "devtier_%s(%s) returned %d" % (op.fam, op.name, rc)
    return out


def load():
    import __graft_entry__ as ge
    return ctypes.CDLL(ge.build_devtier())


# ------------------------------------------------------------------------------------------------ fe25519
def _incl(excl):
    return [x - 1 for x in excl]


FE_CARRIED = Cls("carried", _incl(FEB.carried()), FE_OFF)
FE_LOOSE = Cls("loose", _incl(FEB.loose()), FE_OFF)
FE_SEMI = Cls("semi-loose", _incl(FEB.semi_loose()), FE_OFF)
FE_U32 = Cls("u32", [2**32 - 1] * 10, FE_OFF)
FE_HALF = Cls("u31", [2**31 - 1] * 10, FE_OFF)
FE_SUB_F = Cls("minuend", [2**32 - 1 - t for t in [0x7FFFFDA] + [0x3FFFFFE if i % 2 else 0x7FFFFFE for i in range(1, 10)]], FE_OFF)
FE_NEG = _incl(FEB.sub([1] * 10, FEB.carried()))            # limbs of 2p - carried
FEB.mul(FEB.loose(), FEB.semi_loose()); FEB.sq(FEB.semi_loose())     # the classes below are the ones the proof covers
assert all(a <= b for a, b in zip(FEB.sub(FEB.carried(), FEB.carried()), FEB.loose()))          # carried - carried is loose


def _inv_pairs(ca, cb, p, off, rfac, seed):
    """(a, b) with a b / rfac = 1 and = -1 mod p, a canonical and b canonical, and zero or a multiple of p on either side"""
    rnd = random.Random(seed)
    out = []
    for a in (2, p - 2, (p + 1) // 2, rnd.randrange(3, p), rnd.randrange(3, p)):
        inv = pow(a, p - 2, p)
        for t in (inv, p - inv, inv * rfac % p, (p - inv) * rfac % p):
            out += [(canon(a, off), canon(t, off)), (canon(t, off), canon(a, off))]
    z, m = canon(0, off), canon(p, off)
    out += [(z, cb.largest()), (ca.largest(), z), (z, z)]
    if ca.admits(m) and cb.admits(m):
        out += [(m, cb.largest()), (ca.largest(), m), (m, m)]
    return [c for c in out if ca.admits(c[0]) and cb.admits(c[1])]


def _sqrt_ref(u, v):
    return RIS.sqrt_ratio_m1(u % P25519, v % P25519)


FE_OPS = [
    Op("fe", "fe_mul", 0, [[FE_LOOSE], [FE_SEMI]], lambda a, b: a * b, out_l=FE_CARRIED.l, extra=_inv_pairs(FE_LOOSE, FE_SEMI, P25519, FE_OFF, 1, 11)),
    Op("fe", "fe_sq", 1, [[FE_SEMI]], lambda a: a * a, out_l=FE_CARRIED.l),
    Op("fe", "fe_add", 2, [[FE_HALF], [FE_HALF]], lambda a, b: a + b, exact=True),
    Op("fe", "fe_add_carried", 2, [[FE_CARRIED], [FE_CARRIED]], lambda a, b: a + b, exact=True, out_l=FE_LOOSE.l),
    Op("fe", "fe_sub", 3, [[FE_SUB_F], [FE_CARRIED]], lambda a, b: a + 2 * P25519 - b, exact=True),
    Op("fe", "fe_sub_carried", 3, [[FE_CARRIED], [FE_CARRIED]], lambda a, b: a + 2 * P25519 - b, exact=True, out_l=FE_LOOSE.l),
    Op("fe", "fe_neg", 4, [[FE_CARRIED]], lambda a: 2 * P25519 - a, exact=True, out_l=FE_NEG),
    Op("fe", "fe_carry", 5, [[FE_U32]], lambda a: a, out_l=FE_CARRIED.l),
    Op("fe", "fe_abs", 6, [[FE_U32]], lambda a: RIS._abs(a % P25519), out_l=[max(x, y) for x, y in zip(FE_NEG, FE_CARRIED.l)]),
    Op("fe", "fe_towords", 7, [[FE_U32]], lambda a: a, exact=True),
    Op("fe", "fe_pow22523", 8, [[FE_SEMI]], lambda a: pow(a, (P25519 - 5) // 8, P25519), out_l=FE_CARRIED.l),
    Op("fe", "fe_sqrt_ratio_m1", 9, [[FE_SEMI], [FE_SEMI]], _sqrt_ref, kind="sqrt",
       extra=[(canon(u, FE_OFF), canon(v, FE_OFF)) for u, v in ((0, 0), (0, 5), (5, 0), (1, 1), (4, 1), (2, 1), (1, 4), (P25519 - 1, 1), (1, P25519 - 1), (2, 4), (RIS.SQRT_M1, 1))]),
]


def check_fe(op, cases, out):
    for c, o in zip(cases, out):
        raw, words, flag = [int(x) for x in o[:10]], val(o[10:18], W8_OFF), int(o[18])
        ref = op.ref(*values(op, c))
        if op.kind == "sqrt":
            assert (bool(flag), words) == ref and val(raw, FE_OFF) % P25519 == ref[1], (op.id, c)
            continue
        got = val(raw, FE_OFF)
        assert (got == ref) if op.exact else (got % P25519 == ref % P25519), (op.id, c, raw)
        assert words == ref % P25519, (op.id, c, words)
        if op.out_l:
            assert all(x <= m for x, m in zip(raw, op.out_l)), (op.id, "result leaves its limb class", c, raw)


# ------------------------------------------------------------------------------------------------ bn254 fq (ten 26-bit limbs, R = 2^260)
def _fqcls(name, v):
    return Cls(name, v.l, FQ_OFF, v.val * PQ // 1000 - 1)


def _milli(x):
    return x * 1000 // PQ


K = FQB.C
V = FQB.V
FQ_MUL_IN = V([2**29 - 1] * 10, 15000)                      # limbs < 2^29; 15 p each keeps the product safe (the proof's own condition)
FQ_MADD_IN = V([2**28 - 1] * 10, 11000)
FQ_SUM_IN = V([2**30 - 1] * 10, _milli(1 << 259))
FQ_MINUEND = V([2**28 - 1] * 10, 16000)
FQ_SUB_B = {n: V([1 << (24 + n.bit_length() - 1)] * 9 + [K["fq_k%d" % n][9]], 1000 * n) for n in (4, 8, 16)}    # low limbs <= 2^26 / 2^27 / 2^28, value < n p
FQ_WIDE = V([2**31 - 1] * 10, _milli(1 << 260))             # fq_reduce_weak: limbs < 2^31, value < 2^260
FQ_CARRY_IN = V([2**32 - 1 - 2**6] * 10, _milli(1 << 260))  # fq_carry: the carry into a limb (< 2^6) must not wrap it
RINV260 = pow(R260, PQ - 2, PQ)
RINV261 = pow(R261, PQ - 2, PQ)


def _fq_out(v):
    return {"out_l": v.l, "out_v": v.val * PQ // 1000}


def _fq_ops():
    mul_in, madd_in = _fqcls("mul-in", FQ_MUL_IN), _fqcls("madd-in", FQ_MADD_IN)
    sum_in, minuend = _fqcls("sum-in", FQ_SUM_IN), _fqcls("minuend", FQ_MINUEND)
    wide, carry_in = _fqcls("wide", FQ_WIDE), _fqcls("carry-in", FQ_CARRY_IN)
    ops = [
        Op("fq", "fq_mul", 0, [[mul_in], [mul_in]], lambda a, b: a * b * RINV260, extra=_inv_pairs(mul_in, mul_in, PQ, FQ_OFF, R260, 21), **_fq_out(FQB.mul(FQ_MUL_IN, FQ_MUL_IN))),
        Op("fq", "fq_sq", 1, [[mul_in]], lambda a: a * a * RINV260, **_fq_out(FQB.sq(FQ_MUL_IN))),
        Op("fq", "fq_mul_add2", 2, [[madd_in, madd_in], [madd_in, madd_in]], lambda a, b, c, d: (a * b + c * d) * RINV260,
           extra=[(x, y, y, canon(PQ - val(x, FQ_OFF), FQ_OFF)) for x, y in _inv_pairs(madd_in, madd_in, PQ, FQ_OFF, R260, 22)[:16]],      # a b + b (p - a) = 0 mod p
           **_fq_out(FQB.mul_add2(FQ_MADD_IN, FQ_MADD_IN, FQ_MADD_IN, FQ_MADD_IN))),
        Op("fq", "fq_add_l", 3, [[sum_in], [sum_in]], lambda a, b: a + b, exact=True, **_fq_out(FQB.add_l(FQ_SUM_IN, FQ_SUM_IN))),
        Op("fq", "fq_dbl_l", 4, [[sum_in]], lambda a: 2 * a, exact=True, **_fq_out(FQB.dbl_l(FQ_SUM_IN))),
    ]
    for opid, n in ((5, 4), (6, 8), (7, 16)):
        sub_b = _fqcls("sub%d-b" % n, FQ_SUB_B[n])
        ops.append(Op("fq", "fq_sub_k%d" % n, opid, [[minuend], [sub_b]], (lambda n: lambda a, b: a + n * PQ - b)(n), exact=True, **_fq_out(FQB.sub_k(n, FQ_MINUEND, FQ_SUB_B[n]))))
    ops += [
        Op("fq", "fq_reduce_weak", 8, [[wide]], lambda a: a, **_fq_out(FQB.reduce_weak(FQ_WIDE))),
        Op("fq", "fq_carry", 9, [[carry_in]], lambda a: a, exact=True, **_fq_out(FQB.carry(FQ_CARRY_IN))),
        Op("fq", "fq_to_raw", 10, [[carry_in]], lambda a: a, exact=True),
        Op("fq", "fq_inv", 11, [[wide]], lambda a: pow(a, PQ - 2, PQ) * R260 * R260, out_l=FQB.SAFE.l, out_v=4 * PQ),
    ]
    # the "safe" (always reduced) operations: the operand classes of the comments beside them in bn254_fq.h -- limb sums below 2^31 for
    # fq_add / fq_dbl, the subtrahend of the 8p-borrowing subtraction for fq_sub / fq_neg -- pushed through the proof's limb-wise steps and
    # its weak reduction, so every result is held to FQB.SAFE
    sub_b = _fqcls("sub8-b", FQ_SUB_B[8])
    words = Cls("words", [2**32 - 1] * 8, W8_OFF)
    unpacked = V([FQB.M26] * 9 + [(2**256 - 1) >> 234], _milli(1 << 256) + 1)        # fq_unpack of any eight words
    r2 = V(K["fq_r2_l"], 1000)
    safe = {"out_l": FQB.SAFE.l, "out_v": FQB.SAFE.val * PQ // 1000 - 1}
    assert all(FQB.reduce_weak(v).val == FQB.SAFE.val for v in (FQB.add_l(FQ_SUM_IN, FQ_SUM_IN), FQB.sub_k(8, FQ_SUM_IN, FQ_SUB_B[8]), FQB.dbl_l(FQ_SUM_IN),
                                                                 FQB.sub_k(8, V([0] * 10, 0), FQ_SUB_B[8])))
    FQB.reduce_weak(FQ_WIDE); FQB.carry(FQB.reduce_weak(FQB.sub_k(8, FQ_SUM_IN, FQB.SAFE)))      # fq_eq: reduce b, subtract, reduce, canonical store
    ops += [
        Op("fq", "fq_add", 12, [[sum_in], [sum_in]], lambda a, b: a + b, **safe),
        Op("fq", "fq_sub", 13, [[sum_in], [sub_b]], lambda a, b: a - b, extra=[(canon(0, FQ_OFF), sub_b.largest())], **safe),
        Op("fq", "fq_neg", 14, [[sub_b]], lambda a: -a, **safe),
        Op("fq", "fq_dbl", 15, [[sum_in]], lambda a: 2 * a, **safe),
        Op("fq", "fq_from_raw", 16, [[words]], lambda a: a * R260, **_fq_out(FQB.mul(unpacked, r2))),
        Op("fq", "fq_eq", 17, [[sum_in], [wide]], lambda a, b: (a - b) % PQ == 0, kind="flag", extra=_eq_pairs(sum_in, wide)),
        Op("fq", "fq_is_zero", 18, [[carry_in]], lambda a: a % PQ == 0, kind="flag", extra=[(x,) for k in range(0, 80) for x in _reps(k * PQ, carry_in)]),
    ]
    return ops


def _reps(x, cls):
    """x as a carried limb vector and again with a unit of 2^26 left in each lower limb in turn (a carry still to come), where the class admits it"""
    l = canon(x, FQ_OFF)
    out = [l]
    for i in range(1, 10):
        if l[i]:
            u = list(l); u[i] -= 1; u[i - 1] += 1 << 26
            out.append(u)
    return [r for r in out if cls.admits(r)]


def _eq_pairs(ca, cb):
    """what the verdict kernels compare: zero as 0, p, 2p (and 3p - 1, which is not zero), one as 1, p + 1, 2p + 1, and values that differ
    in the top limb alone"""
    vals = [(a, b) for a in (0, PQ, 2 * PQ, 3 * PQ - 1) for b in (0, PQ, 2 * PQ)]
    vals += [(a, b) for a in (1, PQ + 1, 2 * PQ + 1) for b in (1, PQ + 1, 2 * PQ + 1)]
    one = R260 % PQ                                         # the field's one in Montgomery form, as fq2_one() has it
    vals += [(one + i * PQ, one + j * PQ) for i in range(3) for j in range(3)]
    low = (1 << 234) - 12345
    vals += [(low + (t << 234), low + (u << 234)) for t, u in ((0, 1), (1, 0), (PQ >> 234, 0), (0, PQ >> 234), (5, 5))]
    vals += [(low + (t << 234), low + (t << 234) + PQ) for t in (0, 1, 77)]
    return [(x, y) for a, b in vals for x in _reps(a, ca) for y in _reps(b, cb)[:4]]


FQ_OPS = _fq_ops()
assert FQB.reduce_weak(FQ_WIDE).val == FQB.SAFE.val and FQB.reduce_weak(FQ_WIDE).l == FQB.SAFE.l      # fq_reduce_weak returns SAFE


def check_fq(op, cases, out):
    for c, o in zip(cases, out):
        raw, words = [int(x) for x in o[:10]], val(o[10:18], W8_OFF)
        ref = op.ref(*values(op, c))
        if op.kind == "flag":                               # the predicate in word 0, the first operand's canonical words behind it
            assert raw == [int(ref)] + [0] * 9, (op.id, c, raw)
            assert words == values(op, c)[0] * RINV260 % PQ, (op.id, c, words)
            continue
        got = val(raw, FQ_OFF)
        assert (got == ref) if op.exact else (got % PQ == ref % PQ), (op.id, c, raw)
        assert words == ref * RINV260 % PQ, (op.id, c, words)
        if op.out_l:
            assert all(x <= m for x, m in zip(raw, op.out_l)) and got <= op.out_v, (op.id, "result leaves its class", c, raw)


# ------------------------------------------------------------------------------------------------ bn254 fq9 (nine 29-bit limbs, R = 2^261)
M29 = FQB.M29


def c9(name, vexcl, limb=M29, p=PQ):
    """carried9 below a value: limbs 0..7 <= 2^29 - 1 and the top limb what the value leaves"""
    return Cls(name, [limb] * 8 + [(vexcl - 1) >> 232], N9_OFF, vexcl - 1)


C9_261, C9_260, C9_259 = c9("carried9<2^261", R261), c9("carried9<2^260", R260), c9("carried9<2^259", 1 << 259)
K9 = FQB.header_constants9()
FAT = {k: [K9["fq9_k%d" % k][0] + (1 << 29)] + [K9["fq9_k%d" % k][i] + (1 << 29) - 1 for i in range(1, 8)] + [K9["fq9_k%d" % k][8] - 1] for k in (4, 8)}
G1B = FQB.G1_MMADD9_BOUNDS
# the loose operands of g1_mmadd9's fused Y3 (limb bounds from the proof): Q - X3 + 8p and 4p - Y1
C9_LOOSE8 = Cls("loose8", [FQB.LOOSE8_LIMB] * 8 + [(17 * PQ) >> 232], N9_OFF, 17 * PQ)
C9_LOOSE4 = Cls("loose4", [FQB.LOOSE4_LIMB] * 8 + [(4 * PQ) >> 232], N9_OFF, 4 * PQ)


def _below(k, num=1, den=1):
    return c9("carried9<%d/%dp" % (k * num, den), k * num * PQ // den)


def _fq9_ops():
    out261 = {"out_l": C9_261.l, "out_v": R261 - 1}
    ops = [
        Op("fq9", "fq9_mul", 0, [[C9_261], [C9_260]], lambda a, b: a * b * RINV261, extra=_inv_pairs(C9_261, C9_260, PQ, N9_OFF, R261, 31), **out261),
        Op("fq9", "fq9_sq", 1, [[C9_260]], lambda a: a * a * RINV261, **out261),
        Op("fq9", "fq9_mul_add2", 2, [[C9_260, C9_260], [C9_260, C9_260]], lambda a, b, c, d: (a * b + c * d) * RINV261,
           extra=[(x, y, y, canon(PQ - val(x, N9_OFF), N9_OFF)) for x, y in _inv_pairs(C9_260, C9_260, PQ, N9_OFF, R261, 32)[:16]], **out261),
        Op("fq9", "fq9_mul_add4", 3, [[C9_259] * 4, [C9_259] * 4], lambda a, b, c, d, e, f, g, h: (a * b + c * d + e * f + g * h) * RINV261, **out261),
        Op("fq9", "fq9_add", 4, [[C9_260], [C9_260]], lambda a, b: a + b, exact=True, **out261),
    ]
    for opid, k in ((5, 4), (6, 8), (7, 16)):
        ops.append(Op("fq9", "fq9_sub_k%d" % k, opid, [[C9_260], [_below(k)]], (lambda k: lambda a, b: a - b + k * PQ)(k), exact=True, **out261))
    ops += [
        Op("fq9", "fq9_sgn_sub_k8", 8, [[_below(4)], [_below(4)], [2]], lambda a, b, neg: (-a if neg else a) - b + 8 * PQ, exact=True, **out261),
        Op("fq9", "fq9_sub2_k4", 9, [[C9_260, _below(4, 1, 3)], [_below(4, 1, 3)]], lambda a, b, c: a - b - 2 * c + 4 * PQ, exact=True, **out261),
        Op("fq9", "fq9_sub2_k8", 10, [[C9_260, _below(8, 1, 3)], [_below(8, 1, 3)]], lambda a, b, c: a - b - 2 * c + 8 * PQ, exact=True, **out261),
        Op("fq9", "fq9_mul_add2_loose", 11, [[_below(6), C9_LOOSE8], [C9_LOOSE4, _below(2)]], lambda a, b, c, d: (a * b + c * d) * RINV261, **out261),
        # fq9_sub_loose<8>(Q, X3): X3 < 5.2 p is what the proof's top-limb argument for the loose difference rests on; fq9_neg_loose<4>(Y1): the
    # accumulator's Y bound
        Op("fq9", "fq9_sub_loose8", 12, [[_below(2)], [_below(52, 1, 10)]], lambda a, b: a - b + 8 * PQ, exact=True, out_l=[FQB.LOOSE8_LIMB] * 9, out_v=R261),
        Op("fq9", "fq9_neg_loose4", 13, [[_below(G1B["Y"])]], lambda a: 4 * PQ - a, exact=True, out_l=[FQB.LOOSE4_LIMB] * 9, out_v=4 * PQ),
        Op("fq9", "fq9_neg_k4", 14, [[_below(4)]], lambda a: 4 * PQ - a, exact=True, **out261),
        Op("fq9", "fq9_neg_k32", 15, [[_below(32)]], lambda a: 32 * PQ - a, exact=True, **out261),
        Op("fq9", "fq9_dbl_l", 16, [[C9_259]], lambda a: 2 * a, exact=True, out_l=[2 * M29] * 9, out_v=R261),
        Op("fq9", "fq9_reslice", 17, [[Cls("carried<2^261", [FQB.M26] * 9 + [(R261 - 1) >> 234], FQ_OFF, R261 - 1)]], lambda a: a, exact=True, **out261),
        Op("fq9", "fq_reslice", 18, [[C9_260]], lambda a: a, exact=True, kind="fq", out_l=[FQB.M26] * 9 + [2**32 - 1], out_v=R261),
        Op("fq9", "fq9_pack8", 19, [[c9("carried9<2^256", 1 << 256)]], lambda a: a, exact=True, kind="pack"),
        Op("fq9", "fq9_unpack8", 20, [[Cls("words", [2**32 - 1] * 8, W8_OFF)]], lambda a: a, exact=True, **out261),
        Op("fq9", "fq9_from_fq", 21, [[_fqcls("sum-in", FQ_SUM_IN)]], lambda a: 2 * a, out_l=C9_261.l, out_v=3 * PQ - 1),
        Op("fq9", "fq9_to_fq", 22, [[C9_261]], lambda a: a * RINV261 * R260, kind="fq", out_l=FQB.SAFE.l, out_v=3 * PQ - 1),
    ]
    return ops


FQ9_OPS = _fq9_ops()


def check_fq9(op, cases, out):
    for c, o in zip(cases, out):
        ref = op.ref(*values(op, c))
        if op.kind == "fq":
            raw, got, rinv = [int(x) for x in o[:10]], val(o[:10], FQ_OFF), RINV260
        else:
            raw, got, rinv = [int(x) for x in o[:9]], val(o[:9], N9_OFF), RINV261
        words = val(o[10:18], W8_OFF)
        assert (got == ref) if op.exact else (got % PQ == ref % PQ), (op.id, c, raw)
        if op.kind == "pack":
            assert words == ref, (op.id, c)
        else:
            assert words == ref * rinv % PQ, (op.id, c, words)
        if op.out_l:
            assert all(x <= m for x, m in zip(raw, op.out_l)) and got <= op.out_v, (op.id, "result leaves its class", c, raw)


# ------------------------------------------------------------------------------------------------ bn254 fr9 (nine 29-bit limbs mod r)
def r9(name, vexcl):
    return Cls(name, [M29] * 8 + [(vexcl - 1) >> 232], N9_OFF, vexcl - 1)


R9_261, R9_260 = r9("carried9<2^261", R261), r9("carried9<2^260", R260)
RRINV261 = pow(R261, PR - 2, PR)
FR9_OPS = [
    Op("fr9", "fr9_mul", 0, [[R9_261], [R9_260]], lambda a, b: a * b * RRINV261, extra=_inv_pairs(R9_261, R9_260, PR, N9_OFF, R261, 41), out_l=R9_261.l, out_v=R261 - 1),
    Op("fr9", "fr9_add", 1, [[R9_260], [R9_260]], lambda a, b: a + b, exact=True, out_l=R9_261.l, out_v=R261 - 1),
    Op("fr9", "fr9_sub_k2", 2, [[R9_260], [r9("carried9<2r", 2 * PR)]], lambda a, b: a - b + 2 * PR, exact=True, out_l=R9_261.l, out_v=R261 - 1),
    Op("fr9", "fr9_reduce_weak", 3, [[R9_261]], lambda a: a, out_l=R9_261.l, out_v=23 * PR // 10),
    Op("fr9", "fr9_from_fr", 4, [[Cls("words<2r", [2**32 - 1] * 8, W8_OFF, 2 * PR - 1)]], lambda a: 32 * a, out_l=R9_261.l, out_v=int(Fraction(64 * PR * PR, R261)) + PR),
    Op("fr9", "fr9_to_fr", 5, [[R9_261]], lambda a: a, exact=True),
]


def check_fr9(op, cases, out):
    for c, o in zip(cases, out):
        raw, words = [int(x) for x in o[:9]], val(o[9:17], W8_OFF)
        ref = op.ref(*values(op, c))
        got = val(raw, N9_OFF)
        assert (got == ref) if op.exact else (got % PR == ref % PR), (op.id, c, raw)
        assert words < 2 * PR and words % PR == ref * RRINV261 * (1 << 256) % PR, (op.id, c, words)     # fr9_to_fr: below 2r, Montgomery form with R = 2^256
        if op.out_l:
            assert all(x <= m for x, m in zip(raw, op.out_l)) and got <= op.out_v, (op.id, "result leaves its class", c, raw)


# ------------------------------------------------------------------------------------------------ f128 (canonical in, canonical out)
C128 = 45 * 2**40 - 1
M64 = 2**64 - 1
F128_CLS = Cls("canonical", [2**32 - 1] * 4, [0, 32, 64, 96], P128 - 1)


def f128_walk(a, b):
    """f128_mul's own steps on bigints: the number of wraps past 2^128 its sum takes, whether adding 2^128 mod p wrapped once more, the
    high words of the four partial products, and the result"""
    alo, ahi, blo, bhi = a & M64, a >> 64, b & M64, b >> 64
    highs = [(alo * blo) >> 64, (ahi * bhi) >> 64, (alo * bhi) >> 64, (ahi * blo) >> 64]
    w = a * b
    wlo, whi = w & (2**128 - 1), w >> 128
    t = whi * C128
    t2, tlo = t >> 128, t & (2**128 - 1)
    s = wlo + tlo + t2 * C128
    wraps, r = s >> 128, s & (2**128 - 1)
    again, todo = 0, wraps
    while todo:
        todo -= 1
        r += C128
        if r >> 128:
            r &= 2**128 - 1
            again += 1
            todo += 1
    if r >= P128:
        r -= P128
    assert r == a * b % P128
    return wraps, again, highs, r


def f128_target_pair(target, seed, want):
    """a pair whose sum of partial words S is exactly `target` (S = a b mod p in general): b = target / a for seeded a until the walk agrees"""
    rnd = random.Random(seed)
    for _ in range(4000):
        a = rnd.randrange(P128 - 2**100, P128)
        b = target % P128 * pow(a, P128 - 2, P128) % P128
        w = f128_walk(a, b)
        if want(w):
            return a, b
    raise AssertionError("no pair found for the wanted carry structure")


def f128_two_wraps():
    """A pair whose sum wraps 2^128 twice.  The sum is lo(a b) + lo(hi(a b) C) + t2 C with t2 C < 2^92, so both 128-bit terms must lie within
    2^92 of 2^128: with lo(a b) = 2^128 - rho and hi(a b) C = -s (mod 2^128), b = -(rho C + s 2^128) / (a C) mod 2^256 for a fixed odd a.
    A reduced basis of the lattice {(rho 2^62, s 2^62, b)} gives rho, s near 2^65 -- far below t2 C, about 2^91 -- with b near 2^127."""
    M, sc = 1 << 256, 62
    rnd = random.Random(77)
    while True:
        a = rnd.randrange(P128 - 2**120, P128) | 1
        inv = pow(a * C128, -1, M)
        u, v = (-C128 * inv) % M, (-(1 << 128) * inv) % M
        basis = _lll3([[1 << sc, 0, u], [0, 1 << sc, v], [0, 0, M]])
        for x in range(-6, 7):
            for y in range(-6, 7):
                for z in range(-6, 7):
                    vec = [x * basis[0][i] + y * basis[1][i] + z * basis[2][i] for i in range(3)]
                    rho, s, b = vec[0] >> sc, vec[1] >> sc, vec[2]
                    if rho > 0 and s > 0 and 0 < b < P128 and f128_walk(a, b)[0] == 2:
                        return a, b


def f128_wrap_again():
    """A pair whose sum S takes one wrap and ends within 2^128 mod p (= C) below 2^129, so that adding C for the wrap wraps once more.  With
    rho, s as in f128_two_wraps, t2 is linear in (a b, rho, s) and S - 2^129 = t2 C - rho - s must lie in [-C, -1]: a closest-vector problem
    in the same lattice with that quantity as a fourth coordinate (coordinates weighted by the room each has), solved by rounding in a reduced
    basis; the candidates next to the rounded point are walked until one lands in the branch."""
    M, C = 1 << 256, C128
    rnd = random.Random(5)
    dot = lambda x, y: sum(Fraction(p) * q for p, q in zip(x, y))  # noqa: E731
    lam, mu = 1 << 211, 1 << 174
    while True:
        a = rnd.randrange(P128 - 2**120, P128) | 1
        inv = pow(a * C, -1, M)
        u, v = (-C * inv) % M, (-(1 << 128) * inv) % M
        B = _lll3([[lam, 0, u * mu, (C * C - M) + C * C * a * u], [0, lam, v * mu, (C << 128) - M + C * C * a * v], [0, 0, M * mu, C * C * a * M]])
        t = [Fraction(lam << 89), Fraction(lam << 89), Fraction(mu << 127), Fraction((C * C << 128) + (C // 2) * M)]
        bs = []
        for i in range(3):
            w = [Fraction(x) for x in B[i]]
            for j in range(i):
                m = dot(B[i], bs[j]) / dot(bs[j], bs[j])
                w = [p - m * q for p, q in zip(w, bs[j])]
            bs.append(w)
        coef = [0, 0, 0]
        for i in (2, 1, 0):
            coef[i] = round(dot(t, bs[i]) / dot(bs[i], bs[i]))
            t = [p - coef[i] * q for p, q in zip(t, B[i])]
        for d in ((x, y, z) for x in range(-4, 5) for y in range(-4, 5) for z in range(-4, 5)):
            vec = [sum((coef[i] + d[i]) * B[i][k] for i in range(3)) for k in range(4)]
            rho, s, b = vec[0] // lam, vec[1] // lam, vec[2] // mu
            if rho > 0 and s > 0 and 0 < b < P128 and f128_walk(a, b)[:2] == (1, 1):
                return a, b


def _lll3(b):
    """Lenstra-Lenstra-Lovasz reduction of three integer vectors of any length (exact rationals; delta = 3/4)"""
    b = [list(r) for r in b]
    dot = lambda x, y: sum(Fraction(p) * q for p, q in zip(x, y))  # noqa: E731

    def gso():
        bs, mu = [], [[Fraction(0)] * 3 for _ in range(3)]
        for i in range(3):
            v = [Fraction(x) for x in b[i]]
            for j in range(i):
                mu[i][j] = dot(b[i], bs[j]) / dot(bs[j], bs[j])
                v = [p - mu[i][j] * q for p, q in zip(v, bs[j])]
            bs.append(v)
        return bs, mu
    k = 1
    while k < 3:
        for j in reversed(range(k)):
            bs, mu = gso()
            q = round(mu[k][j])
            if q:
                b[k] = [p - q * r for p, r in zip(b[k], b[j])]
        bs, mu = gso()
        if dot(bs[k], bs[k]) >= (Fraction(3, 4) - mu[k][k - 1] ** 2) * dot(bs[k - 1], bs[k - 1]):
            k += 1
        else:
            b[k], b[k - 1] = b[k - 1], b[k]
            k = max(k - 1, 1)
    return b


def f128_built_pairs():
    """operand pairs built backwards from f128_mul's carry structure; each is asserted, with the bigint walk alone, to land where it claims"""
    out = {}
    out["wraps0"] = (3, 5)
    out["wraps1"] = f128_target_pair(2**128 + 12345, 51, lambda w: w[0] == 1 and w[1] == 0)
    out["wraps2"] = f128_two_wraps()
    # the sum ends within 2^128 mod p below 2^129: one wrap, and adding 2^128 mod p for it wraps once more
    out["wraps_again"] = f128_wrap_again()
    # a partial product's high word is at most 2^64 - 2 (from (2^64 - 1)^2); canonical operands reach it in each of the four products
    out["high_lo_lo"] = (M64, M64)
    out["high_hi_hi"] = (M64 << 64, M64 << 64)
    out["high_lo_hi"] = (M64, M64 << 64)
    out["high_hi_lo"] = (M64 << 64, M64)
    assert f128_walk(*out["wraps0"])[0] == 0 and f128_walk(*out["wraps1"])[:2] == (1, 0) and f128_walk(*out["wraps2"])[0] == 2
    assert f128_walk(*out["wraps_again"])[:2] == (1, 1)
    for i, k in enumerate(("high_lo_lo", "high_hi_hi", "high_lo_hi", "high_hi_lo")):
        assert f128_walk(*out[k])[2][i] == 2**64 - 2 and all(x < P128 for x in out[k])
    return out


F128_BUILT = f128_built_pairs()
_F128_OFF = [0, 32, 64, 96]
_f128_extra = [(canon(a, _F128_OFF), canon(b, _F128_OFF)) for a, b in F128_BUILT.values()]
_f128_extra += [(b, a) for a, b in _f128_extra]
F128_OPS = [
    Op("f128", "f128_mul", 0, [[F128_CLS], [F128_CLS]], lambda a, b: a * b, extra=_f128_extra + _inv_pairs(F128_CLS, F128_CLS, P128, _F128_OFF, 1, 53)),
    Op("f128", "f128_add", 1, [[F128_CLS], [F128_CLS]], lambda a, b: a + b, extra=[(canon(a, _F128_OFF), canon(P128 - a, _F128_OFF)) for a in (1, 2, C128, C128 + 1, 2**64, 2**127)]),
    Op("f128", "f128_sub", 2, [[F128_CLS], [F128_CLS]], lambda a, b: a - b, extra=[(canon(a, _F128_OFF), canon(a, _F128_OFF)) for a in (0, 1, P128 - 1, 2**64)]),
    Op("f128", "f128_neg", 3, [[F128_CLS]], lambda a: -a),
]


def check_f128(op, cases, out):
    for c, o in zip(cases, out):
        assert val(o, _F128_OFF) == op.ref(*values(op, c)) % P128, (op.id, c)


# ------------------------------------------------------------------------------------------------ all field families
FIELD_OPS = FE_OPS + FQ_OPS + FQ9_OPS + FR9_OPS + F128_OPS
PRIME = {"fe": P25519, "fq": PQ, "fq9": PQ, "fr9": PR, "f128": P128}
CHECK = {"fe": check_fe, "fq": check_fq, "fq9": check_fq9, "fr9": check_fr9, "f128": check_f128}
_CASES = {}


def cases_of(op):
    """the case list of an op, built once and shared by both legs"""
    if op.id not in _CASES:
        _CASES[op.id] = op.build_cases()
    return _CASES[op.id]


# ------------------------------------------------------------------------------------------------ the MSM loops' point steps
# The accumulator is a known multiple of the generator brought in with Z != 1 (a Jacobian or XYZZ representative with a seeded z); every
# coordinate, in the form's Montgomery representation, is re-expressed inside its bound class: the canonical residue, the residue plus the
# largest multiple of p the class admits, or a seeded multiple.  The expected result is the bigint curve sum.  The BN254 lazy additions
# have no exceptional cases by design, so the multiples are chosen so that no case adds P to +-P or reaches infinity; that is asserted
# over the whole list when it is built, and nothing is filtered afterwards.
class PointOp:
    fam = "point"

    def __init__(self, name, opid, curve, gen, R, off, acc_bounds, ent_bounds, out_bounds, xyzz):
        self.name, self.opid, self.curve, self.gen, self.R, self.off = name, opid, curve, gen, R, off
        self.acc_bounds, self.ent_bounds, self.out_bounds, self.xyzz = acc_bounds, ent_bounds, out_bounds, xyzz
        self.g2 = curve is BN.G2C
        self.nl = len(off)
        self.out_words = (len(acc_bounds) * self.nl + 16 + 1) * (2 if self.g2 else 1) - (1 if self.g2 else 0)

    @property
    def id(self):
        return "point." + self.name

    def pack(self, cases):
        return [np.array([c[0] for c in cases], dtype=np.uint32), np.array([c[1] for c in cases], dtype=np.uint32), np.array([[c[2]] for c in cases], dtype=np.uint32)]

    def build_cases(self):
        return point_cases(self)


_MULT = {}


def _multiples(curve, gen, n=48):
    key = id(curve)
    if key not in _MULT:
        t = [None]
        for _ in range(n):
            t.append(curve.add_pts(t[-1], gen))
        _MULT[key] = t
    return _MULT[key]


def _rep(x, R, bound, off, level, rnd):
    """the limbs of the field element x in Montgomery form, as a carried representative inside value < bound p"""
    num, den = bound
    v0 = x * R % PQ
    mmax = (num * PQ // den - 1 - v0) // PQ
    m = (0, mmax, rnd.randint(0, mmax))[level]
    return canon(v0 + m * PQ, off)


def _comps(op, e):
    return list(e) if op.g2 else [e]


def point_cases(op):
    rnd = random.Random(1000 + op.opid)
    c, T = op.curve, _multiples(op.curve, op.gen)
    F = c                                                   # the curve object carries its field's arithmetic
    cases = []
    plan = [(ka, ke, neg, lvl) for ka in (1, 2, 3, 7, 19, 40) for ke in (5, 11, 23) for neg in (0, 1) for lvl in (0, 1, 2)]
    plan += [(rnd.randint(1, 47), rnd.randint(1, 47), rnd.randint(0, 1), rnd.randint(0, 2)) for _ in range(N_RANDOM)]
    for ka, ke, neg, lvl in plan:
        if ka == ke:
            ke = ke % 47 + 1
        assert ka % BN.R not in (ke % BN.R, -ke % BN.R) and ka % BN.R and ke % BN.R            # never P +- P, never infinity in or out
        (x, y), ent = T[ka], T[ke]
        z = None
        while z is None or z == F.zero or z == F.one:
            z = tuple(rnd.randrange(PQ) for _ in range(2)) if op.g2 else rnd.randrange(1, PQ)
        zz = F.sq(z); zzz = F.mul(zz, z)
        coords = [F.mul(x, zz), F.mul(y, zzz)] + ([zz, zzz] if op.xyzz else [z])
        acc, entl = [], []
        for e, b in zip(coords, op.acc_bounds):
            for comp in _comps(op, e):
                acc += _rep(comp, op.R, b, op.off, lvl, rnd)
        for e, b in zip(ent, op.ent_bounds):
            for comp in _comps(op, e):
                entl += _rep(comp, op.R, b, op.off, lvl, rnd)
        want = c.add_pts(T[ka], c.neg_pt(ent) if neg else ent)
        kr = ka - ke if neg else ka + ke
        assert want is not None and (not 0 < kr < len(T) or want == T[kr])
        cases.append((acc, entl, neg, want))
    return cases


def check_point(op, cases, out):
    F, nl, nc = op.curve, op.nl, 2 if op.g2 else 1
    rinv = pow(op.R, PQ - 2, PQ)
    for case, o in zip(cases, out):
        want = case[3]
        ncoord = len(op.acc_bounds)
        raw = [[[int(x) for x in o[(k * nc + j) * nl:(k * nc + j + 1) * nl]] for j in range(nc)] for k in range(ncoord)]
        base = ncoord * nc * nl
        words = [val(o[base + 8 * i:base + 8 * i + 8], W8_OFF) for i in range(2 * nc)]
        inf = int(o[base + 16 * nc])
        aff = (tuple(words[:2]), tuple(words[2:])) if op.g2 else tuple(words)
        assert inf == 0 and aff == want, (op.id, "affine result", case[2], aff, want)
        # the raw coordinates, by bigints alone: inside the bounds the header gives for the next iteration, and the same point
        el = []
        for k in range(ncoord):
            num, den = op.out_bounds[k]
            for j in range(nc):
                v = val(raw[k][j], op.off)
                assert all(x < (1 << (op.off[1] - op.off[0])) for x in raw[k][j][:-1]) and v * den < num * PQ, (op.id, "coordinate %d leaves its class" % k, raw[k][j])
            vs = [val(r, op.off) * rinv % PQ for r in raw[k]]
            el.append(tuple(vs) if op.g2 else vs[0])
        if op.xyzz:
            X, Y, ZZ, ZZZ = el
            assert F.mul(F.sq(ZZ), ZZ) == F.sq(ZZZ), (op.id, "ZZ^3 != ZZZ^2")
            got = (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ)))
        else:
            X, Y, Z = el
            zi = F.inv(Z); zi2 = F.sq(zi)
            got = (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi)))
        assert got == want, (op.id, "raw coordinates denote another point")


_SAFE, _CANON = (FQB.SAFE.val, 1000), (FQB.CANON.val, 1000)
_G1B = {k: (v, 1) for k, v in FQB.G1_MMADD9_BOUNDS.items()}
_G2B = FQB.G2_MMADD9_BOUNDS
POINT_OPS = [
    PointOp("g1_madd_lazy", 0, BN.G1C, BN.G1, R260, FQ_OFF, [_SAFE] * 3, [_CANON] * 2, [_SAFE] * 3, False),
    PointOp("g1_mmadd_lazy", 1, BN.G1C, BN.G1, R260, FQ_OFF, [_SAFE] * 4, [_CANON] * 2, [_SAFE] * 4, True),
    PointOp("g1_mmadd9", 2, BN.G1C, BN.G1, R261, N9_OFF, [_G1B[k] for k in ("X", "Y", "ZZ", "ZZZ")], [_G1B["qx"], _G1B["qy"]],
            [_G1B["X"], _G1B["Y"], (2, 1), (2, 1)], True),
    PointOp("g2_madd_lazy", 3, BN.G2C, BN.G2, R260, FQ_OFF, [_SAFE] * 3, [_CANON] * 2, [_SAFE] * 3, False),
    PointOp("g2_mmadd9", 4, BN.G2C, BN.G2, R261, N9_OFF, [_G2B[k] for k in ("X", "Y", "ZZ", "ZZZ")], [_G2B["q"]] * 2,
            [_G2B["X"], _G2B["Y"], (2, 1), (2, 1)], True),
]
CHECK["point"] = check_point
# ------------------------------------------------------------------------------------------------ sc25519 (eight 32-bit words mod l, R = 2^256)
LSC = RIS.L
R256 = 1 << 256
SC_LT_L = Cls("below l", [2**32 - 1] * 8, W8_OFF, LSC - 1)                 # Montgomery form is always fully reduced
SC_ANY = Cls("any 256 bits", [2**32 - 1] * 8, W8_OFF)                     # sc_montmul's first operand, sc_from_raw256
SC_RAW253 = Cls("raw below 2^253", [2**32 - 1] * 8, W8_OFF, 2**253 - 1)   # the recodings' "canonical raw scalar (< 2^253)"
SC_WIDE = Cls("512 bits", [2**32 - 1] * 16, [32 * i for i in range(16)])
SC_RINV = pow(R256, LSC - 2, LSC)


def _sc_inv(a):
    return pow(a, LSC - 2, LSC) * R256 * R256                             # (a R)^-1 R^2 = a^-1 R; 0 for a = 0


def _digits(words, nd):
    d = [(int(words[j >> 1]) >> (16 * (j & 1))) & 0xFFFF for j in range(nd)]
    return [x - 65536 if x >= 32768 else x for x in d]


SC_OPS = [
    Op("sc", "sc_mul", 0, [[SC_ANY], [SC_LT_L]], lambda a, b: a * b * SC_RINV, extra=_inv_pairs(SC_ANY, SC_LT_L, LSC, W8_OFF, R256, 61)),
    Op("sc", "sc_add", 1, [[SC_LT_L], [SC_LT_L]], lambda a, b: a + b, extra=[(canon(a, W8_OFF), canon(LSC - a, W8_OFF)) for a in (1, 2, LSC - 1, 2**252)]),
    Op("sc", "sc_sub", 2, [[SC_LT_L], [SC_LT_L]], lambda a, b: a - b, extra=[(canon(a, W8_OFF), canon(a, W8_OFF)) for a in (0, 1, LSC - 1)]),
    Op("sc", "sc_neg", 3, [[SC_LT_L]], lambda a: -a),
    Op("sc", "sc_invert", 4, [[SC_LT_L]], _sc_inv),
    Op("sc", "sc_invert_fermat", 5, [[SC_LT_L]], _sc_inv),
    Op("sc", "sc_from_wide", 6, [[SC_WIDE]], lambda a: a * R256),
    Op("sc", "sc_recode_signed1024", 7, [[SC_RAW253]], lambda a: a, kind=(26, 10, -511, 512)),
    Op("sc", "sc_recode_signed65536", 8, [[SC_RAW253]], lambda a: a, kind=(16, 16, -32768, 32767)),
    Op("sc", "sc_from_raw256", 9, [[SC_ANY]], lambda a: a * R256),
    Op("sc", "sc_to_raw", 10, [[SC_LT_L]], lambda a: a),
]


def check_sc(op, cases, out):
    for c, o in zip(cases, out):
        ref = op.ref(*values(op, c))
        if op.kind:                                                       # a recoding: digits inside their range that sum to the scalar
            nd, wb, lo, hi = op.kind
            d = _digits(o, nd)
            assert all(lo <= x <= hi for x in d) and sum(x << (wb * j) for j, x in enumerate(d)) == ref, (op.id, c, d)
            assert all(int(x) == 0 for x in o[(nd + 1) // 2:]), (op.id, "words past the digits", c)
            continue
        assert val(o[:8], W8_OFF) == ref % LSC, (op.id, c)                  # fully reduced, so equal as integers
        assert val(o[8:16], W8_OFF) == ref * SC_RINV % LSC, (op.id, c)


# ------------------------------------------------------------------------------------------------ Fp<FrParams> (eight 32-bit words mod r, R = 2^256, values below 2r)
FP_LT_2R = Cls("below 2r", [2**32 - 1] * 8, W8_OFF, 2 * PR - 1)
FP_LT_R = Cls("below r", [2**32 - 1] * 8, W8_OFF, PR - 1)
FP_ANY = Cls("any 256 bits", [2**32 - 1] * 8, W8_OFF)
# the second operand beside a 256-bit first one: the row carry floor((a b_i + t) / 2^256) <= b_i + 1 and t[8] <= 1 are added in 32 bits
# (fp_mul's t8), so b_i <= 2^32 - 3; at b_i = 2^32 - 1 and a = 2^256 - 1 the sum wraps (seen on the host leg)
FP_LT_R_NARROW = Cls("below r, words below 2^32 - 2", [2**32 - 3] * 8, W8_OFF, PR - 1)
FP_RINV = pow(R256, PR - 2, PR)
# fr_glv_split's lattice basis (bn254_g.h): (A1, -NB1) is in {(a, b): a + b lambda = 0 mod r}, which gives lambda
_GLV_A1, _GLV_NB1 = 0x89d3256894d213e3, 0x6f4d8248eeb859fc8211bbeb7d4f1128
GLV_LAMBDA = _GLV_A1 * pow(_GLV_NB1, PR - 2, PR) % PR
assert (GLV_LAMBDA * GLV_LAMBDA + GLV_LAMBDA + 1) % PR == 0
FP_OPS = [
    Op("fp", "fp_mul", 0, [[FP_LT_2R], [FP_LT_2R]], lambda a, b: a * b * FP_RINV, extra=_inv_pairs(FP_LT_2R, FP_LT_2R, PR, W8_OFF, R256, 71)),
    Op("fp", "fp_mul_wide_operand", 0, [[FP_ANY], [FP_LT_R_NARROW]], lambda a, b: a * b * FP_RINV),          # "or a < 2^256 with b < p ..."
    Op("fp", "fp_add", 1, [[FP_LT_2R], [FP_LT_2R]], lambda a, b: a + b),
    Op("fp", "fp_sub", 2, [[FP_LT_2R], [FP_LT_2R]], lambda a, b: a - b, extra=[(canon(a, W8_OFF), canon(a, W8_OFF)) for a in (0, 1, PR, 2 * PR - 1)]),
    Op("fp", "fp_neg", 3, [[FP_LT_2R]], lambda a: -a),
    Op("fp", "fp_inv", 4, [[FP_LT_2R]], lambda a: pow(a, PR - 2, PR) * R256 * R256),
    Op("fp", "fp_from_wide", 5, [[SC_WIDE]], lambda a: a * R256),
    Op("fp", "fr_glv_split", 6, [[FP_LT_R]], lambda a: a, kind="glv"),
    Op("fp", "fp_from_raw", 7, [[FP_ANY]], lambda a: a * R256),
    Op("fp", "fp_to_raw", 8, [[FP_LT_2R]], lambda a: a),
]


def check_fp(op, cases, out):
    for c, o in zip(cases, out):
        ref = op.ref(*values(op, c))
        if op.kind == "glv":                                              # k = k1 + k2 lambda mod r with both halves below 2^128
            k1, k2 = val(o[0:4], W8_OFF[:4]) * (-1 if o[4] else 1), val(o[5:9], W8_OFF[:4]) * (-1 if o[9] else 1)
            assert int(o[4]) < 2 and int(o[9]) < 2 and (k1 + k2 * GLV_LAMBDA - ref) % PR == 0, (op.id, c, k1, k2)
            continue
        got = val(o[:8], W8_OFF)
        assert got < 2 * PR and got % PR == ref % PR, (op.id, c, got)        # every result stays below 2r
        assert val(o[8:16], W8_OFF) == ref * FP_RINV % PR, (op.id, c)


# ------------------------------------------------------------------------------------------------ ed25519 group steps
# The formulas are complete, so beside ordinary pairs the cases are the ones the BN254 steps must avoid: acc = entry, acc = -entry, acc
# neutral (and a neutral second operand for ge_add).  Points are known multiples of the basepoint with Z != 1; every coordinate is a carried
# limb vector, canonical or with units of 2^25 borrowed down into odd limbs (a carried, non-canonical representative of the same integer).
D2 = 2 * RIS.D % P25519


def _fe_limbs(x, level):
    l = canon(x % P25519, FE_OFF)
    if level:
        for i in (1, 3, 5, 7):
            if l[i] < 2**18 - 1 and l[i + 1] >= 1:
                l[i] += 2**25
                l[i + 1] -= 1
    assert FE_CARRIED.admits(l) and val(l, FE_OFF) == x % P25519
    return l


def _affine(pt):
    zi = pow(pt.Z, P25519 - 2, P25519)
    return pt.X * zi % P25519, pt.Y * zi % P25519


class GeOp:
    fam, out_words = "ge", 48

    def __init__(self, name, opid, second):
        self.name, self.opid, self.second = name, opid, second

    @property
    def id(self):
        return "ge." + self.name

    def pack(self, cases):
        a = np.array([c[0] for c in cases], dtype=np.uint32)
        b = np.array([c[1] for c in cases], dtype=np.uint32) if self.second else None
        c = np.array([[c[2]] for c in cases], dtype=np.uint32) if self.second == "entry" else None
        return [a, b, c]

    def build_cases(self):
        rnd = random.Random(300 + self.opid)
        T = [RIS.IDENTITY]
        for _ in range(64):
            T.append(T[-1] + RIS.BASEPOINT)
        mul = lambda k: T[k] if k >= 0 else -T[-k]  # noqa: E731
        plan = [(ka, ke, neg) for ka in (0, 1, 2, 7, 31) for ke in (1, 2, 7, 31) for neg in (0, 1)]          # holds acc = entry, acc = -entry, acc neutral
        plan += [(ka, 0, 0) for ka in (0, 1, 5)] if self.second == "extended" else []                         # a neutral second operand
        plan += [(rnd.randint(0, 32), rnd.randint(1, 32), rnd.randint(0, 1)) for _ in range(N_RANDOM)]
        assert {(1, 1, 0), (1, 1, 1), (0, 1, 0)} <= set(plan)
        cases = []
        for n, (ka, ke, neg) in enumerate(plan):
            lvl = n % 2
            x, y = _affine(mul(ka))
            z = rnd.randrange(2, P25519)
            acc = sum((_fe_limbs(v, lvl) for v in (x * z, y * z, z, x * y * z)), [])
            ex, ey = _affine(mul(ke))
            if self.second == "niels":
                if neg:
                    ex = -ex % P25519
                b, want = sum((_fe_limbs(v, lvl) for v in (ey + ex, ey - ex, D2 * ex * ey)), []), mul(ka) + mul(-ke if neg else ke)
            elif self.second == "extended":
                if neg:
                    ex = -ex % P25519
                w = rnd.randrange(2, P25519)
                b, want = sum((_fe_limbs(v, lvl) for v in (ex * w, ey * w, w, ex * ey * w)), []), mul(ka) + mul(-ke if neg else ke)
            elif self.second == "entry":                                     # the packed table entry: three canonical 255-bit integers
                b = [(v % P25519 >> (32 * i)) & 0xFFFFFFFF for v in (ey + ex, ey - ex, D2 * ex * ey) for i in range(8)]
                want = mul(ka) + mul(-ke if neg else ke)
            else:
                b, want = None, (mul(ka).double() if self.name == "ge_dbl" else mul(ka))
            cases.append((acc, b, neg, want))
        return cases


GE_OPS = [GeOp("ge_madd", 0, "niels"), GeOp("ge_add", 1, "extended"), GeOp("ge_dbl", 2, None), GeOp("edg_accumulate", 3, "entry"), GeOp("ge_ristretto_encode", 4, None)]


def check_ge(op, cases, out):
    for case, o in zip(cases, out):
        want = case[3]
        raw = [[int(x) for x in o[10 * k:10 * k + 10]] for k in range(4)]
        assert all(FE_CARRIED.admits(r) for r in raw), (op.id, "a coordinate is not carried", raw)
        X, Y, Z, T = (val(r, FE_OFF) % P25519 for r in raw)
        assert Z and (T * Z - X * Y) % P25519 == 0, (op.id, "T is not X Y / Z")
        zi = pow(Z, P25519 - 2, P25519)
        assert (X * zi % P25519, Y * zi % P25519) == _affine(want), (op.id, "another point", case[2])
        assert val(o[40:48], W8_OFF) == int.from_bytes(want.encode(), "little"), (op.id, "ristretto encoding")


FIELD_OPS += SC_OPS + FP_OPS
PRIME.update({"sc": LSC, "fp": PR})
CHECK.update({"sc": check_sc, "fp": check_fp, "ge": check_ge})
ALL_OPS = FIELD_OPS + POINT_OPS + GE_OPS
