"""Case generators and bigint references of the device tier of the Groth16 verifier's arithmetic (tests/devtier/devtier_pairing.hip), shared by
its host leg (tests/test_devtier_pairing.py) and its device leg (tests/test_gpu_devtier_pairing.py).

Family fq2: every arithmetic opcode of the Fq2 machine through fq2vm::alu, operands as raw limbs in the class tests/test_fq_bounds.py proves
the operations closed over (FQB.FQ2_CLASS: carried, below 3p).  Family fq12: the lane-per-chain tower of bn254_pairing.h against the oracle's
polynomial-basis Fq12.  The Fq2 machine: each chain of fq2vm_programs.h on a slot buffer, the device interpreter against the host one word for
word, and the bigint meaning of what a chain leaves.  All references are oracle/py bigints."""
import ctypes
import math
import os
import random
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tools"))
import devtier_cases as DC  # noqa: E402
from devtier_cases import Cls, Op, FQB, BN, PQ, FQ_OFF, W8_OFF, R260, RINV260, canon, val, edges, values, _rep, _fqcls  # noqa: E402,F401
import gen_fq2vm as GEN  # noqa: E402  (the tower's coefficient order, the Frobenius constants, the slot numbers, the Fq2 square root)

X = GEN.X
assert (GEN.P, GEN.R) == (PQ, BN.R)
SAFE = _fqcls("fq2-component", FQB.FQ2_CLASS)               # the class of every Fq2 component in this file
SAFE_B = (FQB.FQ2_CLASS.val, 1000)                          # the same as a bound for _rep


def load():
    import __graft_entry__ as ge
    return ctypes.CDLL(ge.build_devtier_pairing())


def mont(x):
    return canon(x * R260 % PQ, FQ_OFF)


def unmont(limbs):
    return val(limbs, FQ_OFF) * RINV260 % PQ


# ------------------------------------------------------------------------------------------------ family fq2
OPC = {n: i for i, n in enumerate(GEN.OPNAME)}
FQ2_DBL, FQ2_IS_ZERO, FQ2_EQ = 32, 33, 34
DC.OUT_WORDS["fq2"] = 37
DC.PRIME["fq2"] = PQ
assert pow(PQ - 1, (PQ - 1) // 2, PQ) == PQ - 1             # -1 is no square in Fq: a0^2 + a1^2 = 0 only at a = 0, the one element f_inv cannot invert


def _f2_inv(a):
    """f_inv returns 0 for 0 (its Fermat ladder on a zero norm); no other element has a zero norm"""
    return (0, 0) if a == (0, 0) else BN.f2_inv(a)


def _bound(vs):
    return {"out_l": [max(v.l[i] for v in vs) for i in range(10)], "out_v": max(v.val for v in vs) * PQ // 1000}


def _zero_forms(cls):
    return [r for k in (0, 1, 2) for r in DC._reps(k * PQ, cls)]


def _fq2_extras():
    rnd = random.Random(2024)
    top, z = SAFE.largest(), canon(0, FQ_OFF)
    ex = {"mul": [], "inv": [], "sub": [(z, z, top, top)], "eq": [], "zero": []}
    for _ in range(6):
        a = (rnd.randrange(PQ), rnd.randrange(PQ))
        ai = BN.f2_inv(a)
        for lvl in (0, 1, 2):
            A = [_rep(c, R260, SAFE_B, FQ_OFF, lvl, rnd) for c in a]
            for t in (ai, BN.f2_neg(ai), (a[0], -a[1] % PQ)):                  # products equal to 1, to -1, and a conj(a), which lies in Fq
                T = [_rep(c, R260, SAFE_B, FQ_OFF, (lvl + 1) % 3, rnd) for c in t]
                ex["mul"] += [(A[0], A[1], T[0], T[1]), (T[0], T[1], A[0], A[1])]
            ex["eq"] += [(A[0], A[1], _rep(a[0], R260, SAFE_B, FQ_OFF, k, rnd), _rep(a[1], R260, SAFE_B, FQ_OFF, 2 - k, rnd)) for k in (0, 1, 2)]
            ex["eq"].append((A[0], A[1], A[0], _rep((a[1] + 1) % PQ, R260, SAFE_B, FQ_OFF, lvl, rnd)))
            ex["inv"] += [(A[0], z), (z, A[1]), (A[0], canon(PQ, FQ_OFF)), (canon(2 * PQ, FQ_OFF), A[1])]
    zf = _zero_forms(SAFE)
    ex["mul"] += [(z, z, top, top), (top, top, z, z), (z, z, z, z)] + [(a, b, top, top) for a in zf[:6] for b in zf[:6]]
    ex["inv"] += [(a, b) for a in zf for b in zf]                              # zero in every form: the header returns zero
    ex["zero"] = [(a, b) for a in zf for b in zf] + [(a, canon(1, FQ_OFF)) for a in zf] + [(canon(3 * PQ - 1, FQ_OFF), a) for a in zf]
    one = [r for k in (0, 1, 2) for r in DC._reps(R260 % PQ + k * PQ, SAFE)]    # the field's one as 1, p + 1, 2p + 1 (Montgomery form)
    ex["eq"] += [(a, zf[i % len(zf)], b, zf[(i * 7 + j) % len(zf)]) for i, a in enumerate(one) for j, b in enumerate(one)]
    ex["eq"] += [(a, b, z, z) for a in zf[:8] for b in zf[:8]]
    return ex


def _fq2_ops():
    c, two = FQB.FQ2_CLASS, (FQB.FQ2_CLASS, FQB.FQ2_CLASS)
    A, AB = [[SAFE, SAFE]], [[SAFE, SAFE], [SAFE, SAFE]]
    ex = _fq2_extras()
    t3 = lambda s: lambda a, b: tuple((3 * x + s * 2 * y) % PQ for x, y in zip(a, b))  # noqa: E731
    ops = [
        Op("fq2", "MUL", OPC["MUL"], AB, BN.f2_mul, extra=ex["mul"], **_bound(FQB.f_mul(two, two))),
        Op("fq2", "SQ", OPC["SQ"], A, BN.f2_sq, **_bound(FQB.f_sq(two))),
        Op("fq2", "ADD", OPC["ADD"], AB, BN.f2_add, **_bound(FQB.f_add2(two, two))),
        Op("fq2", "SUB", OPC["SUB"], AB, BN.f2_sub, extra=ex["sub"], **_bound(FQB.f_sub2(two, two))),
        Op("fq2", "MULXI", OPC["MULXI"], A, lambda a: BN.f2_mul(a, (9, 1)), **_bound(FQB.fq2_mul_xi(two))),
        Op("fq2", "CONJ", OPC["CONJ"], A, lambda a: (a[0], -a[1] % PQ), **_bound([c, FQB.f_neg2(two)[1]])),
        Op("fq2", "MUL0", OPC["MUL0"], AB, lambda a, b: BN.f2_scalar(a, b[0]), extra=ex["mul"], **_bound(FQB.fq2_mul_fq(two, c))),
        Op("fq2", "MUL1", OPC["MUL1"], AB, lambda a, b: BN.f2_scalar(a, b[1]), extra=ex["mul"], **_bound(FQB.fq2_mul_fq(two, c))),
        Op("fq2", "INV", OPC["INV"], A, _f2_inv, extra=ex["inv"], **_bound(FQB.f_inv(two))),
        Op("fq2", "NEG", OPC["NEG"], A, BN.f2_neg, **_bound(FQB.f_neg2(two))),
        Op("fq2", "T3M", OPC["T3M"], AB, t3(-1), extra=ex["sub"], **_bound([FQB.fq_t3(c, c, True)])),
        Op("fq2", "T3P", OPC["T3P"], AB, t3(+1), extra=ex["sub"], **_bound([FQB.fq_t3(c, c, False)])),
        Op("fq2", "MOV", OPC["MOV"], A, lambda a: a, **_bound([c])),
        Op("fq2", "f_dbl", FQ2_DBL, A, lambda a: BN.f2_add(a, a), **_bound(FQB.f_dbl2(two))),
        Op("fq2", "f_is_zero", FQ2_IS_ZERO, A, lambda a: a == (0, 0), kind="flag", extra=ex["zero"]),
        Op("fq2", "fq2_eq", FQ2_EQ, AB, lambda a, b: a == b, kind="flag", extra=ex["eq"]),
    ]
    for op in ops:
        assert op.kind == "flag" or (op.out_v <= c.val * PQ // 1000 and op.out_l[:9] == c.l[:9] and op.out_l[9] <= c.l[9]), op.id      # the proof closes over the class: results are operands again
    return ops


FQ2_OPS = _fq2_ops()


def check_fq2(op, cases, out):
    for c, o in zip(cases, out):
        v = [x * RINV260 % PQ for x in values(op, c)]
        ref = op.ref(*[tuple(v[i:i + 2]) for i in range(0, len(v), 2)])
        raw = [[int(x) for x in o[:10]], [int(x) for x in o[10:20]]]
        words, flag = (val(o[20:28], W8_OFF), val(o[28:36], W8_OFF)), int(o[36])
        if op.kind == "flag":                               # the predicate; the operand itself comes back
            assert flag == int(ref) and raw == [list(c[0]), list(c[1])] and words == tuple(v[:2]), (op.id, c, flag)
            continue
        assert flag == 0 and tuple(unmont(r) for r in raw) == ref, (op.id, "value", c, raw)
        assert words == ref, (op.id, "canonical words", c, words)
        for r in raw:
            assert all(x <= m for x, m in zip(r, op.out_l)) and val(r, FQ_OFF) <= op.out_v, (op.id, "a component leaves its class", c, r)


DC.CHECK["fq2"] = check_fq2

# ------------------------------------------------------------------------------------------------ tower <-> the oracle's polynomial basis
# A tower element is six Fq2 values in tower order (c0.a0, c0.a1, c0.a2, c1.a0, c1.a1, c1.a2); GEN.coeffs puts them in the order of the powers of
# w, and u = w^6 - 9 turns the coefficient k0 + k1 u of w^i into k0 - 9 k1 at w^i and k1 at w^(i + 6).


def to_poly(t):
    k = GEN.coeffs((tuple(t[0:3]), tuple(t[3:6])))
    return [(c[0] - 9 * c[1]) % PQ for c in k] + [c[1] for c in k]


def from_poly(c):
    a = GEN.from_coeffs([((c[i] + 9 * c[i + 6]) % PQ, c[i + 6]) for i in range(6)])
    return list(a[0]) + list(a[1])


ONE_T = [(1, 0)] + [(0, 0)] * 5
assert to_poly(ONE_T) == BN.F12_ONE and from_poly(to_poly([(i, 2 * i + 1) for i in range(6)])) == [(i, 2 * i + 1) for i in range(6)]
M_CHAIN = 2 * X * (6 * X * X + 3 * X + 1)                    # the x-chain's exponent factor (bn254_pairing.h, which tools/gen_fq2vm.py follows) on GEN.X
assert math.gcd(M_CHAIN, BN.R) == 1

_FROB = {}


def frob(x, j):
    """x^(p^j) = f12_pow(x, P**j): the map is Fq-linear, so the power is taken of the twelve basis elements once and x's coefficients applied"""
    if j not in _FROB:
        _FROB[j] = [BN.f12_pow(BN.f12([0] * i + [1]), PQ ** j) for i in range(12)]
    acc = [0] * 12
    for c, b in zip(x, _FROB[j]):
        if c:
            acc = [(s + c * t) % PQ for s, t in zip(acc, b)]
    return acc


_FE = {}


def final_exp(x):
    key = tuple(x)
    if key not in _FE:
        _FE[key] = BN.final_exponentiate(list(x))
    return _FE[key]


# ------------------------------------------------------------------------------------------------ family fq12
F12_NAMES = ["fq6_mul", "fq6_inv", "fq12_mul", "fq12_sq", "fq12_mul_line", "fq12_inv", "fq12_conj", "fq12_frob_p2", "fq12_frob_p1", "fq12_frob_p3", "fq12_cyclo_sq",
             "fq12_pow_x", "fq12_is_one", "line_double", "line_add", "miller_loop", "final_exponentiation", "final_exponentiation_chain"]
F12_OUT = 217
N_ARITH, N_LONG = 64 + 6, 6                                # a second workgroup with a tail; the long ops cost a second of bigints apiece
T1 = 6 * X * X                                             # the plain ate loop count t - 1 of bn254_pairing.h's miller_loop


def limbs_of(fq2s, lvl, rnd):
    """Fq2 values -> raw limbs, every Fq component at one of the three _rep levels (canonical, the largest multiple of p the class admits, seeded)"""
    out = []
    for a in fq2s:
        for c in a:
            out += _rep(c, R260, SAFE_B, FQ_OFF, lvl if lvl < 3 else rnd.randrange(3), rnd)
    return out


class F12Op:
    fam = "fq12"
    out_words = F12_OUT

    def __init__(self, name):
        self.name, self.opid = name, F12_NAMES.index(name)

    @property
    def id(self):
        return "fq12." + self.name

    def pack(self, cases):
        a = np.array([c[0] for c in cases], dtype=np.uint32)
        b = np.array([c[1] for c in cases], dtype=np.uint32) if cases[0][1] is not None else None
        return [a, b, None]

    def build_cases(self):
        return f12_cases(self)


def _rand12(rnd):
    return [(rnd.randrange(PQ), rnd.randrange(PQ)) for _ in range(6)]


_CYC = []


def cyclotomic(i):
    """elements of the cyclotomic subgroup: final_exponentiate of seeded elements -- one bigint power g = final_exponentiate(s), then
    g^k = final_exponentiate(s^k) for seeded k"""
    if not _CYC:
        rnd = random.Random(77)
        g = final_exp(to_poly(_rand12(rnd)))
        _CYC.extend([BN.f12_pow(g, rnd.randrange(1, 1 << 64)) for _ in range(N_ARITH)])
    return from_poly(_CYC[i])


def _g2_jac(pt, rnd):
    z = (rnd.randrange(1, PQ), rnd.randrange(1, PQ))
    zz = BN.f2_sq(z)
    return [BN.f2_mul(pt[0], zz), BN.f2_mul(pt[1], BN.f2_mul(zz, z)), z]


_REFMILLER = {}


def ref_ate(q, p):
    """textbook Miller loop of the plain ate pairing, f_{t-1,Q}(P) with t - 1 = 6x^2: affine doubling and addition on the twist"""
    tq, tp = BN.twist(q), BN.cast_g1(p)
    r, f = tq, BN.F12_ONE
    for i in range(T1.bit_length() - 2, -1, -1):
        f = BN.f12_mul(BN.f12_mul(f, f), BN.linefunc(r, r, tp))
        r = BN.G12C.double(r)
        if (T1 >> i) & 1:
            f = BN.f12_mul(f, BN.linefunc(r, tq, tp))
            r = BN.G12C.add_pts(r, tq)
    return f


def ate_of_generators():
    if "e" not in _REFMILLER:
        _REFMILLER["e"] = final_exp(ref_ate(BN.G2, BN.G1))
    return _REFMILLER["e"]


def f12_cases(op):
    """(a limbs, b limbs or None, expected): expected is a polynomial-basis element, a flag, or three Fq2 line coefficients"""
    rnd = random.Random(5000 + op.opid)
    name, cases = op.name, []
    n = N_LONG if name in ("fq12_pow_x", "miller_loop", "final_exponentiation", "final_exponentiation_chain") else N_ARITH
    conj = lambda x: [c if i % 2 == 0 else -c % PQ for i, c in enumerate(x)]  # noqa: E731  (w -> -w)
    for i in range(n):
        lvl = i % 4                                         # 0, 1, 2: every component at that level; 3: a seeded level per component
        x, y = _rand12(rnd), _rand12(rnd)
        if name in ("fq6_mul", "fq6_inv"):
            x, y = x[:3], y[:3]
        z6 = [(0, 0)] * (6 - len(x))
        if i == 4 and name != "fq12_is_one":
            x = ONE_T[:len(x)]
        if i == 5 and name not in ("fq6_inv", "fq12_inv", "final_exponentiation", "final_exponentiation_chain"):
            x = [(0, 0)] * len(x)
        if i == 6:
            x = [x[0]] + [(0, 0)] * (len(x) - 1)            # an element of Fq2
        if i == 7 and len(x) == 6:
            x = [x[0], (0, 0), (0, 0), x[3], x[4], (0, 0)]   # line-shaped: A + (B + C v) w
        if i == 8 and name in ("fq6_mul", "fq12_mul"):
            y = from_poly(BN.f12_inv(to_poly(x + z6)))[:len(x)]         # x against x^-1
        px, py = to_poly(x + z6), to_poly(y + z6)
        if name in ("fq6_mul", "fq12_mul"):
            cases.append((limbs_of(x, lvl, rnd), limbs_of(y, (lvl + 1) % 4, rnd), BN.f12_mul(px, py)))
        elif name in ("fq6_inv", "fq12_inv"):
            cases.append((limbs_of(x, lvl, rnd), None, BN.f12_inv(px)))
        elif name == "fq12_sq":
            cases.append((limbs_of(x, lvl, rnd), None, BN.f12_mul(px, px)))
        elif name == "fq12_mul_line":
            l = [y[0], y[3], y[4]]
            cases.append((limbs_of(x, lvl, rnd), limbs_of(l, (lvl + 2) % 4, rnd), BN.f12_mul(px, to_poly([l[0], (0, 0), (0, 0), l[1], l[2], (0, 0)]))))
        elif name == "fq12_conj":
            if i == 9:
                assert conj(px) == BN.f12_pow(px, PQ ** 6)
            cases.append((limbs_of(x, lvl, rnd), None, conj(px)))
        elif name.startswith("fq12_frob_p"):
            j = int(name[-1])
            if i == 9:
                assert frob(px, j) == BN.f12_pow(px, PQ ** j)
            cases.append((limbs_of(x, lvl, rnd), None, frob(px, j)))
        elif name == "fq12_cyclo_sq":
            g = cyclotomic(i)
            cases.append((limbs_of(g, lvl, rnd), None, BN.f12_mul(to_poly(g), to_poly(g))))
        elif name == "fq12_pow_x":
            g = cyclotomic(i)
            cases.append((limbs_of(g, lvl, rnd), None, BN.f12_pow(to_poly(g), X)))
        elif name == "fq12_is_one":
            e = [ONE_T, x, [(1, 0), (0, 0), (0, 0), (0, 0), (0, 0), (0, 1)], [(1, 1)] + [(0, 0)] * 5, [(2, 0)] + [(0, 0)] * 5, [(0, 0)] * 6][i % 6 if i < 64 else 0]
            cases.append((limbs_of(e, lvl, rnd), None, e == ONE_T))
        elif name in ("line_double", "line_add"):
            t, q = BN.G2C.mul_pt(BN.G2, rnd.randrange(1, BN.R)), BN.G2C.mul_pt(BN.G2, rnd.randrange(1, BN.R))
            p = BN.G1C.mul_pt(BN.G1, rnd.randrange(1, BN.R))
            (Xj, Yj, Zj), f = _g2_jac(t, rnd), BN
            zz = f.f2_sq(Zj); zzz = f.f2_mul(zz, Zj)
            if name == "line_double":                      # 2 Y Z^3 yp, -3 X^2 Z^2 xp, 3 X^3 - 2 Y^2
                x2 = f.f2_sq(Xj)
                want = [f.f2_scalar(f.f2_mul(Yj, zzz), 2 * p[1]), f.f2_scalar(f.f2_mul(x2, zz), -3 * p[0]),
                        f.f2_sub(f.f2_scalar(f.f2_mul(x2, Xj), 3), f.f2_scalar(f.f2_sq(Yj), 2))]
                b = limbs_of([p], (lvl + 1) % 4, rnd)
            else:                                           # D yp, -N xp, N x2 - D y2 with N = y2 Z^3 - Y, D = (x2 Z^2 - X) Z
                N, D = f.f2_sub(f.f2_mul(q[1], zzz), Yj), f.f2_mul(f.f2_sub(f.f2_mul(q[0], zz), Xj), Zj)
                want = [f.f2_scalar(D, p[1]), f.f2_scalar(N, -p[0]), f.f2_sub(f.f2_mul(N, q[0]), f.f2_mul(D, q[1]))]
                b = limbs_of([q[0], q[1], p], (lvl + 1) % 4, rnd)
            cases.append((limbs_of([Xj, Yj, Zj], lvl, rnd), b, want))
        elif name == "miller_loop":                         # bilinearity: one bigint pairing serves every case
            ka, kb = rnd.randrange(1, BN.R), rnd.randrange(1, BN.R)
            q, p = BN.G2C.mul_pt(BN.G2, kb), BN.G1C.mul_pt(BN.G1, ka)
            cases.append((limbs_of([q[0], q[1]], lvl, rnd), limbs_of([p], (lvl + 1) % 4, rnd), ka * kb % BN.R))
        elif name == "final_exponentiation":
            cases.append((limbs_of(x, lvl, rnd), None, final_exp(px)))
        else:
            cases.append((limbs_of(x, lvl, rnd), None, BN.f12_pow(final_exp(px), M_CHAIN)))
    return cases


def f12_parse(o):
    """a result row: six Fq2 values from the raw limbs, the same from the canonical words, the flag, and the raw components"""
    raw = [[int(x) for x in o[10 * k:10 * k + 10]] for k in range(12)]
    t = [(unmont(raw[2 * k]), unmont(raw[2 * k + 1])) for k in range(6)]
    w = [(val(o[120 + 16 * k:128 + 16 * k], W8_OFF), val(o[128 + 16 * k:136 + 16 * k], W8_OFF)) for k in range(6)]
    return t, w, int(o[216]), raw


def check_fq12(op, cases, out):
    for i, (case, o) in enumerate(zip(cases, out)):
        t, w, flag, raw = f12_parse(o)
        want = case[2]
        assert t == w, (op.id, i, "the canonical words differ from the raw limbs' value")
        for k, r in enumerate(raw):
            assert SAFE.admits(r), (op.id, i, "component %d leaves its class" % k, r)
        if op.name == "fq12_is_one":
            assert flag == int(want), (op.id, i, flag)
        elif op.name in ("line_double", "line_add"):
            assert flag == 0 and t[:3] == want and t[3:] == [(0, 0)] * 3, (op.id, i, t[:3], want)
        elif op.name == "miller_loop":                      # after the bigint final exponentiation, where subfield scale factors vanish
            assert final_exp(to_poly(t)) == BN.f12_pow(ate_of_generators(), want), (op.id, i)
        else:
            assert flag == 0 and to_poly(t) == want, (op.id, i, to_poly(t), want)


F12_OPS = [F12Op(n) for n in F12_NAMES]
DC.CHECK["fq12"] = check_fq12
PAIRING_OPS = FQ2_OPS + F12_OPS
cases_of = DC.cases_of
run = DC.run

# ------------------------------------------------------------------------------------------------ the Fq2 machine, chain by chain
CHAINS = {"miller_a": 0, "subgroup": 1, "finish": 2, "miller_b": 3, "lines": 4}
VM_SIZES = (1, 32, 33, 70)                                  # a lone envelope, a full workgroup, a tail of one, three workgroups with a tail of six
SLOT_P2 = GEN.PAIR_SLOTS + GEN.SLOT_P


def vm_geom(lib, chain):
    g = (ctypes.c_uint32 * 4)()
    assert lib.devtier_fq2vm_geom(CHAINS[chain], g) == 0
    return {"slots": g[0], "kwords": g[1], "regs": g[2], "len": g[3]}


def vm_buffer(lib, chain, n, slots, seed):
    """io[slot][20][n]: the given slots (slot -> n Fq2 values) as Montgomery limbs, every other word seeded noise -- a slot the chain does not
    write must come back as it went in"""
    g = vm_geom(lib, chain)
    io = np.random.default_rng(seed).integers(0, 1 << 32, (g["slots"], 20, n), dtype=np.uint32)
    for s, vs in slots.items():
        for i, v in enumerate(vs):
            io[s, :, i] = mont(v[0]) + mont(v[1])
    return io


def vm_run(lib, chain, io, kconst, on_device):
    out = np.ascontiguousarray(io.copy())
    k = None if kconst is None else np.ascontiguousarray(kconst, dtype=np.uint32)
    assert k is None or k.size == vm_geom(lib, chain)["kwords"]
    rc = lib.devtier_fq2vm(CHAINS[chain], ctypes.c_uint32(io.shape[2]), out.ctypes.data_as(ctypes.c_void_p), None if k is None else k.ctypes.data_as(ctypes.c_void_p), ctypes.c_int(on_device))
    assert rc != -7, "chain %s: a word of the guard pattern around the slot buffer was written" % chain
    assert rc == 0, "devtier_fq2vm(%s) returned %d" % (chain, rc)
    return out


def vm_diff(chain, host, dev):
    """the first word that differs, as (chain, envelope, slot, word)"""
    d = np.argwhere(host != dev)
    if d.size == 0:
        return None
    s, w, i = (int(x) for x in d[0])
    return "%d words differ, first: chain %s, envelope %d, slot %d, word %d: host %#x device %#x" % (len(d), chain, i, s, w, int(host[s, w, i]), int(dev[s, w, i]))


def slot_fq2(io, slot, i):
    return (unmont(io[slot, :10, i]), unmont(io[slot, 10:, i]))


def slot_f12(io, slot0, i):
    """six consecutive slots = the coefficients of w^0 .. w^5 -> the oracle's polynomial basis"""
    a = GEN.from_coeffs([slot_fq2(io, slot0 + k, i) for k in range(6)])
    return to_poly(list(a[0]) + list(a[1]))


def f12_slots(x):
    """the inverse: a polynomial-basis element as the six Fq2 values of w^0 .. w^5"""
    t = from_poly(x)
    return GEN.coeffs((tuple(t[0:3]), tuple(t[3:6])))


def probe_indices(n):
    return sorted({i for i in (0, 31, 32, n - 1) if i < n})


_E = {}


def e_generators():
    """e(G1, G2) of the oracle's optimal ate pairing, the one the machine's chains compute"""
    if "e" not in _E:
        _E["e"] = BN.pairing(BN.G2, BN.G1)
    return _E["e"]


class Scenario:
    """One seeded set of 70 envelopes and a key (alpha, beta, gamma, delta as multiples of the generators) whose pairing product is one except where
    `bad` says otherwise: e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) with A = a G1, B = b G2, L = l G1, C = c G1."""

    def __init__(self, n=70, seed=9):
        rnd = random.Random(seed)
        R = BN.R
        self.n, self.rnd = n, rnd
        self.al, self.be, self.ga, self.de = (rnd.randrange(1, R) for _ in range(4))
        self.a, self.b, self.l = ([rnd.randrange(1, R) for _ in range(n)] for _ in range(3))
        self.c = [(x * y - self.al * self.be - z * self.ga) * pow(self.de, -1, R) % R for x, y, z in zip(self.a, self.b, self.l)]
        self.bad = {3, 32, n - 1}                              # envelopes whose product is not one: C is another point
        for i in self.bad:
            self.c[i] = (self.c[i] + 1 + i) % R
        g1, g2 = (lambda k: BN.G1C.mul_pt(BN.G1, k)), (lambda k: BN.G2C.mul_pt(BN.G2, k))
        self.A, self.B = [g1(k) for k in self.a], [g2(k) for k in self.b]
        self.gamma, self.delta, self.beta, self.nalpha = g2(self.ga), g2(self.de), g2(self.be), BN.G1C.neg_pt(g1(self.al))
        self.nC = [BN.G1C.neg_pt(g1(k)) for k in self.c]
        self.Lj = []                                        # L Jacobian with a seeded Z, as the public-input kernel leaves it
        for k in self.l:
            x, y = g1(k)
            z = rnd.randrange(2, PQ)
            self.Lj.append((x * z * z % PQ, y * z * z * z % PQ, z))

    def miller_a_slots(self, n):
        return {GEN.SLOT_QX: [q[0] for q in self.B[:n]], GEN.SLOT_QY: [q[1] for q in self.B[:n]], GEN.SLOT_P: self.A[:n]}

    def miller_b_slots(self, n):
        """g16_vm_pair1's encoding of (gamma, -L): P = (X Z, -Y), the Q.x slot carries (Z^3, 0); pair 2 is -C, affine"""
        return {GEN.SLOT_P: [(x * z % PQ, -y % PQ) for x, y, z in self.Lj[:n]], GEN.SLOT_QX: [(z * z * z % PQ, 0) for _, _, z in self.Lj[:n]],
                GEN.SLOT_QY: [(0, 0)] * n, SLOT_P2: self.nC[:n]}


def subgroup_points(n, seed=21):
    """k G2 for seeded k, and points of the twist outside the subgroup at 1, n // 2, n - 1 (and 32): a seeded x, y by the Fq2 square root, and
    [r] Q != O by bigints"""
    rnd = random.Random(seed)
    outside = {i for i in (1, n // 2, n - 1, 32) if 0 <= i < n}
    pts = []
    for i in range(n):
        if i not in outside:
            pts.append(BN.G2C.mul_pt(BN.G2, rnd.randrange(1, BN.R)))
            continue
        while True:
            x = (rnd.randrange(PQ), rnd.randrange(PQ))
            y = GEN.f2sqrt(BN.f2_add(BN.f2_mul(BN.f2_sq(x), x), BN.B2))
            if y is not None and BN.G2C.mul_pt((x, y), BN.R, reduce=False) is not None:
                break
        assert BN.G2C.is_on_curve((x, y))
        pts.append((x, y))
    return pts, outside


def psi(q):
    return (BN.f2_mul((q[0][0], -q[0][1] % PQ), GEN.gamma(1, 2)), BN.f2_mul((q[1][0], -q[1][1] % PQ), GEN.gamma(1, 3)))


def lines_table(lib, gamma, delta, on_device=0):
    """chain L on gamma and on delta, joined as g16_vm_key_constants joins them: [step][gamma, delta][3 coefficients]; also the two raw buffers"""
    g = vm_geom(lib, "lines")
    io = vm_run(lib, "lines", vm_buffer(lib, "lines", 2, {GEN.SLOT_QX: [gamma[0], delta[0]], GEN.SLOT_QY: [gamma[1], delta[1]]}, 31), None, on_device)
    steps = GEN.N_LINE_SLOTS // 6
    assert g["slots"] == GEN.LINE_SLOT0 + GEN.N_LINE_SLOTS
    tab = np.zeros((steps, 2, 3, 20), dtype=np.uint32)
    for j in range(2):
        tab[:, j] = io[GEN.LINE_SLOT0:, :, j].reshape(steps, 6, 20)[:, :3]
    return tab, io


# ---- one run of each chain on a scenario's first n envelopes, and the bigint meaning of what it leaves (both legs use these)
F0, FB0 = GEN.SLOT_F0, GEN.PAIR_SLOTS + GEN.SLOT_F0
_HOST = {}


def _cached(key, make):
    if key not in _HOST:
        _HOST[key] = make()
    return _HOST[key]


def run_miller_a(lib, scn, n, on_device):
    return vm_run(lib, "miller_a", vm_buffer(lib, "miller_a", n, scn.miller_a_slots(n), 100 + n), None, on_device)


def check_miller_a(scn, io):
    """chain A leaves the Miller value of (B, A) = (b G2, a G1): after the bigint final exponentiation it is e(G1, G2)^(a b)"""
    for i in probe_indices(io.shape[2]):
        assert final_exp(slot_f12(io, F0, i)) == BN.f12_pow(e_generators(), scn.a[i] * scn.b[i] % BN.R), ("miller_a", "envelope", i)


def run_subgroup(lib, n, on_device):
    pts, outside = _cached(("sub", n), lambda: subgroup_points(n))
    io = vm_buffer(lib, "subgroup", n, {GEN.SLOT_QX: [q[0] for q in pts], GEN.SLOT_QY: [q[1] for q in pts]}, 200 + n)
    return vm_run(lib, "subgroup", io, None, on_device), pts, outside


def check_subgroup(io, pts, outside):
    """(Z != 0, both differences zero) is the bigint statement psi(Q) == [6x^2] Q, which holds exactly for the points of the subgroup"""
    n = io.shape[2]
    assert len(outside) >= min(n, 3) and (n <= 32 or max(outside) >= 32)
    for i, q in enumerate(pts):
        sz, sh, sr = (slot_fq2(io, s, i) for s in (GEN.SLOT_SZ, GEN.SLOT_SH, GEN.SLOT_SR))
        stmt = _cached(("psi", q), lambda: psi(q) == BN.G2C.mul_pt(q, T1, reduce=False))
        assert (sz != (0, 0) and sh == (0, 0) and sr == (0, 0)) == stmt and stmt == (i not in outside), ("subgroup", "envelope", i, stmt)


def run_lines(lib, pts, on_device):
    n = len(pts)
    return vm_run(lib, "lines", vm_buffer(lib, "lines", n, {GEN.SLOT_QX: [q[0] for q in pts], GEN.SLOT_QY: [q[1] for q in pts]}, 300 + n), None, on_device)


def run_miller_b(lib, scn, tab, n, on_device):
    return vm_run(lib, "miller_b", vm_buffer(lib, "miller_b", n, scn.miller_b_slots(n), 400 + n), np.ascontiguousarray(tab).reshape(-1), on_device)


def check_miller_b(scn, io):
    """chain B on the line table of (gamma, delta) leaves the product of the Miller values of (gamma, -L) and (delta, -C)"""
    for i in probe_indices(io.shape[2]):
        want = BN.f12_pow(e_generators(), (-scn.l[i] * scn.ga - scn.c[i] * scn.de) % BN.R)
        assert final_exp(slot_f12(io, F0, i)) == want, ("miller_b", "envelope", i)


def finish_inputs(lib, scn, n):
    """the finish chain's buffer from the HOST interpreter's chain A and chain B values, and the key constant (chain A on (beta, -alpha))"""
    def make():
        a = run_miller_a(lib, scn, n, 0)
        tab = _cached(("tab", id(scn)), lambda: lines_table(lib, scn.gamma, scn.delta)[0])
        b = run_miller_b(lib, scn, tab, n, 0)
        k = vm_run(lib, "miller_a", vm_buffer(lib, "miller_a", 1, {GEN.SLOT_QX: [scn.beta[0]], GEN.SLOT_QY: [scn.beta[1]], GEN.SLOT_P: [scn.nalpha]}, 7), None, 0)
        io = vm_buffer(lib, "finish", n, {}, 500 + n)
        io[F0:F0 + 6] = a[F0:F0 + 6]
        io[FB0:FB0 + 6] = b[F0:F0 + 6]
        return io, np.ascontiguousarray(k[F0:F0 + 6, :, 0]).reshape(-1)
    return _cached(("fin", id(scn), n), make)


def run_finish(lib, scn, n, on_device):
    io, k = finish_inputs(lib, scn, n)
    return vm_run(lib, "finish", io, k, on_device), io, k


def check_finish(scn, out, inp, k):
    """the six result slots are map^-1 of final_exponentiate(chain A's value x chain B's x the key's) raised to the x-chain's factor m, which is
    prime to r: exactly one where e(A, B) e(-alpha, beta) e(-L, gamma) e(-C, delta) = 1, and not one for the envelopes built otherwise"""
    n = out.shape[2]
    k12 = slot_f12(k.reshape(6, 20, 1), 0, 0)
    probes = sorted(set(probe_indices(n)) | {i for i in scn.bad if i < n})
    assert n <= 3 or (any(i in scn.bad for i in probes) and any(i not in scn.bad for i in probes))
    for i in probes:
        prod = BN.f12_mul(BN.f12_mul(slot_f12(inp, F0, i), slot_f12(inp, FB0, i)), k12)
        want = BN.f12_pow(final_exp(prod), M_CHAIN)
        res = [slot_fq2(out, GEN.SLOT_RES + s, i) for s in range(6)]
        assert res == list(f12_slots(want)), ("finish", "envelope", i)
        assert (res == [(1, 0)] + [(0, 0)] * 5) == (i not in scn.bad), ("finish", "envelope", i, "valid" if i not in scn.bad else "invalid")
