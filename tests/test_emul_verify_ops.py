"""Envelopes against the caller's statements on the host (no GPU): libzkp_amd/csrc/vst_steps.h compiled from the header the kernels use
(tests/emul/emul_verify_ops.cpp), the membership step run as the 64 lanes of one wave.  Judged against a Python restatement of the
reference's seven verify_* functions (src/proof/*.rs) up to the backend call, on composite.parse_proof, with the commitment from
oracle/py/groth16.py: commit_value_snark.  Envelopes are synthetic: no valid proof is needed to judge classification and binding (the
verdict of an envelope's row is supplied by the test)."""
import ctypes
import os

import numpy as np
import pytest

from libzkp_amd import _native, composite
from oracle.py import groth16

U64, VP = ctypes.c_uint64, ctypes.c_void_p
ACCEPTED, ENVELOPE, STATEMENT, PROOF = 0, 1, 2, 3
R, E, T, M, I, C = 1, 2, 3, 4, 5, 6          # op kinds = scheme bytes
MAX = 2**64 - 1


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_verify_ops.so"))
    L.emul_vst_verify.argtypes = [U64, VP, VP, U64, VP, VP, VP, VP, VP, VP]
    L.emul_vst_verify.restype = U64
    L.emul_vst_slice.argtypes = [U64, VP, U64, VP, VP]
    L.emul_vst_slice.restype = None
    L.emul_vst_op_bytes.restype = ctypes.c_uint32
    assert L.emul_vst_op_bytes() == ctypes.sizeof(_native.Op) == 40
    return L


def P(a):
    return a.ctypes.data_as(VP)


def le(x, n=8):
    return int(x).to_bytes(n, "little")


def env(scheme, payload, commitment=None, version=2):
    commitment = bytes(range(scheme, scheme + 32)) if commitment is None else commitment
    return bytes([version, scheme]) + le(len(payload), 4) + le(len(commitment), 4) + payload + commitment


def env_range(mn, mx):
    return env(R, le(mn) + le(mx) + bytes(672))


def env_threshold(t):
    return env(T, le(t) + bytes(700))


def env_improvement(old, new=None):
    return env(I, le(old) + le(old + 1 if new is None else new) + bytes(100))


def env_equality(commitment):
    return env(E, bytes(256), commitment)


def env_membership(elements, count=None):
    return env(M, le(len(elements) if count is None else count, 4) + b"".join(le(x) for x in elements) + bytes(256))


def env_consistency():
    return env(C, le(1, 4) + bytes(32))


def op(kind, a=0, b=0, c=0, count=0, list_off=0):
    return (kind, count, a, b, c, list_off)


# ---- the restatement: which step of the reference's verify_<scheme>(proof, statement) says no before its backend is called
def ref_envelope(e, kind):
    """parse_and_validate_proof(proof, SCHEME_ID) and the length checks each verify_* makes before its backend (proof_helpers.rs)"""
    try:
        version, scheme, payload, commitment = composite.parse_proof(e)
    except composite.ProofFormatError:
        return None
    u = lambda b: int.from_bytes(b, "little")  # noqa: E731
    if version != composite.PROOF_VERSION or not 1 <= scheme <= 6:
        return None
    good = {R: len(payload) >= 20 and len(commitment) == 32 and u(payload[:8]) <= u(payload[8:16]),
            E: len(commitment) == 32,
            T: len(payload) >= 12 and len(commitment) == 32,
            M: len(commitment) == 32 and len(payload) >= 4 and 1 <= u(payload[:4]) <= 64 and len(payload) > 4 + 8 * u(payload[:4]),
            I: len(payload) >= 16 and len(commitment) == 32,
            C: True}[scheme]
    if not good:
        return None
    if 1 <= kind <= 6 and scheme != kind:
        return None
    return scheme, payload, commitment


def ref_why(o, e, lists):
    kind, count, a, b, c, list_off = o
    kind &= ~0x100
    parsed = ref_envelope(e, kind)
    if parsed is None:
        return ENVELOPE
    if not 1 <= kind <= 6:
        return STATEMENT
    scheme, payload, commitment = parsed
    u = lambda x: int.from_bytes(x, "little")  # noqa: E731
    inside = list_off <= len(lists) and count <= len(lists) - list_off
    if kind == R:          # range_proof.rs:27-48, verify_range_with_bounds
        good = b <= c and (u(payload[:8]), u(payload[8:16])) == (b, c)
    elif kind == T:        # threshold_proof.rs:32-44
        good = u(payload[:8]) == a
    elif kind == I:        # improvement_proof.rs:37-52
        good = u(payload[:8]) == a
    elif kind == E and count == 0:          # equality_proof.rs:50-57
        good = a == b and commitment == groth16.commit_value_snark(a)
    elif kind == E:        # equality_proof.rs:59-61, 34-45
        good = count == 4 and inside and commitment == b"".join(le(x) for x in lists[list_off:list_off + 4])
    elif kind == M:        # set_membership.rs:40-68
        n = u(payload[:4])
        emb = [u(payload[4 + 8 * k: 12 + 8 * k]) for k in range(n)]
        good = 1 <= count <= 64 and inside and count == n and sorted(emb) == sorted(lists[list_off:list_off + count])
    else:
        good = True
    return ACCEPTED if good else STATEMENT


def ops_array(ops):
    arr = (_native.Op * max(len(ops), 1))()
    for i, (kind, count, a, b, c, list_off) in enumerate(ops):
        arr[i].kind, arr[i].count, arr[i].a, arr[i].b, arr[i].c, arr[i].list_off = kind, count, a, b, c, list_off
    return arr


def run(L, ops, envs, lists, accept=None, lead=0, n_lists=None):
    """(ok, why) of the emulated call; asserts that no step read a list value outside [0, n_lists) or broadcast from an idle lane"""
    n = len(ops)
    blob = np.frombuffer(bytes(lead) + b"".join(envs) + b"\0", dtype=np.uint8)
    off = (lead + np.concatenate(([0], np.cumsum([len(e) for e in envs])))).astype(np.uint64)
    la = np.array(list(lists) + [0xDEAD], dtype=np.uint64)          # one value behind the lists, which nothing may read
    ok, why = np.full(n, 9, dtype=np.uint8), np.full(n, 9, dtype=np.uint8)
    acc = None if accept is None else np.asarray(accept, dtype=np.uint8)
    arr = ops_array(ops)
    outside = L.emul_vst_verify(n, ctypes.byref(arr), P(la), len(lists) if n_lists is None else n_lists, P(blob), P(off), None if acc is None else P(acc), P(ok), P(why), None)
    assert outside == 0
    return [int(x) for x in ok], [int(x) for x in why]


def check(L, ops, envs, lists, **kw):
    ok, why = run(L, ops, envs, lists, **kw)
    want = [ref_why(o, e, list(lists)) for o, e in zip(ops, envs)]
    assert why == want, (why, want)
    assert ok == [int(w == ACCEPTED) for w in want]
    return why


# ---- membership
@pytest.mark.parametrize("count", (1, 2, 63, 64))
def test_membership_counts_and_orders(lib, count):
    rng = np.random.default_rng(count)
    els = [int(x) for x in rng.integers(0, 2**64, count, dtype=np.uint64)]
    perm = [els[k] for k in rng.permutation(count)]
    wrong = list(perm); wrong[-1] ^= 1
    lists = els + perm + list(reversed(els)) + wrong
    ops = [op(M, count=count, list_off=k * count) for k in range(4)]
    assert check(lib, ops, [env_membership(els)] * 4, lists) == [ACCEPTED, ACCEPTED, ACCEPTED, STATEMENT]


def test_membership_multiplicities_zero_padding_and_high_bits(lib):
    cases = [([1, 1, 2], [1, 2, 2], STATEMENT),           # same distinct elements, other multiplicities
             ([1, 2, 2], [1, 1, 2], STATEMENT),
             ([1, 1, 2], [2, 1, 1], ACCEPTED),
             ([0, 1], [1, 0], ACCEPTED),                  # zero is an element
             ([1], [1, 0], STATEMENT),                    # the count; zero against what padding would look like
             ([1, 0], [1], STATEMENT),
             ([0], [0], ACCEPTED),
             ([0, 0], [0, 1], STATEMENT),
             ([1], [2**32 + 1], STATEMENT),               # differ only above bit 32
             ([2**32 + 1, 1], [1, 2**32 + 1], ACCEPTED),
             ([MAX], [MAX], ACCEPTED), ([MAX, 0], [0, MAX], ACCEPTED), ([MAX], [MAX - 1], STATEMENT), ([MAX], [2**63 - 1], STATEMENT),
             ([5] * 64, [5] * 64, ACCEPTED), ([5] * 63 + [6], [5] * 62 + [6, 6], STATEMENT), ([5] * 63 + [6], [6] + [5] * 63, ACCEPTED)]
    lists, ops, envs = [], [], []
    for emb, st, _ in cases:
        ops.append(op(M, a=7, count=len(st), list_off=len(lists))); lists += st; envs.append(env_membership(emb))
    assert check(lib, ops, envs, lists) == [w for _, _, w in cases]


def test_membership_statement_counts_0_and_65_are_no_statement(lib):
    lists = list(range(100, 170))
    envs = [env_membership([100]), env_membership(list(range(100, 164))), env_membership([100])]
    ops = [op(M, count=0), op(M, count=65), op(M, count=1)]
    assert check(lib, ops, envs, lists) == [STATEMENT, STATEMENT, ACCEPTED]


def test_list_spans_at_and_behind_the_end_of_the_lists(lib):
    lists = [3, 4, 5, 6]
    cm = b"".join(le(x) for x in lists)
    envs = [env_membership([5, 6]), env_membership([5, 6]), env_membership([5, 6]), env_equality(cm), env_equality(cm), env_membership([6])]
    ops = [op(M, count=2, list_off=2),          # ends exactly at n_lists
           op(M, count=2, list_off=3),          # one element behind it
           op(M, count=2, list_off=MAX),        # list_off + count wraps
           op(E, count=4, list_off=0), op(E, count=4, list_off=1), op(M, count=1, list_off=4)]
    assert check(lib, ops, envs, lists) == [ACCEPTED, STATEMENT, STATEMENT, ACCEPTED, STATEMENT, STATEMENT]
    # no lists at all: every list-bearing op is refused, and nothing is read
    ok, why = run(lib, ops, envs, [], n_lists=0)
    assert why == [STATEMENT] * 6 and ok == [0] * 6


@pytest.mark.parametrize("lead", range(8))
def test_every_envelope_start_offset_mod_8(lib, lead):
    els = [2**40 + 3, 9, 2**63, 0, 9]
    lists = [9, 0, 2**63, 9, 2**40 + 3] + [9, 0, 2**63, 9, 2**40 + 2]
    v = 123456789
    cm = groth16.commit_value_snark(v)
    envs = [env_membership(els), env_membership(els), env_equality(cm), env_range(3, 2**63 + 7), env_membership(els)]
    ops = [op(M, count=5), op(M, count=5, list_off=5), op(E, a=v, b=v), op(R, b=3, c=2**63 + 7), op(M, count=5)]
    assert check(lib, ops, envs, lists, lead=lead) == [ACCEPTED, STATEMENT, ACCEPTED, ACCEPTED, ACCEPTED]


# ---- equality
def test_equality_by_value(lib):
    ops, envs = [], []
    for v in (0, 1, MAX):
        cm = groth16.commit_value_snark(v)
        first, last = bytes([cm[0] ^ 1]) + cm[1:], cm[:-1] + bytes([cm[-1] ^ 0x80])
        for e, o in ((cm, op(E, a=v, b=v)), (cm, op(E, a=v, b=(v + 1) % 2**64)), (first, op(E, a=v, b=v)), (last, op(E, a=v, b=v)),
                     (groth16.commit_value_snark((v + 1) % 2**64), op(E, a=v, b=v))):
            envs.append(env_equality(e)); ops.append(o)
    assert check(lib, ops, envs, []) == [ACCEPTED, STATEMENT, STATEMENT, STATEMENT, STATEMENT] * 3


def test_equality_commitment_form(lib):
    cm = bytes(range(200, 232))
    words = [int.from_bytes(cm[8 * k: 8 * k + 8], "little") for k in range(4)]
    first, last = list(words), list(words)
    first[0] ^= 1; last[3] ^= 1 << 63
    lists = words + first + last
    envs = [env_equality(cm)] * 6
    ops = [op(E, a=1, b=2, count=4),                      # a, b are ignored in the commitment form
           op(E, count=4, list_off=4), op(E, count=4, list_off=8),
           op(E, count=3), op(E, count=5), op(E, count=1)]
    assert check(lib, ops, envs, lists) == [ACCEPTED, STATEMENT, STATEMENT, STATEMENT, STATEMENT, STATEMENT]


# ---- range, threshold, improvement, consistency
def test_range_threshold_improvement_consistency(lib):
    envs = [env_range(5, 9), env_range(5, 9), env_range(5, 9), env_range(5, 9), env_range(0, MAX), env_range(0, 2**63 - 1),
            env_threshold(50), env_threshold(50), env_threshold(50), env_improvement(30), env_improvement(30), env_improvement(30),
            env_consistency(), env_range(9, 5)]
    ops = [op(R, a=7, b=5, c=9), op(R, a=1234, b=5, c=9),          # the value is no part of the statement
           op(R, b=9, c=5),                                        # min > max
           op(R, b=5, c=10),
           op(R, b=0, c=MAX), op(R, b=0, c=MAX),                   # max differing in bit 63 only
           op(T, a=50, count=3, list_off=77), op(T, a=51), op(T, a=49),
           op(I, a=30, b=1), op(I, a=31), op(I, a=29),
           op(C, a=1, b=2, c=3, count=9, list_off=99),             # verify_consistency(proof) has no parameter
           op(R, b=9, c=5)]                                        # an envelope whose own bounds run backwards: a pre-check
    want = [ACCEPTED, ACCEPTED, STATEMENT, STATEMENT, ACCEPTED, STATEMENT, ACCEPTED, STATEMENT, STATEMENT, ACCEPTED, STATEMENT, STATEMENT, ACCEPTED, ENVELOPE]
    assert check(lib, ops, envs, []) == want


def test_kinds_schemes_and_the_order_of_the_steps(lib):
    cm = groth16.commit_value_snark(4)
    envs = [env_threshold(50), env_range(5, 9), env_range(5, 9), env_range(5, 9), env_range(5, 9),
            env_range(5, 9)[:-1], env(R, le(5) + le(9) + bytes(672), version=1), env_range(5, 9)[:-1], env_equality(cm), env(7, bytes(40)), b""]
    ops = [op(R, b=50, c=50),                      # the op's kind is not the scheme byte
           op(0, b=5, c=9), op(7, b=5, c=9),       # no kind at all
           op(R | 0x100, b=5, c=9),                # the self-check flag is ignored
           op(R | 0x200, b=5, c=9),
           op(R, b=5, c=10),                       # broken in framing AND a wrong statement: the envelope decides
           op(R, b=5, c=10),
           op(0),                                  # broken in framing and no kind: the envelope decides
           op(E | 0x100, a=4, b=4),
           op(7), op(R)]
    want = [ENVELOPE, STATEMENT, STATEMENT, ACCEPTED, STATEMENT, ENVELOPE, ENVELOPE, ENVELOPE, ACCEPTED, ENVELOPE, ENVELOPE]
    assert check(lib, ops, envs, []) == want


def test_refused_envelopes_get_no_row_and_refused_rows_say_proof(lib):
    envs = [env_range(5, 9), env_range(5, 9), env_threshold(50), env_threshold(50), env_membership([1, 2]), env_membership([1, 2])]
    ops = [op(R, b=5, c=9), op(R, b=5, c=8), op(T, a=50), op(T, a=50), op(M, count=2), op(M, count=2)]
    lists = [2, 1]
    L = lib
    n = len(ops)
    blob = np.frombuffer(b"".join(envs), dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(e) for e in envs]))).astype(np.uint64)
    ok, why, rec = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=[("scheme", "<u4"), ("len", "<u4"), ("p0", "<u8"), ("p1", "<u8"), ("jobs", "<u4"), ("why", "<u4")])
    accept = np.array([1, 1, 0, 1, 1, 0], dtype=np.uint8)
    arr, la = ops_array(ops), np.array(lists, dtype=np.uint64)
    assert L.emul_vst_verify(n, ctypes.byref(arr), P(la), 2, P(blob), P(off), P(accept), P(ok), P(why), P(rec)) == 0
    assert list(ok) == [1, 0, 0, 1, 1, 0] and list(why) == [ACCEPTED, STATEMENT, PROOF, ACCEPTED, ACCEPTED, PROOF]
    assert list(rec["scheme"]) == [R, 0, T, T, M, M] and list(rec["why"]) == [0, STATEMENT, 0, 0, 0, 0]          # the refused envelope reaches no verifier
    assert list(rec["len"]) == [len(e) for e in envs] and (rec["p0"][0], rec["p1"][0], rec["p0"][2]) == (5, 9, 50)


# ---- the slice function
def slice_ops(L, ops, n_lists):
    arr, out, span = ops_array(ops), ops_array(ops), np.zeros(2, dtype=np.uint64)
    L.emul_vst_slice(len(ops), ctypes.byref(arr), n_lists, ctypes.byref(out), P(span))
    return [(o.kind, o.count, o.a, o.b, o.c, o.list_off) for o in out[:len(ops)]], int(span[0]), int(span[1])


def test_slice_without_a_list_bearing_op_has_an_empty_span(lib):
    ops = [op(R, a=1, b=0, c=9), op(T, a=50, count=3, list_off=4), op(C, count=5, list_off=9), op(E, a=3, b=3), op(I, a=1, b=2),
           op(M, count=0, list_off=2), op(M, count=65, list_off=0), op(E, count=3, list_off=1), op(M, count=2, list_off=99)]
    out, lo, count = slice_ops(lib, ops, 100)
    assert (lo, count) == (0, 0)
    for o, s in zip(ops, out):
        assert s[:5] == o[:5] and s[5] == MAX


def test_slices_carry_the_span_their_ops_name_and_give_the_unsliced_verdicts(lib):
    rng = np.random.default_rng(7)
    lists, ops, envs = [], [], []
    sets = []
    for k in range(9):          # the sets first, so that the ops can name them out of order
        els = [int(x) for x in rng.integers(0, 50, int(rng.integers(1, 7)))]
        sets.append((len(lists), els)); lists += [int(x) for x in rng.permutation(els)]
    cm = bytes(rng.integers(0, 256, 32, dtype=np.uint8))
    cm_at = len(lists); lists += [int.from_bytes(cm[8 * k: 8 * k + 8], "little") for k in range(4)]
    for k in (5, 2, 8, 0):
        at, els = sets[k]
        ops.append(op(M, count=len(els), list_off=at)); envs.append(env_membership(els))
        ops.append(op(R, b=k, c=k + 1)); envs.append(env_range(k, k + 1))
    ops += [op(E, count=4, list_off=cm_at), op(M, count=2, list_off=len(lists) - 1), op(M, count=3, list_off=sets[3][0]), op(E, count=4, list_off=cm_at + 1)]
    envs += [env_equality(cm), env_membership([1, 2]), env_membership([77, 78, 79]), env_equality(cm)]
    whole = check(lib, ops, envs, lists)
    assert whole.count(ACCEPTED) == 9 and whole.count(STATEMENT) == 3
    for lo, hi in ((0, 4), (4, 8), (8, 12), (2, 7), (0, 12), (9, 10), (1, 2)):
        out, s_lo, s_count = slice_ops(lib, ops[lo:hi], len(lists))
        bearing = [o for o in ops[lo:hi] if (o[0] == M or (o[0] == E and o[1] == 4)) and o[5] + o[1] <= len(lists)]
        if bearing:
            assert s_lo == min(o[5] for o in bearing) and s_lo + s_count == max(o[5] + o[1] for o in bearing)
        else:
            assert (s_lo, s_count) == (0, 0)
        ok, why = run(lib, out, envs[lo:hi], lists[s_lo:s_lo + s_count])
        assert why == whole[lo:hi]
