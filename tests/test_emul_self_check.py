"""The batch self-check's per-lane steps on the host (no GPU), compiled from the header the kernels use (batch_self_check.h): the lens
rows and the row <-> op map for a batch of all six kinds with an op refused by validation and an op that failed proving, the equality
commitment against the oracle's MiMC, the membership set comparison, and the scatter of the verdicts that leaves a compact prefix sum."""
import ctypes
import os

import numpy as np
import pytest

from oracle.py import groth16 as g

RANGE, EQ, THR, MEM, IMP, CON = 1, 2, 3, 4, 5, 6
LEN_DYN = 0xFFFFFFFF
RANGE_BYTES, EQ_BYTES, THR_BYTES, IMP_MAX = 1478, 298, 762, 3527


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_self_check.so"))
    L.emul_sc_no_row.restype = ctypes.c_uint32
    L.emul_sc_row_align.restype = ctypes.c_uint32
    L.emul_sc_equality_bound.argtypes = [ctypes.c_void_p, ctypes.c_uint64]
    L.emul_sc_membership_bound.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32]
    return L


def pad256(x):
    return (x + 255) & ~255


def mem_bytes(count):
    return 10 + 4 + 8 * count + 256 + 32


def con_bytes(k):
    return 10 + 4 + 32 * k + (4 + 672 + 32) * (k - 1) + 32


class Batch:
    """A shard's pack view and self-check geometry as stage_shard lays them out, built here from a list of
    (kind, has a row, status found by the host, envelope length or LEN_DYN)."""

    def __init__(self, L, ops, set_counts, con_counts):
        n = len(ops)
        rows = [0] * 7
        for kind, has_row, _, _ in ops:
            rows[kind] += 1 if has_row else 0
        stride = [0, RANGE_BYTES, EQ_BYTES, THR_BYTES, max([mem_bytes(c) for c in set_counts] or [0]), IMP_MAX, max([con_bytes(c) for c in con_counts] or [0])]
        base, off = [0] * 7, 0
        for kind in (RANGE, EQ, MEM, IMP, THR, CON):          # the arena's order
            base[kind] = off
            off += pad256(stride[kind] * rows[kind])
        self.arena_bytes = off
        align = L.emul_sc_row_align()
        row0, total = [0] * 7, 0
        for kind in range(7):
            row0[kind] = total
            total += (rows[kind] + align - 1) // align * align
        self.n, self.rows, self.stride, self.base, self.row0, self.total_rows = n, rows, stride, base, row0, total
        self.src = np.zeros(n, dtype=np.uint64)
        self.lenf = np.zeros(n, dtype=np.uint32)
        self.dix = np.zeros(n, dtype=np.uint32)
        self.dkind = np.zeros(n, dtype=np.uint8)
        self.stf = np.zeros(n, dtype=np.int32)
        self.variant = np.zeros(n, dtype=np.uint8)
        self.expect_row = [None] * n
        seen = [0] * 7
        for i, (kind, has_row, st, ln) in enumerate(ops):
            self.stf[i] = st
            if not has_row:
                continue
            r = seen[kind]
            seen[kind] += 1
            self.variant[i] = kind
            self.src[i] = base[kind] + stride[kind] * r
            self.lenf[i] = ln
            self.expect_row[i] = row0[kind] + r
            if kind == RANGE:
                self.dix[i], self.dkind[i] = r, 1
            if kind == IMP:
                self.dix[i], self.dkind[i] = rows[RANGE] + r, 2
        self.dyn_len = np.zeros(rows[RANGE] + rows[IMP], dtype=np.uint32)
        self.dyn_status = np.zeros(max(rows[RANGE], 1), dtype=np.int32)

    def arr(self, xs, dt):
        return np.array(xs, dtype=dt)

    def run_rows(self, L):
        row_len = np.full(self.total_rows, 0xDEAD, dtype=np.uint32)
        row_op = np.full(self.total_rows, 0xDEAD, dtype=np.uint32)
        op_row = np.full(self.n, 0xDEAD, dtype=np.uint32)
        L.emul_sc_rows(self.n, P(self.src), P(self.lenf), P(self.dix), P(self.dkind), P(self.stf), P(self.dyn_len), P(self.dyn_status), P(self.variant),
                       P(self.arr(self.base, np.uint64)), P(self.arr(self.stride, np.uint64)), P(self.arr(self.row0, np.uint32)), P(self.arr(self.rows, np.uint32)),
                       P(row_len), P(row_op), P(op_row))
        return row_len, row_op, op_row


def six_kinds(L):
    # op:        0 range | 1 equality | 2 threshold | 3 membership(1) | 4 improvement | 5 consistency(4) | 6 equality a != b: refused by validation, no row
    #            7 range that fails on the device | 8 membership(64) | 9 consistency(1) | 10 improvement | 11 threshold whose framing the host refused
    ops = [(RANGE, 1, 0, LEN_DYN), (EQ, 1, 0, EQ_BYTES), (THR, 1, 0, THR_BYTES), (MEM, 1, 0, mem_bytes(1)), (IMP, 1, 0, LEN_DYN), (CON, 1, 0, con_bytes(4)),
           (EQ, 0, 1, 0), (RANGE, 1, 0, LEN_DYN), (MEM, 1, 0, mem_bytes(64)), (CON, 1, 0, con_bytes(1)), (IMP, 1, 0, LEN_DYN), (THR, 1, 1, 0)]
    b = Batch(L, ops, [1, 64], [4, 1])
    b.dyn_len[:] = [RANGE_BYTES, 0, 3301, 3527]          # range rows 0, 1 | improvement rows 0, 1
    b.dyn_status[:] = [0, 1]                             # the second range op: refused on the device (k_build_range)
    return b


def test_rows_and_maps_for_all_six_kinds(lib):
    b = six_kinds(lib)
    row_len, row_op, op_row = b.run_rows(lib)
    no_row = lib.emul_sc_no_row()
    assert b.rows == [0, 2, 1, 2, 2, 2, 2]
    assert [b.row0[k] % lib.emul_sc_row_align() for k in range(7)] == [0] * 7 and len(set(b.row0[1:])) == 6
    want_len = {0: RANGE_BYTES, 1: EQ_BYTES, 2: THR_BYTES, 3: mem_bytes(1), 4: 3301, 5: con_bytes(4), 7: 0, 8: mem_bytes(64), 9: con_bytes(1), 10: 3527, 11: 0}
    for i in range(b.n):
        if b.expect_row[i] is None:
            assert op_row[i] == no_row
            continue
        g_ = b.expect_row[i]
        assert op_row[i] == g_ and row_op[g_] == i, i
        assert row_len[g_] == want_len[i], (i, row_len[g_])
    used = sorted(r for r in b.expect_row if r is not None)
    assert (np.delete(row_len, used) == 0xDEAD).all() and (np.delete(row_op, used) == 0xDEAD).all()          # the padding rows are nobody's


def equality_envelope(value):
    env = bytearray(EQ_BYTES)
    env[0:2] = b"\x02\x02"
    env[2:6] = (256).to_bytes(4, "little")
    env[6:10] = (32).to_bytes(4, "little")
    env[10:266] = bytes((7 * i + 1) & 0xFF for i in range(256))
    env[266:298] = g.commit_value_snark(value)
    return env


def membership_envelope(the_set):
    body = len(the_set).to_bytes(4, "little") + b"".join(int(x).to_bytes(8, "little") for x in the_set) + bytes(256)
    return bytearray(b"\x02\x04" + len(body).to_bytes(4, "little") + (32).to_bytes(4, "little") + body + bytes(32))


def as_buf(env):
    return (ctypes.c_uint8 * len(env)).from_buffer(env)


@pytest.mark.parametrize("value", [0, 1, 77, 2**32, 2**64 - 1])
def test_equality_commitment_is_the_oracles_mimc(lib, value):
    env = equality_envelope(value)
    assert lib.emul_sc_equality_bound(as_buf(env), value) == 1
    assert lib.emul_sc_equality_bound(as_buf(env), value ^ 1) == 0          # another staged value
    for at in (266, 280, 297):
        bad = bytearray(env)
        bad[at] ^= 1
        assert lib.emul_sc_equality_bound(as_buf(bad), value) == 0, at
    bad = bytearray(env)
    bad[100] ^= 1                                                            # a proof byte: the pairing check's business, not the binding's
    assert lib.emul_sc_equality_bound(as_buf(bad), value) == 1


@pytest.mark.parametrize("count", [1, 64])
def test_membership_set_comparison(lib, count):
    rng = np.random.default_rng(count)
    the_set = rng.integers(0, 2**64, count, dtype=np.uint64)
    staged = np.zeros(64, dtype=np.uint64)
    staged[:count] = the_set
    env = membership_envelope(the_set)
    assert len(env) == mem_bytes(count)
    assert lib.emul_sc_membership_bound(as_buf(env), P(staged), count) == 1
    for k in sorted({0, count // 2, count - 1}):                             # one element changed, in the envelope or in the staged set
        bad = bytearray(env)
        bad[14 + 8 * k + 3] ^= 0x10
        assert lib.emul_sc_membership_bound(as_buf(bad), P(staged), count) == 0, k
        other = staged.copy()
        other[k] ^= np.uint64(1)
        assert lib.emul_sc_membership_bound(as_buf(env), P(other), count) == 0, k
    for wrong in {count - 1, count + 1} - {-1}:                              # the count changed on either side
        assert lib.emul_sc_membership_bound(as_buf(env), P(staged), wrong) == 0
        bad = bytearray(env)
        bad[10:14] = wrong.to_bytes(4, "little")
        assert lib.emul_sc_membership_bound(as_buf(bad), P(staged), count) == 0
    if count > 1:                                                            # the staged order is what counts (stricter than upstream's multiset)
        swapped = staged.copy()
        swapped[[0, 1]] = swapped[[1, 0]]
        assert lib.emul_sc_membership_bound(as_buf(env), P(swapped), count) == 0
    assert lib.emul_sc_membership_bound(as_buf(env), P(staged), 65) == 0


def test_bind_ands_into_the_rows_verdicts(lib):
    b = six_kinds(lib)
    row_len, _, _ = b.run_rows(lib)
    arena = np.zeros(b.arena_bytes, dtype=np.uint8)
    sets = np.zeros((2, 64), dtype=np.uint64)
    sets[0, 0] = 9
    sets[1] = np.arange(100, 164)
    mem_len = np.array([1, 64], dtype=np.uint32)
    eq_value = np.array([77], dtype=np.uint64)
    envs = {b.base[EQ]: equality_envelope(77), b.base[MEM]: membership_envelope(sets[0, :1]), b.base[MEM] + b.stride[MEM]: membership_envelope(sets[1])}

    def run(verdicts, tamper=None):
        a = arena.copy()
        for at, env in envs.items():
            a[at:at + len(env)] = np.frombuffer(bytes(env), dtype=np.uint8)
        if tamper is not None:
            a[tamper] ^= 1
        ok = np.array(verdicts, dtype=np.uint8)
        lib.emul_sc_bind(P(a), P(b.arr(b.base, np.uint64)), P(b.arr(b.stride, np.uint64)), P(b.arr(b.row0, np.uint32)), P(b.arr(b.rows, np.uint32)), P(row_len), P(ok),
                         P(eq_value), P(sets), P(mem_len))
        return ok
    ones = np.ones(b.total_rows, dtype=np.uint8)
    assert (run(ones) == 1).all()
    e, m0, m1 = b.row0[EQ], b.row0[MEM], b.row0[MEM] + 1
    for at, row in ((b.base[EQ] + 270, e), (b.base[MEM] + 14, m0), (b.base[MEM] + b.stride[MEM] + 100, m1), (b.base[MEM] + b.stride[MEM] + 10, m1)):
        got = run(ones, tamper=at)
        assert got[row] == 0 and got.sum() == b.total_rows - 1, (at, row)
    refused = ones.copy()
    refused[m1] = 0                                                          # what the verifier refused stays refused, the others are untouched
    got = run(refused)
    assert got[m1] == 0 and got.sum() == b.total_rows - 1


def test_apply_leaves_a_compact_prefix_sum(lib):
    b = six_kinds(lib)
    row_len, row_op, op_row = b.run_rows(lib)
    # what k_batch_lens writes for this batch
    len0 = np.array([RANGE_BYTES, EQ_BYTES, THR_BYTES, mem_bytes(1), 3301, con_bytes(4), 0, 0, mem_bytes(64), con_bytes(1), 3527, 0], dtype=np.uint32)
    st0 = np.array([0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 1], dtype=np.int32)
    live = [i for i in range(b.n) if st0[i] == 0]

    def run(refuse):
        ok = np.ones(b.total_rows, dtype=np.uint8)
        for i in refuse:
            ok[op_row[i]] = 0
        ln, st = len0.copy(), st0.copy()
        off = np.zeros(b.n + 1, dtype=np.uint64)
        cnt = np.zeros(2, dtype=np.uint32)
        lib.emul_sc_apply(b.n, P(op_row), P(ok), P(ln), P(st), P(off), P(cnt))
        return ln, st, off, cnt.tolist()
    ln, st, off, cnt = run([])
    assert (ln == len0).all() and (st == st0).all() and cnt == [len(live), 0]
    for refuse in ([4], [0, 8], live, [7, 11]):          # (7 and 11 failed before: their rows' verdicts change nothing)
        ln, st, off, cnt = run(refuse)
        hit = [i for i in refuse if st0[i] == 0]
        for i in range(b.n):
            assert st[i] == (2 if i in hit else st0[i]) and ln[i] == (0 if i in hit else len0[i]), (refuse, i)
        assert cnt == [len(live), len(hit)]
        assert off[0] == 0 and (np.diff(off.astype(np.int64)) == ln).all()          # compact: op i's bytes end where op i + 1's begin


def test_flip_touches_one_bit(lib):
    b = six_kinds(lib)
    arena = np.zeros(b.arena_bytes, dtype=np.uint8)
    arena[:] = 0xA5
    lib.emul_sc_flip(P(arena), P(b.src), 8, 100)
    changed = np.nonzero(arena != 0xA5)[0].tolist()
    assert changed == [int(b.src[8]) + 100] and arena[changed[0]] == 0xA4
