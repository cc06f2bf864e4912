"""The staging plan of a mixed batch on the host (no GPU): plan_shards, plan_stage_layout and fill_stage_image of libzkp_amd/csrc/batch_plan.h,
compiled from the header the library uses (tests/emul/emul_batch_plan.cpp), against a model written here from include/libzkp_hip.h and the
header's comment block: rows and strides per variant, every offset of the three device blocks, every byte of the staging image, the framed
threshold / consistency images and their job lists."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from libzkp_amd import _native

RANGE, EQ, THR, MEM, IMP, CON = 1, 2, 3, 4, 5, 6
FLAG = 0x100
RANGE_BYTES, EQ_BYTES, THR_BYTES, IMP_MAX, RP = 1478, 298, 762, 3527, 672
MAX_SET, ROW_ALIGN, LEN_DYN, NO_ROW = 64, 64, 0xFFFFFFFF, 0xFFFFFFFF
DYN_NONE, DYN_LEN_STATUS, DYN_LEN_ONLY = 0, 1, 2
KIND_THRESHOLD, KIND_CONSISTENCY = 2, 3                     # the job kinds of the Bulletproofs pipeline
OP = np.dtype([("kind", "<u4"), ("count", "<u4"), ("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("list_off", "<u8")])
FILL = 0xA5                                                 # what the image holds before the fill: bytes nobody writes keep it
# the take order of the three blocks (the header's comment): name -> bytes per unit
IMAGE = ("i_rv", "i_rmin", "i_rmax", "i_rseed", "i_ev", "i_eseed", "i_mv", "i_msets", "i_mlen", "i_mseed", "i_io", "i_in", "i_tseed", "i_cseed", "i_ccount", "i_clen",
         "i_src", "i_lenf", "i_dix", "i_dkind", "i_stf")
IMAGE_SC = ("i_thr", "i_var", "i_rlen", "i_rop", "i_rok", "i_oprow", "i_cnt")
LAYOUT_NAMES = IMAGE + IMAGE_SC + ("a_dlen", "a_dst", "m_off", "m_status", "m_len")


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pad256(x):
    return (x + 255) & ~255


def mem_bytes(count):
    return 10 + 4 + 8 * count + 256 + 32


def con_bytes(k):
    return 0 if k == 0 else 10 + 4 + 32 * k + (4 + RP) * (k - 1) + 32 * (k - 1) + 32


def le(x, n):
    return int(x).to_bytes(n, "little")


class Ops:
    """a caller's op list: ops, their value lists and one seed per op (byte b of op i's seed is distinct per op)"""

    def __init__(self):
        self.rows, self.lists = [], []

    def add(self, kind, a=0, b=0, c=0, vals=None, count=None):
        off = len(self.lists)
        if vals is not None:
            self.lists.extend(vals)
        self.rows.append((kind, len(vals or ()) if count is None else count, a, b, c, off))
        return self

    def arrays(self, flagged):
        ops = np.array(self.rows, dtype=OP).reshape(len(self.rows))
        if flagged:
            ops["kind"] |= FLAG
        lists = np.array(self.lists + [0xDEAD], dtype=np.uint64)          # never empty, so never a null pointer
        n = len(ops)
        seeds = ((np.arange(32 * max(n, 1)) * 131 + 7) % 251).astype(np.uint8)
        return ops, lists, seeds


def op_max(kind, count):
    return {RANGE: RANGE_BYTES, EQ: EQ_BYTES, THR: THR_BYTES, MEM: mem_bytes(count if count <= MAX_SET else 0), IMP: IMP_MAX, CON: con_bytes(count)}[kind]


def model(ops, lists, seeds, gidx, flagged):
    """The rules restated: returns (layout dict, var table, row_ok, image, products)."""
    n = len(gidx)
    lists = [int(x) for x in lists]
    o = [tuple(int(x) for x in ops[g]) for g in gidx]
    o = [(k & ~FLAG, cnt, a, b, c, off) for k, cnt, a, b, c, off in o]
    vals = [lists[off:off + cnt] if k in (THR, CON) or (k == MEM and cnt <= MAX_SET) else [] for k, cnt, a, b, c, off in o]
    row_ok = []
    for (k, cnt, a, b, c, off), v in zip(o, vals):
        row_ok.append({EQ: a == b, MEM: 0 < cnt <= MAX_SET and a in v, IMP: b > a}.get(k, True))
    rows = [0] * 7
    stride = [0, RANGE_BYTES, EQ_BYTES, THR_BYTES, 0, IMP_MAX, 0]
    for (k, cnt, *_), ok in zip(o, row_ok):
        rows[k] += 1 if ok else 0
        if k == MEM and ok:
            stride[MEM] = max(stride[MEM], mem_bytes(cnt))          # valid ops only
        if k == CON:
            stride[CON] = max(stride[CON], con_bytes(cnt or 1))     # all ops, an empty list counted as one value
    R, E, T, M, I, C = (rows[k] for k in (RANGE, EQ, THR, MEM, IMP, CON))
    lay, sizes = {}, {}

    def block(names_sizes):
        off = 0
        for name, size in names_sizes:
            lay[name], sizes[name] = off, size
            off += pad256(size)
        return off
    row0, total = [0] * 7, 0
    if flagged:
        for k in range(7):
            row0[k] = total
            total += (rows[k] + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN
    image_regions = [("i_rv", 8 * R), ("i_rmin", 8 * R), ("i_rmax", 8 * R), ("i_rseed", 32 * R), ("i_ev", 8 * E), ("i_eseed", 32 * E), ("i_mv", 8 * M), ("i_msets", 8 * MAX_SET * M),
                     ("i_mlen", 4 * M), ("i_mseed", 32 * M), ("i_io", 8 * I), ("i_in", 8 * I), ("i_tseed", 32 * T), ("i_cseed", 32 * C), ("i_ccount", 4 * C), ("i_clen", 4 * C),
                     ("i_src", 8 * n), ("i_lenf", 4 * n), ("i_dix", 4 * n), ("i_dkind", n), ("i_stf", 4 * n)]
    if flagged:
        image_regions += [("i_thr", 8 * T), ("i_var", n), ("i_rlen", 4 * total), ("i_rop", 4 * total), ("i_rok", total), ("i_oprow", 4 * n), ("i_cnt", 8)]
    in_bytes = block(image_regions)
    if not flagged:
        for name in IMAGE_SC:
            lay[name], sizes[name] = 0, 0
    arena_order = (RANGE, EQ, MEM, IMP, THR, CON)
    arena_bytes = block([("arena%d" % k, stride[k] * rows[k]) for k in arena_order] + [("a_dlen", 4 * (R + I)), ("a_dst", 4 * R)])
    arena = [0] + [lay["arena%d" % k] for k in range(1, 7)]
    meta_bytes = block([("m_off", 8 * (n + 1)), ("m_status", 4 * n), ("m_len", 4 * n)])
    max_total = sum(op_max(k, cnt) for k, cnt, *_ in o)
    # ---- the image
    img = bytearray([FILL]) * in_bytes

    def put(name, index, width, value):
        at = lay[name] + width * index
        img[at:at + width] = le(value, width) if not isinstance(value, (bytes, bytearray)) else value
    seen = [0] * 7
    thr_img, con_img = bytearray(stride[THR] * T), bytearray(stride[CON] * C)
    thr_jobs, thr_commits, con_jobs, con_commits, con_counts, con_lens, variant = [], [], [], [], [], [], []
    for j, ((k, cnt, a, b, c, off), v, ok) in enumerate(zip(o, vals, row_ok)):
        seed = bytes(seeds[32 * gidx[j]:32 * gidx[j] + 32])                                 # by the op's index in the CALLER's list
        src = lenf = dix = 0
        dkind, st = DYN_NONE, 0 if ok else 1
        variant.append(k if ok else 0)
        if ok:
            r = seen[k]
            seen[k] += 1
            src = arena[k] + stride[k] * r
        if k == RANGE:
            put("i_rv", r, 8, a), put("i_rmin", r, 8, b), put("i_rmax", r, 8, c), put("i_rseed", r, 32, seed)
            lenf, dix, dkind = LEN_DYN, r, DYN_LEN_STATUS
        elif k == EQ and ok:
            put("i_ev", r, 8, a), put("i_eseed", r, 32, seed)
            lenf = EQ_BYTES
        elif k == MEM and ok:
            put("i_mv", r, 8, a), put("i_mlen", r, 4, cnt), put("i_mseed", r, 32, seed)
            for slot in range(MAX_SET):
                put("i_msets", MAX_SET * r + slot, 8, v[slot] if slot < cnt else 0)
            lenf = mem_bytes(cnt)
        elif k == IMP and ok:
            put("i_io", r, 8, a), put("i_in", r, 8, b)
            lenf, dix, dkind = LEN_DYN, R + r, DYN_LEN_ONLY                                   # the improvement lengths lie behind the range lengths
        elif k == THR:
            put("i_tseed", r, 32, seed)
            if flagged:
                put("i_thr", r, 8, a)
            total_v = sum(v)
            framed = cnt > 0 and total_v < 2**64 and total_v >= a
            if framed:
                base = stride[THR] * r
                thr_img[base:base + 26] = bytes([2, 3]) + le(8 + 4 + 4 + RP + 32, 4) + le(32, 4) + le(a, 8) + le(64, 4) + le(RP, 4)
                thr_jobs.append((total_v - a, r, 0, 0, 2**64 - 1, KIND_THRESHOLD, base + 26, base + 26 + RP))
                thr_commits.append((total_v, r, 0, base + 26 + RP + 32))
                lenf = THR_BYTES
            else:
                st = 1
        elif k == CON:
            put("i_cseed", r, 32, seed)
            framed = cnt > 0 and all(x <= y for x, y in zip(v, v[1:]))
            if framed:
                base, need = stride[CON] * r, con_bytes(cnt)
                con_img[base:base + 14] = bytes([2, 6]) + le(need - 10 - 32, 4) + le(32, 4) + le(cnt, 4)
                commits = base + 14
                proofs = commits + 32 * cnt
                dcs = proofs + (4 + RP) * (cnt - 1)
                con_commits += [(v[i], r, i, commits + 32 * i) for i in range(cnt)]
                for i in range(1, cnt):
                    at = proofs + (4 + RP) * (i - 1)
                    con_img[at:at + 4] = le(RP, 4)
                    con_jobs.append((v[i] - v[i - 1], r, i - 1, i, i - 1, KIND_CONSISTENCY, at + 4, dcs + 32 * (i - 1)))
                lenf = need
            else:
                st = 1
            con_counts.append(cnt), con_lens.append(lenf)
            put("i_ccount", r, 4, cnt), put("i_clen", r, 4, lenf)
        put("i_src", j, 8, src), put("i_lenf", j, 4, lenf), put("i_dix", j, 4, dix), put("i_dkind", j, 1, dkind), put("i_stf", j, 4, st)
        if flagged:
            put("i_var", j, 1, variant[-1])
    products = {"thr_img": bytes(thr_img), "con_img": bytes(con_img), "con_counts": con_counts, "con_lens": con_lens, "op_variant": variant if flagged else [],
                "thr_jobs": thr_jobs, "thr_commits": thr_commits, "con_jobs": con_jobs, "con_commits": con_commits}
    head = {"max_total": max_total, "in_bytes": in_bytes, "arena_bytes": arena_bytes, "meta_bytes": meta_bytes}
    var = [(rows[k], stride[k], arena[k], row0[k]) for k in range(7)]
    return head, lay, sizes, var, [int(x) for x in row_ok], bytes(img), products


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_batch_plan.so"))
    vp = ctypes.c_void_p
    L.emul_bp_layout_words.restype = ctypes.c_uint32
    L.emul_bp_plan_shards.argtypes = [ctypes.c_uint64, vp, ctypes.c_uint32, vp]
    L.emul_bp_plan.argtypes = [ctypes.c_uint32, vp, vp, vp, ctypes.c_int, vp, vp]
    L.emul_bp_fill.argtypes = [vp, vp, vp, vp]
    L.emul_bp_product.argtypes = [ctypes.c_uint32, vp]
    L.emul_bp_product.restype = ctypes.c_uint64
    S = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_self_check.so"))
    assert S.emul_sc_row_align() == ROW_ALIGN and ctypes.c_uint32(S.emul_sc_no_row()).value == NO_ROW
    L.self_check = S
    return L


def product(L, which, dtype, cols=None):
    size = L.emul_bp_product(which, None)
    a = np.zeros(size // np.dtype(dtype).itemsize, dtype=dtype)
    L.emul_bp_product(which, P(a) if size else None)
    return a if cols is None else [tuple(int(x) for x in row) for row in a.reshape(-1, cols)]


def stage(L, batch, gidx, flagged):
    """the C side's plan and fill of the shard holding ops `gidx`"""
    ops, lists, seeds = batch.arrays(flagged)
    g = np.array(gidx, dtype=np.uint32)
    words = L.emul_bp_layout_words()
    assert words == 4 + 4 * 7 + len(LAYOUT_NAMES)
    layout = np.full(words + 1, 0x5151, dtype=np.uint64)
    row_ok = np.full(len(g) + 1, 0x51, dtype=np.uint8)
    L.emul_bp_plan(len(g), P(g), P(ops), P(lists), int(flagged), P(layout), P(row_ok))
    assert layout[words] == 0x5151 and row_ok[len(g)] == 0x51
    w = [int(x) for x in layout[:words]]
    head = dict(zip(("max_total", "in_bytes", "arena_bytes", "meta_bytes"), w[:4]))
    var = [tuple(w[4 + 4 * k:8 + 4 * k]) for k in range(7)]
    lay = dict(zip(LAYOUT_NAMES, w[32:]))
    image = np.full(head["in_bytes"] + 256, FILL, dtype=np.uint8)                            # 256 guard bytes behind the image
    L.emul_bp_fill(P(ops), P(lists), P(seeds), P(image))
    assert (image[head["in_bytes"]:] == FILL).all()
    products = {"thr_img": product(L, 0, np.uint8).tobytes(), "con_img": product(L, 1, np.uint8).tobytes(), "con_counts": product(L, 2, np.uint32).tolist(),
                "con_lens": product(L, 3, np.uint32).tolist(), "op_variant": product(L, 4, np.uint8).tolist(), "thr_jobs": product(L, 5, np.uint64, 8),
                "thr_commits": product(L, 6, np.uint64, 4), "con_jobs": product(L, 7, np.uint64, 8), "con_commits": product(L, 8, np.uint64, 4)}
    return head, lay, var, row_ok[:len(g)].tolist(), image[:head["in_bytes"]], products, (ops, lists, seeds)


def check_regions(head, lay, sizes, var, flagged):
    """every region 256-aligned, inside its block, disjoint from the others of the block"""
    arena = {"arena%d" % k: var[k][2] for k in range(1, 7)}
    blocks = {"in_bytes": [n for n in IMAGE + (IMAGE_SC if flagged else ())], "arena_bytes": list(arena) + ["a_dlen", "a_dst"], "meta_bytes": ["m_off", "m_status", "m_len"]}
    for total, names in blocks.items():
        spans = sorted(((arena[n] if n in arena else lay[n]), sizes[n], n) for n in names)
        end = 0
        for off, size, name in spans:
            assert off % 256 == 0 and off + size <= head[total], (name, off, size, head[total])
            if size:
                assert off >= end, (name, off, end)
                end = off + size
        assert head[total] % 256 == 0


def check_self_check_rows(L, n, lay, var, image, variant):
    """k_self_check_rows' step over the plan's geometry: row_op[op_row[i]] == i for every op with a row, SC_NO_ROW for the rest"""
    total = sum((v[0] + ROW_ALIGN - 1) // ROW_ALIGN * ROW_ALIGN for v in var)
    at = lambda name: ctypes.c_void_p(image.ctypes.data + lay[name])  # noqa: E731
    dyn_len = np.zeros(var[RANGE][0] + var[IMP][0] + 1, dtype=np.uint32)
    dyn_status = np.zeros(var[RANGE][0] + 1, dtype=np.int32)
    geo = [np.array([v[c] for v in var], dtype=dt) for c, dt in ((2, np.uint64), (1, np.uint64), (3, np.uint32), (0, np.uint32))]          # base, stride, row0, rows
    row_len, row_op, op_row = (np.full(m + 1, 0xDEAD, dtype=np.uint32) for m in (total, total, n))
    L.self_check.emul_sc_rows(n, at("i_src"), at("i_lenf"), at("i_dix"), at("i_dkind"), at("i_stf"), P(dyn_len), P(dyn_status), at("i_var"),
                              P(geo[0]), P(geo[1]), P(geo[2]), P(geo[3]), P(row_len), P(row_op), P(op_row))
    taken = set()
    for i in range(n):
        if variant[i] == 0:
            assert op_row[i] == NO_ROW
            continue
        g = int(op_row[i])
        k = variant[i]
        assert var[k][3] <= g < var[k][3] + var[k][0] and row_op[g] == i and g not in taken, (i, g)
        taken.add(g)
    assert all(v[3] % ROW_ALIGN == 0 for v in var) and row_op[total] == 0xDEAD and op_row[n] == 0xDEAD


def check(L, batch, gidx=None, flagged=False):
    gidx = list(range(len(batch.rows))) if gidx is None else gidx
    head, lay, var, row_ok, image, products, (ops, lists, seeds) = stage(L, batch, gidx, flagged)
    m_head, m_lay, sizes, m_var, m_row_ok, m_image, m_products = model(ops, lists, seeds, gidx, flagged)
    assert head == m_head
    assert var == m_var
    assert lay == {name: m_lay[name] for name in LAYOUT_NAMES}
    assert row_ok == m_row_ok
    if image.tobytes() != m_image:
        bad = np.nonzero(image != np.frombuffer(m_image, dtype=np.uint8))[0]
        region = max((off, name) for name, off in lay.items() if name.startswith("i_") and off <= bad[0])
        raise AssertionError("image differs at byte %d (%s + %d): %d for %d" % (bad[0], region[1], bad[0] - region[0], image[bad[0]], m_image[bad[0]]))
    assert products == m_products
    check_regions(head, lay, sizes, var, flagged)
    # the sum zkp_hip_process_batch_bytes returns for the same ops
    mine = np.ascontiguousarray(ops[gidx]) if len(gidx) else np.zeros(0, dtype=OP)
    total = ctypes.c_uint64(1)
    assert _native.lib().zkp_hip_process_batch_bytes(len(mine), P(mine) if len(mine) else None, ctypes.byref(total)) == 0, _native.last_error()
    assert total.value == head["max_total"]
    if flagged:
        check_self_check_rows(L, len(gidx), lay, var, image, products["op_variant"])
    return head, lay, var, image, products


def both(L, batch, gidx=None):
    return check(L, batch, gidx, False), check(L, batch, gidx, True)


def all_kinds():
    """two or more of every kind, interleaved: valid and refused ops of each, lists of different lengths"""
    b = Ops()
    b.add(RANGE, 5, 0, 100).add(EQ, 77, 77).add(THR, 10, vals=(4, 5, 6)).add(MEM, 3, vals=(1, 2, 3)).add(IMP, 10, 20).add(CON, vals=(1, 2, 2, 9))
    b.add(EQ, 1, 2).add(RANGE, 500, 0, 100).add(MEM, 9, vals=tuple(range(64))).add(CON, vals=(7,)).add(IMP, 5, 5).add(THR, 50, vals=(1, 2))
    b.add(CON, vals=(3, 2)).add(MEM, 99, vals=tuple(range(40))).add(EQ, 2**64 - 1, 2**64 - 1).add(THR, 0, vals=(2**64 - 1,)).add(IMP, 0, 2**64 - 1).add(RANGE, 2**64 - 1, 1, 2**64 - 1)
    return b


def test_empty_shard(lib):
    for (head, lay, var, image, _) in both(lib, Ops()):
        assert head["max_total"] == 0 and head["arena_bytes"] == 0 and head["meta_bytes"] == 256 and all(v[0] == 0 for v in var)
    assert check(lib, Ops())[0]["in_bytes"] == 0 and check(lib, Ops(), flagged=True)[0]["in_bytes"] == 256          # the two counters


@pytest.mark.parametrize("kind", (RANGE, EQ, THR, MEM, IMP, CON))
def test_each_kind_alone(lib, kind):
    b = Ops()
    {RANGE: lambda: b.add(RANGE, 5, 1, 9), EQ: lambda: b.add(EQ, 8, 8), THR: lambda: b.add(THR, 3, vals=(1, 2)), MEM: lambda: b.add(MEM, 4, vals=(4,)),
     IMP: lambda: b.add(IMP, 1, 2), CON: lambda: b.add(CON, vals=(1, 1))}[kind]()
    for (head, lay, var, image, _) in both(lib, b):
        assert [v[0] for v in var] == [1 if k == kind else 0 for k in range(7)]
        assert head["max_total"] == op_max(kind, b.rows[0][1]) and var[kind][2] == 0


def test_all_six_kinds_interleaved(lib):
    (head, lay, var, image, prod), (_, _, fvar, _, fprod) = both(lib, all_kinds())
    assert [v[0] for v in var] == [0, 3, 2, 3, 2, 2, 3] and [v[3] for v in fvar] == [0, 0, 64, 128, 192, 256, 320]
    assert fprod["op_variant"] == [1, 2, 3, 4, 5, 6, 0, 1, 4, 6, 0, 3, 6, 0, 2, 3, 5, 1]
    assert prod["con_lens"] == [con_bytes(4), con_bytes(1), 0] and var[CON][1] == con_bytes(4)


def test_equality_and_improvement_validation(lib):
    b = Ops().add(EQ, 1, 2).add(EQ, 3, 3).add(IMP, 5, 5).add(IMP, 6, 5).add(IMP, 5, 6)          # a != b | a == b | new == old | new < old | new > old
    (head, lay, var, image, _), (_, _, _, _, fprod) = both(lib, b)
    assert var[EQ][0] == 1 and var[IMP][0] == 1 and fprod["op_variant"] == [0, 2, 0, 0, 5]
    assert np.frombuffer(image.tobytes(), dtype="<i4", count=5, offset=lay["i_stf"]).tolist() == [1, 0, 1, 1, 0]
    assert head["max_total"] == 2 * EQ_BYTES + 3 * IMP_MAX                                       # refused ops count too


def test_membership_sets_and_stride(lib):
    # sets of 0, 1, 64 and 65 elements, a value outside its set, and the largest set on an invalid op: it must not widen the stride
    b = Ops().add(MEM, 5, vals=()).add(MEM, 5, vals=(5,)).add(MEM, 63, vals=tuple(range(64))).add(MEM, 64, vals=tuple(range(65))).add(MEM, 99, vals=(1, 2, 3))
    (head, lay, var, image, _), _ = both(lib, b)
    assert var[MEM][:2] == (2, mem_bytes(64)) and head["max_total"] == mem_bytes(0) + mem_bytes(1) + mem_bytes(64) + mem_bytes(0) + mem_bytes(3)
    b = Ops().add(MEM, 2, vals=(1, 2, 3)).add(MEM, 99, vals=tuple(range(64))).add(MEM, 7, vals=(7,))
    (head, lay, var, image, _), _ = both(lib, b)
    assert var[MEM][:2] == (2, mem_bytes(3))
    assert np.frombuffer(image.tobytes(), dtype="<u8", count=2, offset=lay["i_src"] + 8).tolist() == [0, var[MEM][2] + mem_bytes(3)]
    assert both(lib, Ops().add(MEM, 99, vals=(1, 2)))[0][2][MEM][:2] == (0, 0)                   # no valid op: no rows, stride 0


def test_threshold_framing(lib):
    # count 0 | sum below the threshold | a sum that wraps 2^64 | a valid op
    b = Ops().add(THR, 0, vals=()).add(THR, 10, vals=(4, 5)).add(THR, 1, vals=(2**64 - 1, 1)).add(THR, 10, vals=(4, 6, 1))
    (head, lay, var, image, prod), _ = both(lib, b)
    assert var[THR][:2] == (4, THR_BYTES) and len(prod["thr_jobs"]) == 1 and prod["thr_jobs"][0][:2] == (1, 3)
    assert np.frombuffer(image.tobytes(), dtype="<u4", count=4, offset=lay["i_lenf"]).tolist() == [0, 0, 0, THR_BYTES]
    assert np.frombuffer(image.tobytes(), dtype="<i4", count=4, offset=lay["i_stf"]).tolist() == [1, 1, 1, 0]
    assert prod["thr_img"][:3 * THR_BYTES] == bytes(3 * THR_BYTES)


def test_consistency_counts_and_stride(lib):
    # counts 0, 1, 2 and 5, a decreasing list; the stride is the maximum over all of them
    b = Ops().add(CON, vals=()).add(CON, vals=(4,)).add(CON, vals=(4, 4)).add(CON, vals=(1, 2, 3, 4, 5)).add(CON, vals=(3, 2, 1))
    (head, lay, var, image, prod), _ = both(lib, b)
    assert var[CON][:2] == (5, con_bytes(5)) and prod["con_lens"] == [0, con_bytes(1), con_bytes(2), con_bytes(5), 0] and prod["con_counts"] == [0, 1, 2, 5, 3]
    assert len(prod["con_jobs"]) == 0 + 0 + 1 + 4 and len(prod["con_commits"]) == 1 + 2 + 5
    # a refused op carries the longest list: it still sets the stride; an empty list alone is sized as one value
    assert both(lib, Ops().add(CON, vals=(1, 2)).add(CON, vals=(9, 8, 7, 6)))[0][2][CON][:2] == (2, con_bytes(4))
    assert both(lib, Ops().add(CON, vals=()))[0][2][CON][:2] == (1, con_bytes(1))


def test_two_shards_take_their_seeds_by_global_index(lib):
    b = Ops()                                                                                     # kinds in blocks, so that a shard's ops are not contiguous
    for i in range(4):
        b.add(RANGE, i, 0, 9)
    for i in range(4):
        b.add(EQ, i, i)
    b.add(THR, 1, vals=(1,)).add(THR, 2, vals=(1, 1)).add(CON, vals=(1, 2)).add(CON, vals=(3,)).add(MEM, 1, vals=(1,)).add(MEM, 2, vals=(1, 2)).add(IMP, 1, 2).add(IMP, 2, 3)
    ops, lists, seeds = b.arrays(False)
    owner = np.full(len(ops), 99, dtype=np.uint32)
    lib.emul_bp_plan_shards(len(ops), P(ops), 2, P(owner))
    shards = [[i for i in range(len(ops)) if owner[i] == s] for s in (0, 1)]
    assert sorted(shards[0] + shards[1]) == list(range(len(ops)))
    for kind in (RANGE, EQ, THR, MEM, IMP, CON):                                                  # every bucket cut into halves +-1, in order
        bucket = [i for i in range(len(ops)) if ops["kind"][i] == kind]
        assert [owner[i] for i in bucket] == sorted(owner[i] for i in bucket) and abs(2 * sum(int(owner[i]) for i in bucket) - len(bucket)) <= 1
    gidx = shards[1]
    assert gidx != list(range(gidx[0], gidx[0] + len(gidx)))                                      # not contiguous
    (head, lay, var, image, _), _ = both(lib, b, gidx)
    both(lib, b, shards[0])
    first_range = next(i for i in gidx if ops["kind"][i] == RANGE)
    assert first_range != gidx.index(first_range)
    assert image[lay["i_rseed"]:lay["i_rseed"] + 32].tobytes() == seeds[32 * first_range:32 * first_range + 32].tobytes()
    max_total = sum(check(lib, b, s)[0]["max_total"] for s in shards)
    assert max_total == check(lib, b)[0]["max_total"]


@pytest.mark.parametrize("rows", (63, 64, 65))
def test_rows_across_the_row_alignment(lib, rows):
    b = Ops()
    for i in range(rows):
        b.add(EQ, i, i)
        if i in (10, 40):
            b.add(THR, 1, vals=(i,))
    (_, _, var, _, _), (_, flay, fvar, _, _) = both(lib, b)
    assert [v[3] for v in var] == [0] * 7                                                          # unflagged: no rows are laid out
    want = (rows + 63) // 64 * 64
    assert fvar[EQ][3] == 0 and fvar[THR][3] == want and fvar[MEM][3] == want + 64
    assert flay["i_rop"] - flay["i_rlen"] == pad256(4 * (want + 64))


def test_the_program_of_its_own_passes_under_host_sanitizers(tmp_path):
    """the emulation has a main that stages the all-kinds batch into buffers of exactly the planned size: built as a program with
    -fsanitize=address,undefined and run stand-alone"""
    import __graft_entry__ as ge
    exe = str(tmp_path / "emul_batch_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ge.EMUL_DIR, "emul_batch_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emul_batch_plan ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
