"""ZKP_HIP_OP_SELF_CHECK in zkp_hip_op::kind (include/libzkp_hip.h), as the two entry points that need no device see it: the flag is a
property of the whole batch, every reader of `kind` masks it, and a flagged list plans and sizes exactly as the same list unflagged."""
import ctypes

import numpy as np

from libzkp_amd import _native, workloads as wl

FLAG = _native.OP_SELF_CHECK


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def mixed_12():
    """two ops of each of the six kinds, interleaved; lists as zkp_hip_process_batch takes them"""
    ops = np.zeros(12, dtype=wl.OP_DTYPE)
    lists = []

    def put(i, kind, a=0, b=0, c=0, vals=()):
        ops[i] = (kind, len(vals), a, b, c, len(lists))
        lists.extend(vals)
    for r in range(2):
        put(6 * r + 0, wl.OP_RANGE, 5 + r, 0, 100)
        put(6 * r + 1, wl.OP_EQUALITY, 77 + r, 77 + r)
        put(6 * r + 2, wl.OP_THRESHOLD, 10, vals=(4, 5, 6 + r))
        put(6 * r + 3, wl.OP_MEMBERSHIP, 3, vals=(1, 2, 3) if r == 0 else tuple(range(64)))
        put(6 * r + 4, wl.OP_IMPROVEMENT, 10 + r, 20 + r)
        put(6 * r + 5, wl.OP_CONSISTENCY, vals=(1, 2, 2, 9)[:1 + 3 * r])
    return ops, np.array(lists, dtype=np.uint64)


def plan(L, ops, shards):
    owner = np.full(len(ops), 99, dtype=np.uint32)
    rc = L.zkp_hip_plan_shards(len(ops), P(ops), shards, P(owner))
    return rc, owner.tolist()


def size(L, ops):
    total = ctypes.c_uint64(12345)
    rc = L.zkp_hip_process_batch_bytes(len(ops), P(ops), ctypes.byref(total))
    return rc, total.value


def test_flag_value_is_the_header_s():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "libzkp_hip.h")).read()
    assert int(re.search(r"#define ZKP_HIP_OP_SELF_CHECK (0x[0-9a-f]+)u", hdr).group(1), 16) == FLAG == 0x100
    assert re.search(r"ZKP_HIP_COUNTER_BATCH_SELF_CHECK = (\d+)", hdr).group(1) == str(_native.COUNTER_BATCH_SELF_CHECK) == "4"


def test_flagged_list_plans_and_sizes_as_the_unflagged_one():
    L = _native.lib()
    ops, _ = mixed_12()
    flagged = ops.copy()
    flagged["kind"] |= FLAG
    for shards in (1, 2, 3, 5):
        rc0, o0 = plan(L, ops, shards)
        rc1, o1 = plan(L, flagged, shards)
        assert rc0 == 0 and rc1 == 0, (rc0, rc1, _native.last_error())
        assert o0 == o1 and max(o0) < shards
    rc0, t0 = size(L, ops)
    rc1, t1 = size(L, flagged)
    assert (rc0, rc1) == (0, 0), _native.last_error()
    assert t0 == t1 == wl.max_output_bytes(ops)


def test_flag_on_some_ops_only_is_an_argument_error():
    L = _native.lib()
    ops, _ = mixed_12()
    for some in ([0], [11], list(range(1, 12)), [3, 4, 5]):
        mix = ops.copy()
        mix["kind"][some] |= FLAG
        rc, _ = plan(L, mix, 2)
        assert rc == -3 and "self-check is a property of the whole batch" in _native.last_error(), (some, rc, _native.last_error())
        rc, total = size(L, mix)
        assert rc == -3 and "self-check is a property of the whole batch" in _native.last_error(), (some, rc, _native.last_error())


def test_other_bits_of_kind_stay_unknown():
    L = _native.lib()
    ops, _ = mixed_12()
    for bad in (0 | FLAG, 7 | FLAG, 0x200 | 1, 0x1000100 | 1):
        b = ops.copy()
        b["kind"] |= FLAG
        b["kind"][4] = bad
        assert plan(L, b, 2)[0] == -3 and "unknown operation kind" in _native.last_error(), hex(bad)
        assert size(L, b)[0] == -3 and "unknown operation kind" in _native.last_error(), hex(bad)
