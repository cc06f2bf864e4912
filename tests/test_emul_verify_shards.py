"""How one verify call is cut over the registered shards, on the host (no GPU): the plan of libzkp_amd/csrc/verify_shards.h compiled from
the header the library uses (tests/emul/emul_verify_shards.cpp) -- weights, slice count, slice boundaries, participating shards."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

U64 = ctypes.c_uint64
SHARDS = (1, 2, 3, 8, 64)
MINS = (1, 3, 4, 7, 4096, 8193)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_verify_shards.so"))
    L.emul_vs_plan_uniform.argtypes = [U64, ctypes.c_uint32, ctypes.c_uint32, U64, ctypes.c_void_p]
    L.emul_vs_plan_weighted.argtypes = [U64, ctypes.c_void_p, ctypes.c_uint32, U64, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_vs_participants.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_vs_list_fanout.argtypes = [U64, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, U64, U64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.emul_vs_list_fanout.restype = None
    for f in (L.emul_vs_plan_uniform, L.emul_vs_plan_weighted, L.emul_vs_participants, L.emul_vs_max_shards):
        f.restype = ctypes.c_uint32
    return L


def P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def plan_uniform(L, n, unit, shards, min_jobs):
    b = np.full(66, 2**64 - 1, dtype=np.uint64)
    c = L.emul_vs_plan_uniform(n, unit, shards, min_jobs, P(b))
    assert (b[min(shards, 64) + 1:] == 2**64 - 1).all()                # shards + 1 entries at the most (counts tried and dropped use them too)
    return [int(x) for x in b[:c + 1]]


def plan_weighted(L, weights, shards, min_jobs):
    w = np.asarray(weights, dtype=np.uint32)
    b = np.full(66, 2**64 - 1, dtype=np.uint64)
    prefix = np.zeros(len(w) + 1, dtype=np.uint64)
    c = L.emul_vs_plan_weighted(len(w), P(w), shards, min_jobs, P(b), P(prefix))
    counted = np.maximum(w, 1).astype(np.uint64)                       # a zero-job envelope still costs something
    assert (prefix == np.concatenate(([0], np.cumsum(counted)))).all()
    return [int(x) for x in b[:c + 1]], prefix.astype(object)


def check_partition(bounds, n, shards):
    """contiguous, in order, covers [0, n), none empty, at most `shards` slices"""
    assert bounds[0] == 0 and bounds[-1] == n
    assert all(lo < hi for lo, hi in zip(bounds, bounds[1:]))
    assert 1 <= len(bounds) - 1 <= shards


@pytest.mark.parametrize("unit", (1, 2))
@pytest.mark.parametrize("shards", SHARDS)
def test_uniform_weights(lib, unit, shards):
    for n in (1, 2, 3, 12, 13, 64, 65, 1000, 4095, 4096, 8191, 8192, 8193, 16384, 65536):
        for m in MINS:
            bounds = plan_uniform(lib, n, unit, shards, m)
            check_partition(bounds, n, shards)
            count, total = len(bounds) - 1, n * unit
            sizes = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
            assert max(sizes) - min(sizes) <= 1 and set(sizes) <= {n // count, -(-n // count)}       # equal envelope counts +-1
            assert count <= max(1, min(shards, total // m))
            assert count == 1 or min(sizes) * unit >= m                                              # every slice takes the path a batch of its size takes
            if total < 2 * m:
                assert count == 1
            if m % unit == 0 and m >= unit:                                                          # the stated count exactly: min(S, total / min), at least 1
                assert count == max(1, min(shards, total // m))


def test_the_cases_the_library_meets(lib):
    # 13 envelopes, two shards, a minimum of 4 jobs: slices of 7 and 6, whatever the unit weight
    assert plan_uniform(lib, 13, 1, 2, 4) == [0, 7, 13] and plan_uniform(lib, 13, 2, 2, 4) == [0, 7, 13]
    # 65 536 Groth16 envelopes on eight shards at the default threshold: seven slices would be 9362 each, eight are 8192 < 8193
    assert len(plan_uniform(lib, 65536, 1, 8, 8193)) - 1 == 7
    assert plan_uniform(lib, 65544, 1, 8, 8193) == [8193 * s for s in range(9)]
    # 16 384 range envelopes (32 768 jobs) on eight shards at the default threshold of 4096 jobs: eight slices of 2048 envelopes
    assert plan_uniform(lib, 16384, 2, 8, 4096) == [2048 * s for s in range(9)]
    # below twice the minimum: one slice; an odd minimum under weight 2 lowers the count until every slice reaches it (15 * 2 = 30 jobs, min 7)
    assert plan_uniform(lib, 4095, 2, 8, 4096) == [0, 4095]
    assert plan_uniform(lib, 15, 2, 64, 7) == [0, 5, 10, 15]


def test_no_envelope_one_envelope_one_shard_and_sixty_four(lib):
    assert lib.emul_vs_max_shards() == 64
    assert plan_uniform(lib, 0, 2, 8, 1) == [0]                                                      # n = 0: no slice at all
    assert plan_weighted(lib, [], 8, 1)[0] == [0]
    for shards in SHARDS:
        assert plan_uniform(lib, 1, 2, shards, 1) == [0, 1]
        assert plan_weighted(lib, [7], shards, 1)[0] == [0, 1]
    assert plan_uniform(lib, 1000, 1, 1, 1) == [0, 1000]
    assert plan_uniform(lib, 64, 1, 64, 1) == list(range(65))                                        # min_jobs = 1: one envelope per shard
    assert plan_uniform(lib, 63, 1, 64, 1) == list(range(64))                                        # never more slices than envelopes
    assert plan_uniform(lib, 3, 2, 64, 1) == [0, 1, 2, 3]
    assert len(plan_uniform(lib, 1000, 1, 1000, 1)) - 1 == 64                                        # more shards than the library registers: capped


def test_sums_are_64_bit(lib):
    n = 2**32 - 1                                                                                    # 2^33 - 2 jobs
    bounds = plan_uniform(lib, n, 2, 64, 4096)
    check_partition(bounds, n, 64)
    sizes = [hi - lo for lo, hi in zip(bounds, bounds[1:])]
    assert len(sizes) == 64 and set(sizes) <= {n // 64, n // 64 + 1} and bounds == [-(-s * n // 64) for s in range(65)]
    assert plan_uniform(lib, n, 2, 2, 2**32 - 2) == [0, 2**31, n]                                    # a minimum only a 64-bit total reaches twice
    assert plan_uniform(lib, n, 2, 2, 2**32 - 1) == [0, n]                                           # the lighter half weighs 2^32 - 2
    assert plan_uniform(lib, n, 2, 2, 2**32) == [0, n]                                               # total = 2^33 - 2 < 2 * 2^32


@pytest.mark.parametrize("shards", SHARDS)
def test_ragged_weights(lib, shards):
    rng = np.random.default_rng(5)
    for n in (1, 2, 13, 100, 5000, 70000):
        shapes = (np.zeros(n), rng.integers(0, 5, n), np.where(np.arange(n) == n // 2, 100000, 1), rng.integers(0, 1000, n), rng.choice([0, 1, 4], n))
        for w in shapes:
            for m in MINS:
                bounds, prefix = plan_weighted(lib, w, shards, m)
                check_partition(bounds, n, shards)
                count, total = len(bounds) - 1, int(prefix[-1])
                weights = [int(prefix[hi] - prefix[lo]) for lo, hi in zip(bounds, bounds[1:])]
                assert count <= max(1, min(shards, total // m))
                assert count == 1 or min(weights) >= m
                if total < 2 * m:
                    assert count == 1
                wmax = max(int(w.max()), 1)
                assert all(abs(x - total / count) < wmax for x in weights) or count == 1             # no slice further from the mean than the largest envelope
                for s in range(1, count):                                                             # boundary s: the first envelope at which the running weight reaches s * total / count
                    assert prefix[bounds[s]] * count >= s * total and prefix[bounds[s] - 1] * count < s * total


def test_all_zero_consistency_weights_count_as_one_each(lib):
    bounds, prefix = plan_weighted(lib, [0] * 13, 2, 4)
    assert bounds == [0, 7, 13] and int(prefix[-1]) == 13
    assert plan_weighted(lib, [0] * 7, 2, 4)[0] == [0, 7]                                            # 7 < 2 * 4
    # lists of 1, 2 and 5 values: 0, 1 and 4 jobs, counted 1, 1, 4
    bounds, prefix = plan_weighted(lib, [0, 1, 4] * 4 + [0], 2, 4)
    assert int(prefix[-1]) == 25 and bounds == [0, 7, 13]                                            # 13 of 25 jobs are reached inside envelope 6


def test_one_heavy_envelope_does_not_leave_a_light_or_empty_slice(lib):
    assert plan_weighted(lib, [100, 1, 1], 3, 34)[0] == [0, 3]                                       # thirds would be 100 / empty / 2
    assert plan_weighted(lib, [1, 150, 1, 48], 2, 100)[0] == [0, 4]                                  # halves would be 151 / 49
    assert plan_weighted(lib, [1, 150, 1, 48], 2, 49)[0] == [0, 2, 4]


def test_participants(lib):
    def part(caller, holds):
        out = np.full(65, 999, dtype=np.uint32)
        h = np.asarray(holds, dtype=np.uint8)
        m = lib.emul_vs_participants(caller, len(h), P(h), P(out))
        assert out[m] == 999
        return [int(x) for x in out[:m]]
    assert part(0, [1, 1, 1]) == [0, 1, 2]
    assert part(0, [1, 0, 1, 1]) == [0, 2, 3]                       # a shard without the key takes no part
    assert part(2, [1, 0, 1, 1]) == [2, 3, 0]                       # registration order, starting with the caller's
    assert part(1, [1, 0, 1, 1]) == []                              # the caller's shard holds none: the call stays put and fails as it always has
    assert part(0, [1]) == [0]


# ---- the fan-out data of the calls over a list of envelopes of any scheme (vs_list_fanout): the mixed verifier's, the statements call's, the composites call's
def list_fanout(L, weights, need_eq, need_mem, has_key, bp_min=4096, g16_min=8193):
    """-> (prefix, holds, unit, min_jobs); has_key: per shard (equality, membership)"""
    w = np.asarray(weights, dtype=np.uint32)
    k = np.asarray(has_key, dtype=np.uint8).reshape(-1, 2)
    prefix, holds, out = np.full(len(w) + 2, 2**64 - 1, dtype=np.uint64), np.full(len(k) + 1, 77, dtype=np.uint8), np.full(2, 2**64 - 1, dtype=np.uint64)
    L.emul_vs_list_fanout(len(w), P(w), int(need_eq), int(need_mem), len(k), P(k), bp_min, g16_min, P(prefix), P(holds), P(out))
    assert prefix[-1] == 2**64 - 1 and holds[-1] == 77                                               # n + 1 sums and one flag per shard, no more
    return [int(x) for x in prefix[:-1]], [int(x) for x in holds[:-1]], int(out[0]), int(out[1])


KEYS = [(1, 1), (1, 0), (0, 1), (0, 0)]                                                              # four shards: both keys, equality only, membership only, none


def test_list_fanout_without_groth16_work_leaves_every_shard_in(lib):
    prefix, holds, unit, min_jobs = list_fanout(lib, [2, 1, 1], False, False, KEYS)
    assert holds == [1, 1, 1, 1] and prefix == [0, 2, 3, 4] and unit == 0 and min_jobs == 8193
    assert list_fanout(lib, [2, 1, 1], False, False, [(0, 0)] * 3)[1] == [1, 1, 1]


def test_list_fanout_keeps_only_the_shards_that_hold_every_needed_key(lib):
    assert list_fanout(lib, [1], True, False, KEYS)[1] == [1, 1, 0, 0]                               # equality needed
    assert list_fanout(lib, [1], False, True, KEYS)[1] == [1, 0, 1, 0]                               # membership needed: the other column of the table
    assert list_fanout(lib, [1], True, True, KEYS)[1] == [1, 0, 0, 0]                                # both
    assert list_fanout(lib, [1], True, True, [(1, 1)] * 64)[1] == [1] * 64
    assert list_fanout(lib, [1], True, True, [])[1] == []


def test_list_fanout_a_caller_without_the_key_keeps_the_call(lib):
    holds = np.asarray(list_fanout(lib, [1] * 10, True, False, [(0, 1), (1, 1), (1, 0)])[1], dtype=np.uint8)
    assert holds.tolist() == [0, 1, 1]
    out = np.zeros(8, dtype=np.uint32)
    assert lib.emul_vs_participants(0, 3, P(holds), P(out)) == 0                                     # vs_participants, unchanged: the call stays put and fails as it always has
    assert lib.emul_vs_participants(1, 3, P(holds), P(out)) == 2 and out[:2].tolist() == [1, 2]


def test_list_fanout_counts_zero_weights_as_one_and_takes_the_larger_threshold(lib):
    prefix, _, unit, _ = list_fanout(lib, [0, 0, 4, 0, 2], False, False, KEYS)
    assert prefix == [0, 1, 2, 6, 7, 9] and unit == 0                                                # vs_prefix's sums: the plan reads the weights there, not from `unit`
    assert list_fanout(lib, [], False, False, KEYS)[0] == [0]
    for bp_min, g16_min in ((4096, 8193), (8193, 4096), (7, 7), (1, 2**40)):
        assert list_fanout(lib, [1], True, True, KEYS, bp_min, g16_min)[3] == max(bp_min, g16_min)
    # the plan over these data: 16 384 range envelopes of a mixed list on eight shards cut at 8193 jobs, not at 4096
    prefix, holds, unit, min_jobs = list_fanout(lib, [2] * 16384, False, False, [(0, 0)] * 8)
    b = np.zeros(66, dtype=np.uint64)
    pf = np.asarray(prefix, dtype=np.uint64)
    count = lib.emul_vs_plan_weighted(16384, P(np.full(16384, 2, dtype=np.uint32)), sum(holds), min_jobs, P(b), P(pf))
    assert count == 3 and 32768 // 8193 == 3


def test_the_program_of_its_own_passes_under_host_sanitizers(tmp_path):
    """the emulation has a main that walks a grid of cases: built as a program with -fsanitize=address,undefined and run stand-alone"""
    import __graft_entry__ as ge
    exe = str(tmp_path / "emul_verify_shards")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ge.EMUL_DIR, "emul_verify_shards.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emul_verify_shards ok" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
