"""The verdict of the Bulletproofs whole-batch check itself (bpv_impl.inc, kernels k_rlc_* of bpv_kernels.hip) on the MI355X.

By default the check is only a shortcut: when it does not stand the per-job path runs and the verdicts are right either way, so
a check that refused clean batches would show only as a slower verifier.  With ZKP_HIP_BP_BATCH_VERIFY_ONLY a call whose check
does not stand fails ("the batch check did not stand"), which makes its verdict observable: clean batches must stand, and every
well-formed forgery of tests/bp_forge.py that reaches a verification equation -- a wrong value in each of the 17 point slots and 5
scalars of a proof -- must be refused by the check alone.  The weights are fresh operating-system randomness in every call; a
false accept has probability 2^-128, so nothing here is retried or skipped.

Two kinds of forgery never enter the sum, by the order of upstream's own rules (tests/test_bp_forge.py pins the kind of every
forgery against the Python oracle): a proof point that is the identity, and an embedded commitment or digest that disagrees with the
envelope's.  The parse / decode steps reject those envelopes before the combination, as they do for envelopes that do not decode,
so with the ONLY switch the call returns 0 with exactly that row refused; asserting "did not stand" for them would ask the verifier
to skip a rule upstream applies first."""
import ctypes

import numpy as np
import pytest

import bp_forge as F
from util import P, U64, oracle_verify

pytestmark = pytest.mark.gpu

ONLY, MIN = "ZKP_HIP_BP_BATCH_VERIFY_ONLY", "ZKP_HIP_BATCH_VERIFY_MIN"
SIZE = {8: 1094, 16: 1222, 32: 1350, 64: 1478}
VTB = 256                                                                # block size of k_rlc_points / k_rlc_scatter (bpv_kernels.hip)


@pytest.fixture(scope="module")
def hip():
    from libzkp_amd import _native
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    return L


@pytest.fixture
def alone(monkeypatch):
    """the batch check forced for every size, and no per-job pass behind it"""
    monkeypatch.setenv(ONLY, "1")
    monkeypatch.setenv(MIN, "1")
    return monkeypatch


def prove_range(L, v, mn, mx, bits, rng):
    n = len(v)
    v, mn, mx = (np.array(a, dtype=np.uint64) for a in (v, mn, mx))
    seeds = np.frombuffer(rng.bytes(32 * n), dtype=np.uint8).copy()
    out = np.zeros((n, 1478), dtype=np.uint8); lens = np.zeros(n, dtype=np.uint32); st = np.zeros(n, dtype=np.int32)
    assert L.zkp_hip_prove_range_batch(n, P(v), P(mn), P(mx), bits, P(seeds), P(out), 1478, P(lens), P(st)) == 0
    assert (lens == SIZE[bits]).all()
    return [out[i, :lens[i]].tobytes() for i in range(n)]


def random_range(L, n, bits, rng, same_bounds=False):
    cap = min(2**bits - 1, 2**62)
    span = rng.integers(1, cap, n, dtype=np.uint64, endpoint=True)
    mn = rng.integers(0, 2**40, n, dtype=np.uint64)
    if same_bounds:
        span[:] = cap; mn[:] = 1000
    v = mn + rng.integers(0, 2**62, n, dtype=np.uint64) % (span + np.uint64(1))
    mx = mn + span
    return prove_range(L, v, mn, mx, bits, rng), [int(x) for x in mn], [int(x) for x in mx]


def random_threshold(n, bits, rng, thr=None):
    import libzkp_amd as z
    cap = min(2**bits - 1, 2**40)
    lists = [[int(x) for x in rng.integers(0, 2**30, int(k))] for k in rng.integers(1, 5, n)]
    if thr is None:
        ths = [sum(v) - int(rng.integers(0, min(cap, sum(v)), endpoint=True)) for v in lists]
    else:                                                               # one threshold for the whole batch
        lists = [[thr + int(rng.integers(0, cap, endpoint=True))] for _ in range(n)]
        ths = [thr] * n
    return z.prove_threshold_batch(lists, ths, seeds=rng.bytes(32 * n), n_bits=bits), ths


def random_consistency(ks, rng):
    import libzkp_amd as z
    data = [sorted(int(x) for x in rng.integers(0, 2**50, k)) for k in ks]
    return z.prove_consistency_batch(data, seeds=rng.bytes(32 * len(data)))


def gpu_verify(scheme, envs, *bounds):
    """verdicts of one call; raises NativeError when the call fails"""
    import libzkp_amd as z
    if scheme == 1:
        return z.verify_range_batch(envs, *bounds)
    if scheme == 3:
        return z.verify_threshold_batch(envs, *bounds)
    return z.verify_consistency_batch(envs)


def oracle_accepts_all(oracle_c, scheme, envs, *bounds):
    if scheme == 1:
        stride = max(len(e) for e in envs)
        buf = np.zeros((len(envs), stride), dtype=np.uint8)
        for i, e in enumerate(envs):
            buf[i, :len(e)] = np.frombuffer(e, dtype=np.uint8)
        lens = np.array([len(e) for e in envs], dtype=np.uint32)
        mn, mx = (np.array(b, dtype=np.uint64) for b in bounds)
        return bool(oracle_verify(oracle_c, buf, lens, mn, mx, threads=16)[1].all())
    return all(F.c_verify(oracle_c, e, *(b[i] for b in bounds)) for i, e in enumerate(envs))


def stands(oracle_c, scheme, envs, *bounds):
    """the oracle accepts every envelope and so does the batch check on its own (call under the `alone` fixture)"""
    assert oracle_accepts_all(oracle_c, scheme, envs, *bounds)
    assert gpu_verify(scheme, envs, *bounds) == [True] * len(envs)


def does_not_stand(scheme, envs, *bounds):
    from libzkp_amd._native import NativeError
    with pytest.raises(NativeError, match="the batch check did not stand"):
        gpu_verify(scheme, envs, *bounds)


# ---------------------------------------------------------------------------------------------- a. clean batches stand, alone
def test_clean_range_batches_stand_alone(hip, oracle_c, alone):
    rng = np.random.default_rng(101)
    envs, mn, mx = random_range(hip, 300, 64, rng)
    assert oracle_accepts_all(oracle_c, 1, envs, mn, mx)
    for n in (1, 2, 31, 32, 33, 129, 300):
        assert gpu_verify(1, envs[:n], mn[:n], mx[:n]) == [True] * n, n
    # one envelope 200 times: equal points with equal digits only where the weights' digits agree, equal Niels rows throughout
    assert gpu_verify(1, envs[7:8] * 200, mn[7:8] * 200, mx[7:8] * 200) == [True] * 200
    # the four widths in one batch: 3, 4, 5 and 6 live L / R slots per job side by side
    mixed, mmn, mmx = [], [], []
    for bits in (8, 16, 32, 64):
        e, a, b = random_range(hip, 40, bits, rng)
        mixed.append(e); mmn.append(a); mmx.append(b)
    inter = lambda parts: [x for row in zip(*parts) for x in row]       # noqa: E731
    stands(oracle_c, 1, inter(mixed), inter(mmn), inter(mmx))
    # edge values: v = min, v = max, min = max, max = 2^64 - 1, the widest difference a width can hold
    top = 2**64 - 1
    v, a, b = [5, 900, 7, 2**63 + 5, top, 0, top], [5, 10, 7, 3, 0, 0, top], [10**6, 900, 7, top, top, top, top]
    stands(oracle_c, 1, prove_range(hip, v, a, b, 64, rng), a, b)
    v, a, b = [100, 355, 100, 9], [100, 100, 100, 9], [355, 355, 355, 9]
    stands(oracle_c, 1, prove_range(hip, v, a, b, 8, rng), a, b)


def test_clean_threshold_and_consistency_batches_stand_alone(hip, oracle_c, alone):
    rng = np.random.default_rng(102)
    envs, ths = [], []
    for bits in (64, 8, 16, 32):
        e, t = random_threshold(50, bits, rng)
        envs += e; ths += t
    import libzkp_amd as z
    envs += z.prove_threshold_batch([[10, 20, 30]], [60], seeds=rng.bytes(32)); ths += [60]      # tight: sum == threshold
    stands(oracle_c, 3, envs, ths)
    stands(oracle_c, 3, envs[:1], ths[:1])
    cons = random_consistency([1, 2, 3, 4, 5, 6, 7, 8, 2, 1, 8, 3], rng) + z.prove_consistency_batch([[7, 7]], seeds=rng.bytes(32))
    stands(oracle_c, 6, cons)
    stands(oracle_c, 6, cons[1:2])
    # envelopes of one value only: no job at all, so no batch check; the verdicts are still the oracle's
    singles = random_consistency([1] * 9, rng)
    b = bytearray(singles[4]); b[-1] ^= 1; singles[4] = bytes(b)                                   # its digest
    want = [F.c_verify(oracle_c, e) for e in singles]
    assert want == [True] * 4 + [False] + [True] * 4
    assert gpu_verify(6, singles) == want


# ---------------------------------------------------------------------------------------------- f. granularity
def test_clean_batches_around_the_block_size_stand_alone(hip, oracle_c, alone):
    """17 M point terms just below, at and above a multiple of the 256-thread blocks of k_rlc_points (over M) and k_rlc_scatter (over 17 M)"""
    rng = np.random.default_rng(103)
    envs, ths = random_threshold(513, 64, rng)                          # one job per envelope: M = n
    assert oracle_accepts_all(oracle_c, 3, envs, ths)
    sizes = (15, 16, 30, 241, 255, 256, 257, 271, 511, 512, 513)         # 17 M = 255, 272, 510, 4097 = 16 * 256 + 1, ..., 4607 = 18 * 256 - 1
    assert {17 * 15, 17 * 241, 17 * 271} == {VTB - 1, 16 * VTB + 1, 18 * VTB - 1} and 17 * 256 % VTB == 0
    for n in sizes:
        assert gpu_verify(3, envs[:n], ths[:n]) == [True] * n, n
    renvs, mn, mx = random_range(hip, 129, 64, rng)                     # two jobs per envelope: M = 254, 256, 258
    assert oracle_accepts_all(oracle_c, 1, renvs, mn, mx)
    for n in (127, 128, 129):
        assert gpu_verify(1, renvs[:n], mn[:n], mx[:n]) == [True] * n, n


# ---------------------------------------------------------------------------------------------- b. / e. the default path
def test_the_default_path_at_2048_envelopes_is_the_batch_check_and_it_stands(hip, oracle_c, monkeypatch):
    rng = np.random.default_rng(104)
    n = 2048                                                            # 4096 jobs = RLC_MIN_JOBS
    envs, mn, mx = random_range(hip, n, 64, rng)
    assert oracle_accepts_all(oracle_c, 1, envs, mn, mx)
    monkeypatch.setenv(ONLY, "1")                                       # no override of the threshold
    assert gpu_verify(1, envs, mn, mx) == [True] * n                    # a check that fell back silently would fail here
    forged = [f for f in F.field_forgeries(envs[0]) if f.name == "rp_max.t_x:plus_1"]
    assert len(forged) == 1
    does_not_stand(1, [forged[0].env] + envs[1:], mn, mx)               # and the check did run: it is what refuses this batch
    tenvs, ths = random_threshold(4096, 64, rng)
    sample = list(range(0, 4096, 64))
    assert oracle_accepts_all(oracle_c, 3, [tenvs[i] for i in sample], [ths[i] for i in sample])
    assert gpu_verify(3, tenvs, ths) == [True] * 4096
    does_not_stand(3, tenvs[:4000] + [F.field_forgeries(tenvs[4000])[0].env] + tenvs[4001:], ths)
    # one job fewer than the threshold: the per-job path, which the switch leaves alone
    bad = [F.field_forgeries(tenvs[9])[0].env if i == 9 else tenvs[i] for i in range(4095)]
    assert gpu_verify(3, bad, ths[:4095]) == [i != 9 for i in range(4095)]
    # e. no switch at all: one forged scalar at the first, the last and an interior row; exactly that row is refused
    monkeypatch.delenv(ONLY)
    for row in (0, 2047, 1337):
        f = [f for f in F.field_forgeries(envs[row]) if f.name == "rp_min.a:plus_1"][0]
        batch = envs[:row] + [f.env] + envs[row + 1:]
        got = gpu_verify(1, batch, mn, mx)
        assert got == [i != row for i in range(n)], row
        for i in sorted({row, 0, 1, row // 2, max(row - 1, 0), min(row + 1, n - 1), n - 1}):
            assert F.c_verify(oracle_c, batch[i], mn[i], mx[i]) == got[i], (row, i)


# ---------------------------------------------------------------------------------------------- c. / d. forgeries and exclusions
def batch_of_64(hip, scheme, bits, rng):
    """64 valid envelopes under the same bounds; rows 0 and 1 have the same shape (base and donor of the forger)"""
    if scheme == 1:
        envs, mn, mx = random_range(hip, 64, bits, rng, same_bounds=True)
        return envs, (mn, mx)
    if scheme == 3:
        envs, ths = random_threshold(64, bits, rng, thr=12345)
        return envs, (ths,)
    return random_consistency([3, 3] + [int(k) for k in rng.integers(1, 9, 62)], rng), ()


CASES = [(1, 64), (1, 8), (3, 64), (6, 64)]


@pytest.mark.parametrize("scheme,bits", CASES)
def test_every_forged_field_is_refused_by_the_check_alone(hip, oracle_c, monkeypatch, scheme, bits):
    rng = np.random.default_rng(105 + scheme + bits)
    envs, bounds = batch_of_64(hip, scheme, bits, rng)
    assert oracle_accepts_all(oracle_c, scheme, envs, *bounds)
    row_bounds = [b[0] for b in bounds]                                 # the same in every row
    forged = F.forgeries(envs[0], donor=envs[1])
    lg, n_proofs, n_comm = {8: 3, 64: 6}[bits], {1: 2, 3: 1, 6: 2}[scheme], {1: 3, 3: 2, 6: 5}[scheme]
    n_fields = n_proofs * ((4 + 2 * lg) * 3 + 5 * 2) + n_comm * 3
    assert len(F.field_forgeries(envs[0])) == n_fields and len(forged) == n_fields + {1: 3, 3: 2, 6: 7}[scheme]
    ran, stages = 0, {"equation": 0, "rule": 0}
    monkeypatch.setenv(MIN, "1")
    for idx, f in enumerate(forged):
        row = (0, 63, 1 + (7 * idx) % 62)[idx % 3]                      # first, last and interior rows in turn
        batch = envs[:row] + [f.env] + envs[row + 1:]
        want = [i != row for i in range(64)]
        assert F.c_verify(oracle_c, f.env, *row_bounds) is False, f.name
        monkeypatch.setenv(ONLY, "1")
        if f.stage == "equation":
            does_not_stand(scheme, batch, *bounds)
        else:                                                           # refused by a rule before the sum, which stands for the other 63
            assert gpu_verify(scheme, batch, *bounds) == want, f.name
        monkeypatch.delenv(ONLY)
        assert gpu_verify(scheme, batch, *bounds) == want, f.name       # the per-job pass names exactly the forged row
        ran += 1; stages[f.stage] += 1
    assert ran == len(forged)
    n_identity = n_proofs * (4 + 2 * lg)
    assert stages["rule"] == n_identity + n_comm * 3 + {1: 0, 3: 0, 6: 2}[scheme] and stages["equation"] == ran - stages["rule"]
    # opposite errors in two copies of one envelope: each refused alone, both together, and both named by the per-job pass
    for idx, (name, plus, minus) in enumerate(F.opposite_pairs(envs[0])):
        r1, r2 = (0, 63) if idx % 2 == 0 else (5 + idx, 40 + idx)
        both = list(envs); both[r1], both[r2] = plus, minus
        one = list(envs); one[r2] = minus
        assert F.c_verify(oracle_c, minus, *row_bounds) is False and F.c_verify(oracle_c, plus, *row_bounds) is False, name
        monkeypatch.setenv(ONLY, "1")
        does_not_stand(scheme, both, *bounds)
        does_not_stand(scheme, one, *bounds)
        monkeypatch.delenv(ONLY)
        assert gpu_verify(scheme, both, *bounds) == [i not in (r1, r2) for i in range(64)], name


@pytest.mark.parametrize("scheme,bits", CASES)
def test_excluded_envelopes_leave_the_check_standing(hip, oracle_c, alone, scheme, bits):
    rng = np.random.default_rng(205 + scheme + bits)
    envs, bounds = batch_of_64(hip, scheme, bits, rng)
    assert oracle_accepts_all(oracle_c, scheme, envs, *bounds)
    ex = F.excluded(envs[0])
    assert len(ex) >= 5 + 3 * (4 + 2 * 3 + 2)
    batch, want, bb = [], [], [[] for _ in bounds]
    for i in range(max(len(ex), 64)):                                    # valid and excluded rows alternate; the batch ends on an excluded one
        for e, good in ((envs[i % 64], True), (ex[i % len(ex)][1], False)):
            batch.append(e); want.append(good)
            for k, b in enumerate(bounds):
                bb[k].append(b[0])
    for name, e in ex[::7]:
        assert F.c_verify(oracle_c, e, *(b[0] for b in bounds)) is False, name
    assert gpu_verify(scheme, batch, *bb) == want
    only_excluded = [e for _, e in ex]
    assert gpu_verify(scheme, only_excluded, *([b[0]] * len(ex) for b in bounds)) == [False] * len(ex)
