"""The Bulletproofs batch verifiers after a batch check that did not stand (bp_localise.h; k_bp_seg_*, k_bp_gather, k_bp_scatter of
bpv_kernels.hip; localise_bp of bpv_impl.inc) on the MI355X: segment checks from what the failed check left behind, the per-job pass over
the suspect segments' jobs only.

Every case compares the verdicts with the same call under ZKP_HIP_NO_BATCH_VERIFY (the per-job pass alone) and with the C oracle on the
bad rows and their neighbours, and asserts exactly what the call did from the counters (api.bp_verify_counters).  The weights are fresh
operating-system randomness in every call; a segment with a forged job passes its check with probability 2^-128, so nothing is retried or
skipped."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bp_forge as F
from test_gpu_bp_batch_check import gpu_verify, random_consistency, random_range, random_threshold

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN, NO, SEG, LOC, ONLY = "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY", "ZKP_HIP_BP_LOCALISE_SEGMENT", "ZKP_HIP_BP_LOCALISE", "ZKP_HIP_BP_BATCH_VERIFY_ONLY"
SWITCHES = (MIN, NO, SEG, LOC, ONLY)
TILE_JOBS = 64                                                           # BP_LOC_TILE_JOBS (bp_localise.h): jobs of one tile of k_bp_seg_points, 17 point terms each
ZERO = {"failed_checks": 0, "segment_checks": 0, "jobs_again": 0, "ms": 0.0}


@pytest.fixture(scope="module")
def hip():
    from libzkp_amd import _native
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    return L


@pytest.fixture(scope="module")
def ranges(hip):
    """300 valid 64-bit range envelopes under the same bounds (any row may take a forgery of any other), and 40 of each width"""
    rng = np.random.default_rng(301)
    envs, mn, mx = random_range(hip, 300, 64, rng, same_bounds=True)
    widths = {bits: random_range(hip, 40, bits, rng, same_bounds=True) for bits in (8, 16, 32)}
    return envs, mn, mx, widths


@pytest.fixture(scope="module")
def thresholds(hip):
    return random_threshold(200, 64, np.random.default_rng(302), thr=12345)


def forged(env, name):
    f = [f for f in F.field_forgeries(env) if f.name == name]
    assert len(f) == 1 and f[0].stage == "equation"
    return f[0].env


def expected(jobs, size, bad_rows):
    """what a call must count: jobs = jobs of every envelope, bad_rows = rows with a forgery that reaches an equation"""
    n, M = len(jobs), sum(jobs)
    suspects = sorted({r // size for r in bad_rows})
    again = sum(sum(jobs[s * size:(s + 1) * size]) for s in suspects)
    return {"failed_checks": 1, "segment_checks": -(-n // size), "jobs_again": M if 2 * again >= M else again}


def run(mp, oracle_c, scheme, envs, bounds, bad_rows, size=None, **switches):
    """one call with the batch check forced; verdicts against the per-job pass alone and the oracle; returns the counters"""
    import libzkp_amd.api as api
    n = len(envs)
    mp.setenv(MIN, "1")
    if size:
        mp.setenv(SEG, str(size))
    for k, v in switches.items():
        mp.setenv(k, v)
    api.bp_verify_counters(reset=True)
    got = gpu_verify(scheme, envs, *bounds)
    c = api.bp_verify_counters(reset=True)
    assert api.bp_verify_counters(reset=False) == ZERO                 # reset means reset
    mp.setenv(NO, "1")
    ref = gpu_verify(scheme, envs, *bounds)
    mp.delenv(NO)
    assert api.bp_verify_counters(reset=False) == ZERO                 # no batch check, nothing counted
    for k in (SEG,) + tuple(switches):
        mp.delenv(k, raising=False)
    assert got == ref and got == [i not in bad_rows for i in range(n)]
    near = set()
    for r in bad_rows:
        near |= {max(r - 1, 0), r, min(r + 1, n - 1)}
    for i in sorted(near | {0, n - 1}):
        assert F.c_verify(oracle_c, envs[i], *(b[i] for b in bounds)) == got[i], i
    assert c["ms"] > 0 or c["failed_checks"] == 0
    return {k: c[k] for k in ("failed_checks", "segment_checks", "jobs_again")}


def with_rows(envs, rows):
    out = list(envs)
    for r, e in rows.items():
        out[r] = e
    return out


# ---------------------------------------------------------------------------------------------- range envelopes, two jobs each
@pytest.mark.parametrize("name", ("rp_min.a:plus_1", "rp_max.T1:plus_B"))
def test_one_forged_field_at_the_first_last_and_an_interior_envelope(hip, oracle_c, monkeypatch, ranges, name):
    envs, mn, mx, _ = ranges
    n, size = 128, 8
    for row in (0, n - 1, 77):
        batch = with_rows(envs[:n], {row: forged(envs[row], name)})
        c = run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), {row}, size)
        assert c == expected([2] * n, size, {row}) == {"failed_checks": 1, "segment_checks": 16, "jobs_again": 16}


def test_partial_last_segment_two_in_one_segment_and_segments_of_one(hip, oracle_c, monkeypatch, ranges):
    envs, mn, mx, _ = ranges
    n = 100                                                             # 12 segments of 8 and one of 4
    batch = with_rows(envs[:n], {98: forged(envs[98], "rp_min.a:plus_1")})
    assert run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), {98}, 8) == {"failed_checks": 1, "segment_checks": 13, "jobs_again": 8}
    n = 128
    batch = with_rows(envs[:n], {17: forged(envs[17], "rp_min.a:plus_1"), 22: forged(envs[22], "rp_max.S:neg")})
    assert run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), {17, 22}, 8) == {"failed_checks": 1, "segment_checks": 16, "jobs_again": 16}
    assert run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), {17, 22}, 4) == {"failed_checks": 1, "segment_checks": 32, "jobs_again": 16}
    assert run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), {17, 22}, 1) == {"failed_checks": 1, "segment_checks": 128, "jobs_again": 4}


def test_opposite_errors_in_one_segment_and_in_two(hip, oracle_c, monkeypatch, ranges):
    envs, mn, mx, _ = ranges
    n, size = 128, 8
    for idx, (name, plus, minus) in enumerate(F.opposite_pairs(envs[0])[::2]):
        r1, r2 = 40 + idx, 47                                           # both in segment 5
        c = run(monkeypatch, oracle_c, 1, with_rows(envs[:n], {r1: plus, r2: minus}), (mn[:n], mx[:n]), {r1, r2}, size)
        assert c == {"failed_checks": 1, "segment_checks": 16, "jobs_again": 16}, name
        r1, r2 = 3 + idx, 100                                           # segments 0 and 12
        c = run(monkeypatch, oracle_c, 1, with_rows(envs[:n], {r1: plus, r2: minus}), (mn[:n], mx[:n]), {r1, r2}, size)
        assert c == {"failed_checks": 1, "segment_checks": 16, "jobs_again": 32}, name


def test_a_batch_that_mixes_the_four_bit_widths(hip, oracle_c, monkeypatch, ranges):
    envs, mn, mx, widths = ranges
    parts = [(envs[:40], mn[:40], mx[:40])] + [widths[b] for b in (8, 16, 32)]
    inter = lambda k: [x for row in zip(*(p[k] for p in parts)) for x in row]          # noqa: E731  (64, 8, 16, 32, 64, ...)
    batch, bmn, bmx = inter(0), inter(1), inter(2)
    n, size = 160, 4
    rows = {1: "rp_min.a:plus_1", 78: "rp_max.R1:plus_B", 159: "rp_min.t_x:neg"}                 # an 8-, a 16- and a 32-bit envelope
    assert [len(batch[r]) for r in rows] == [1094, 1222, 1350]
    bad = with_rows(batch, {r: forged(batch[r], name) for r, name in rows.items()})
    assert run(monkeypatch, oracle_c, 1, bad, (bmn, bmx), set(rows), size) == {"failed_checks": 1, "segment_checks": 40, "jobs_again": 24}


def test_half_rule_and_the_off_switch(hip, oracle_c, monkeypatch, ranges):
    envs, mn, mx, _ = ranges
    n, size = 64, 8
    half = {r: forged(envs[r], "rp_min.a:plus_1") for r in (1, 17, 33, 49)}                       # four of eight segments: 64 of 128 jobs
    assert run(monkeypatch, oracle_c, 1, with_rows(envs[:n], half), (mn[:n], mx[:n]), set(half), size) == {"failed_checks": 1, "segment_checks": 8, "jobs_again": 128}
    less = {r: half[r] for r in (1, 17, 33)}
    assert run(monkeypatch, oracle_c, 1, with_rows(envs[:n], less), (mn[:n], mx[:n]), set(less), size) == {"failed_checks": 1, "segment_checks": 8, "jobs_again": 48}
    off = run(monkeypatch, oracle_c, 1, with_rows(envs[:n], less), (mn[:n], mx[:n]), set(less), size, **{LOC: "0"})
    assert off == {"failed_checks": 1, "segment_checks": 0, "jobs_again": 128}
    # the diagnostic switch keeps its place: the call fails at the batch check, before any localisation
    import libzkp_amd.api as api
    from libzkp_amd._native import NativeError
    monkeypatch.setenv(MIN, "1"); monkeypatch.setenv(ONLY, "1")
    with pytest.raises(NativeError, match="the batch check did not stand"):
        gpu_verify(1, with_rows(envs[:n], less), mn[:n], mx[:n])
    assert api.bp_verify_counters(reset=True) == ZERO


def test_rule_refused_envelopes_make_no_segment_suspect(hip, oracle_c, monkeypatch, ranges):
    envs, mn, mx, _ = ranges
    ex = F.excluded(envs[0])[::3][:64]
    batch = [e for i in range(64) for e in (envs[i + 1], ex[i % len(ex)][1])]                      # valid and excluded rows alternate
    n, size = 128, 8
    refused = set(range(1, n, 2))
    c = run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), refused, size)
    assert c == {"failed_checks": 0, "segment_checks": 0, "jobs_again": 0}                         # the check stands for the others
    row = 42
    batch[row] = forged(batch[row], "rp_max.b:plus_1")
    c = run(monkeypatch, oracle_c, 1, batch, (mn[:n], mx[:n]), refused | {row}, size)
    assert c == {"failed_checks": 1, "segment_checks": 16, "jobs_again": 16}                       # only the forgery's segment, its refused rows included


def test_segments_around_the_tile_capacity(hip, oracle_c, monkeypatch, ranges, thresholds):
    """17 * jobs point terms of a segment one tile short of, at and beyond a whole number of tiles of k_bp_seg_points"""
    tenvs, ths = thresholds
    assert 17 * (TILE_JOBS - 1) == 17 * TILE_JOBS - 17 and len(tenvs) == 200 > 3 * (TILE_JOBS + 1)
    row = TILE_JOBS + 7                                                 # in the second segment at every size
    batch = with_rows(tenvs, {row: forged(tenvs[row], "rp.a:plus_1")})
    for size in (TILE_JOBS - 1, TILE_JOBS, TILE_JOBS + 1):              # one job per envelope: 63, 64, 65 jobs
        c = run(monkeypatch, oracle_c, 3, batch, (ths,), {row}, size)
        assert c == {"failed_checks": 1, "segment_checks": 4, "jobs_again": size}, size
    envs, mn, mx, _ = ranges
    n = 300
    row = 299                                                           # the partial last segment
    batch = with_rows(envs, {row: forged(envs[row], "rp_min.a:plus_1")})
    for size, segs, last in ((TILE_JOBS // 2, 10, 12), (TILE_JOBS // 2 + 1, 10, 3), (TILE_JOBS, 5, 44), (TILE_JOBS + 1, 5, 40)):      # 64, 66, 128, 130 jobs
        assert n - (segs - 1) * size == last
        c = run(monkeypatch, oracle_c, 1, batch, (mn, mx), {row}, size)
        assert c == {"failed_checks": 1, "segment_checks": segs, "jobs_again": 2 * last}, size
    row = 2 * TILE_JOBS + 5                                             # a whole segment of two tiles and of two tiles and two jobs
    batch = with_rows(envs, {row: forged(envs[row], "rp_max.L5:plus_B")})
    for size in (TILE_JOBS, TILE_JOBS + 1):
        c = run(monkeypatch, oracle_c, 1, batch, (mn, mx), {row}, size)
        assert c == {"failed_checks": 1, "segment_checks": 5, "jobs_again": 2 * size}, size


# ---------------------------------------------------------------------------------------------- threshold and consistency envelopes
def test_threshold_envelopes_one_job_each(hip, oracle_c, monkeypatch, thresholds):
    tenvs, ths = thresholds
    n, size = 197, 8                                                    # 24 segments of 8 and one of 5
    for rows in ({0}, {196}, {100, 103}, {7, 8}):
        batch = with_rows(tenvs[:n], {r: forged(tenvs[r], "rp.t_x:plus_1") for r in rows})
        c = run(monkeypatch, oracle_c, 3, batch, (ths[:n],), rows, size)
        assert c == expected([1] * n, size, rows), rows
    assert expected([1] * n, size, {196})["jobs_again"] == 5 and expected([1] * n, size, {7, 8})["jobs_again"] == 16


def test_consistency_envelopes_with_varying_job_counts(hip, oracle_c, monkeypatch):
    rng = np.random.default_rng(303)
    ks = [1, 3, 2, 1, 1, 8, 5, 1, 2, 2, 2, 2, 1, 1, 1, 1, 4, 1, 1, 6, 7, 3, 1, 2] * 3 + [5, 1]      # 74 envelopes: zero-job ones first and last in segments of 4, segment 3 without a job
    envs = random_consistency(ks, rng)
    jobs = [k - 1 for k in ks]
    n, size = len(ks), 4
    for rows in ({5}, {1, 2}, {72}, {19, 29}):
        batch = with_rows(envs, {r: forged(envs[r], "rp1.a:plus_1") for r in rows})
        c = run(monkeypatch, oracle_c, 6, batch, (), rows, size)
        assert c == expected(jobs, size, rows), rows
    assert expected(jobs, size, {5}) == {"failed_checks": 1, "segment_checks": 19, "jobs_again": 11}
    assert expected(jobs, size, {72})["jobs_again"] == 4                # the partial last segment
    # a bad digest on an envelope without a job: refused by the rule, and the check stands
    for row in (0, 3, 12):
        b = bytearray(envs[row]); b[-1] ^= 1
        c = run(monkeypatch, oracle_c, 6, with_rows(envs, {row: bytes(b)}), (), {row}, size)
        assert c == {"failed_checks": 0, "segment_checks": 0, "jobs_again": 0}
    b = bytearray(envs[12]); b[-1] ^= 1                                  # ... beside a forgery that reaches an equation
    c = run(monkeypatch, oracle_c, 6, with_rows(envs, {12: bytes(b), 6: forged(envs[6], "rp2.b:plus_1")}), (), {6, 12}, size)
    assert c == {"failed_checks": 1, "segment_checks": 19, "jobs_again": 11}


# ---------------------------------------------------------------------------------------------- the default path and the callers built on it
def test_the_default_path_at_2048_envelopes(hip, oracle_c, monkeypatch):
    import libzkp_amd.api as api
    rng = np.random.default_rng(304)
    n = 2048                                                            # 4096 jobs = RLC_MIN_JOBS: no switch at all
    envs, mn, mx = random_range(hip, n, 64, rng, same_bounds=True)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    row = 1337
    batch = with_rows(envs, {row: forged(envs[row], "rp_min.a:plus_1")})
    api.bp_verify_counters(reset=True)
    got = gpu_verify(1, batch, mn, mx)
    c = api.bp_verify_counters(reset=True)
    print(c)
    assert got == [i != row for i in range(n)]
    assert c["failed_checks"] == 1 and c["segment_checks"] >= 2 and 0 < c["jobs_again"] < 2 * n
    monkeypatch.setenv(NO, "1")
    assert gpu_verify(1, batch, mn, mx) == got
    for i in (0, row - 1, row, row + 1, n - 1):
        assert F.c_verify(oracle_c, batch[i], mn[i], mx[i]) == got[i]
    assert api.bp_verify_counters(reset=False) == ZERO


def test_the_mixed_verifier_inherits_the_path(hip, oracle_c, monkeypatch, ranges):
    import libzkp_amd as z
    import libzkp_amd.api as api
    envs, mn, mx, _ = ranges
    n, row = 96, 50
    batch = with_rows(envs[:n], {row: forged(envs[row], "rp_min.a:plus_1")})
    monkeypatch.setenv(MIN, "1"); monkeypatch.setenv(SEG, "8")
    api.bp_verify_counters(reset=True)
    got = z.verify_envelopes(batch)
    c = api.bp_verify_counters(reset=True)
    assert got == [i != row for i in range(n)]
    assert {k: c[k] for k in ("failed_checks", "segment_checks", "jobs_again")} == {"failed_checks": 1, "segment_checks": 12, "jobs_again": 16}
    monkeypatch.setenv(NO, "1")
    assert z.verify_envelopes(batch) == got
    for i in (row - 1, row, row + 1):
        assert F.c_verify(oracle_c, batch[i], mn[i], mx[i]) == got[i]


_TWO_SHARDS_CHILD = r"""
import json, os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
import bp_forge as F
from libzkp_amd import _native
L = _native.lib()
_native.init_devices([0, 0])                                  # two shards of the library on one GPU
rng = np.random.default_rng(99)
n = 96
assert L.zkp_hip_use_device(0) == 0
envs = z.prove_range_batch([int(x) for x in rng.integers(0, 1000, n)], [0] * n, [1000] * n, seeds=rng.bytes(32 * n))
out = {}
api.bp_verify_counters(reset=True)
os.environ["ZKP_HIP_BATCH_VERIFY_MIN"] = "1"
for shard, bad, size in ((0, 10, 8), (1, 90, 16)):
    assert L.zkp_hip_use_device(shard) == 0
    batch = list(envs)
    batch[bad] = [f for f in F.field_forgeries(envs[bad]) if f.name == "rp_min.a:plus_1"][0].env
    os.environ["ZKP_HIP_BP_LOCALISE_SEGMENT"] = str(size)
    got = z.verify_range_batch(batch, [0] * n, [1000] * n)
    del os.environ["ZKP_HIP_BP_LOCALISE_SEGMENT"]
    c = api.bp_verify_counters(reset=False); c.pop("ms")
    out["after_%d" % shard] = c
    os.environ["ZKP_HIP_NO_BATCH_VERIFY"] = "1"
    ref = z.verify_range_batch(batch, [0] * n, [1000] * n)
    del os.environ["ZKP_HIP_NO_BATCH_VERIFY"]
    out["same_%d" % shard] = got == ref
    out["false_%d" % shard] = [i for i, v in enumerate(got) if not v]
c = api.bp_verify_counters(reset=True); out["ms_positive"] = c.pop("ms") > 0
out["read_and_reset"] = c
out["then"] = api.bp_verify_counters(reset=False)
print(json.dumps(out))
"""


def test_two_shards_on_one_device_sum_their_counters():
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out = subprocess.run([sys.executable, "-c", _TWO_SHARDS_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    print(r)
    assert r["same_0"] and r["same_1"] and r["false_0"] == [10] and r["false_1"] == [90]
    assert r["after_0"] == {"failed_checks": 1, "segment_checks": 12, "jobs_again": 16}
    assert r["after_1"] == {"failed_checks": 2, "segment_checks": 18, "jobs_again": 48}          # shard 0's and shard 1's, summed
    assert r["read_and_reset"] == r["after_1"] and r["ms_positive"]
    assert r["then"] == ZERO
