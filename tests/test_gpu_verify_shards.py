"""One zkp_hip_verify_*_batch call spread over every registered shard (libzkp_amd/csrc/verify_shards.h, verify_fan_out in zkp_hip.hip), on
the MI355X with device 0 registered twice: the verdicts of a fanned-out call are the ones its envelopes deserve and the ones the same call
gives under ZKP_HIP_VERIFY_SHARDS=0, and the fan-out counter (api.verify_fanout_counters) says what was spread: slices and envelopes.
13 envelopes per scheme under ZKP_HIP_VERIFY_SHARD_MIN=4 make two uneven slices (7 and 6); the spoiled positions are 0, the last of slice
0, the first of slice 1 and the last.  Every scenario runs in a child process (a shard registration of its own); the children run once per
module and the tests read their results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ZKP_HIP_VERIFY_SHARDS", "ZKP_HIP_VERIFY_SHARD_MIN", "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_G16_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY",
            "ZKP_HIP_BP_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_BATCH_VERIFY_ONLY")
N, BAD = 13, (0, 6, 7, 12)
WANT = [i not in BAD for i in range(N)]
SCHEMES = ("range", "threshold", "consistency", "equality", "membership", "improvement")
ZERO = {"launches": 0, "point_adds": 0}

_COMMON = r"""
import json, os, sys, threading
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native
L = _native.lib()
GOLD = os.path.join(sys.argv[1], "tests", "golden")
N, BAD = 13, (0, 6, 7, 12)
rng = np.random.default_rng(1307)

def load_key(kind):
    api.install_proving_key(kind, open(os.path.join(GOLD, ("equality_mimc_pk.bin", "membership_mimc_pk.bin")[kind]), "rb").read())

def flip(b, off):
    b = bytearray(b); b[off] ^= 1
    return bytes(b)

def honest(scheme):
    # (envelopes, the other arguments of the scheme's verify call)
    if scheme == "range":                                        # the four widths in turn: envelopes of four lengths in one call
        envs = [z.prove_range_batch([50 + i], [10], [200], n_bits=(8, 16, 32, 64)[i % 4])[0] for i in range(N)]
        assert len({len(e) for e in envs}) == 4
        return envs, [[10] * N, [200] * N]
    if scheme == "threshold":
        lists = [[int(x) for x in rng.integers(0, 2**30, 1 + i % 4)] for i in range(N)]
        ths = [sum(v) - i for i, v in enumerate(lists)]
        return z.prove_threshold_batch(lists, ths), [ths]
    if scheme == "consistency":                                  # lists of 5, 1 and 2 values: 4, 0 and 1 jobs, so the weights differ and zero-job envelopes occur
        data = [sorted(int(x) for x in rng.integers(0, 2**50, (5, 1, 2)[i % 3])) for i in range(N)]
        return z.prove_consistency_batch(data), []
    if scheme == "equality":
        vals = [int(x) for x in rng.integers(0, 2**63, N)]
        return z.prove_equality_batch(vals, vals), []
    if scheme == "membership":
        sets = [[int(x) for x in rng.integers(1, 2**64, 1 + 5 * i, dtype=np.uint64)] for i in range(N)]
        return z.prove_membership_batch([s[i % len(s)] for i, s in enumerate(sets)], sets), []
    olds = [int(x) for x in rng.integers(0, 2**62, N)]
    return z.prove_improvement_batch(olds, [o + 1 + i for i, o in enumerate(olds)]), [olds]

def spoil(scheme, envs, args):
    # position 0: a flipped proof byte; 6: a truncated length; 7: a wrong bound / old value / commitment byte; 12: a flipped byte
    envs, args = list(envs), [list(a) for a in args]
    envs[0] = flip(envs[0], 100)
    envs[6] = envs[6][:-5]
    if scheme == "range":
        args[1][7] += 1
    elif scheme in ("threshold", "improvement"):
        args[0][7] += 1
    elif scheme == "consistency":
        envs[7] = flip(envs[7], 14 + 3)                          # a byte of the first commitment
    else:
        envs[7] = flip(envs[7], len(envs[7]) - 7)                # a byte of the envelope's commitment
    envs[12] = flip(envs[12], len(envs[12]) - 40)
    return envs, args

def call(scheme, envs, args):
    if scheme == "range": return z.verify_range_batch(envs, *args)
    if scheme == "threshold": return z.verify_threshold_batch(envs, *args)
    if scheme == "consistency": return z.verify_consistency_batch(envs)
    if scheme == "improvement": return z.verify_improvement_batch(envs, *args)
    return api._verify_snark_envelopes(0 if scheme == "equality" else 1, envs)

def counted(scheme, envs, args, **env):
    # (verdicts, what the fan-out counter saw of this one call) under the given switches
    os.environ.update(env)
    api.verify_fanout_counters(reset=True)
    try:
        got = [bool(x) for x in call(scheme, envs, args)]
    finally:
        c = api.verify_fanout_counters(reset=True)
        for k in env: del os.environ[k]
    assert api.verify_fanout_counters(reset=False) == {"launches": 0, "point_adds": 0, "ms": 0.0}
    return got, {"launches": c["launches"], "point_adds": c["point_adds"], "ms_positive": c["ms"] > 0}

out = {}
"""

_TWO_SHARDS = _COMMON + r"""
import bp_forge as F
_native.init_devices([0, 0])                                     # two shards of the library on one GPU
load_key(0); load_key(1)
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "4"
for scheme in ("range", "threshold", "consistency", "equality", "membership", "improvement"):
    envs, args = honest(scheme)
    r = {}
    r["honest"], r["honest_counters"] = counted(scheme, envs, args)
    envs, args = spoil(scheme, envs, args)
    r["fanned"], r["fanned_counters"] = counted(scheme, envs, args)
    r["one_shard"], r["one_shard_counters"] = counted(scheme, envs, args, ZKP_HIP_VERIFY_SHARDS="0")
    out[scheme] = r
    if scheme == "equality":
        eq_envs = envs
    if scheme == "range":
        rg = (envs, args)

# every slice makes its own batch check: 13 range envelopes of one width, 26 jobs, slices of 14 and 12 jobs against a threshold of 4
vals = [int(x) for x in rng.integers(1000, 2000, N)]
envs = z.prove_range_batch(vals, [1000] * N, [2000] * N)
args = [[1000] * N, [2000] * N]
b = {}
b["honest_check_only"], b["honest_check_only_counters"] = counted("range", envs, args, ZKP_HIP_BATCH_VERIFY_MIN="4", ZKP_HIP_BP_BATCH_VERIFY_ONLY="1")
forged = [f for f in F.forgeries(envs[3], donor=envs[4]) if f.stage == "equation"][0]
bad = envs[:3] + [forged.env] + envs[4:]
b["forged"], b["forged_counters"] = counted("range", bad, args, ZKP_HIP_BATCH_VERIFY_MIN="4")
b["forged_one_shard"], _ = counted("range", bad, args, ZKP_HIP_BATCH_VERIFY_MIN="4", ZKP_HIP_VERIFY_SHARDS="0")
try:
    counted("range", bad, args, ZKP_HIP_BATCH_VERIFY_MIN="4", ZKP_HIP_BP_BATCH_VERIFY_ONLY="1")
    b["forged_check_only_error"] = None
except _native.NativeError as e:
    b["forged_check_only_error"] = str(e)
# the slice without the forged envelope, as a call of its own: its check stands
b["other_slice_alone"], _ = counted("range", bad[7:], [a[7:] for a in args], ZKP_HIP_BATCH_VERIFY_MIN="4", ZKP_HIP_BP_BATCH_VERIFY_ONLY="1", ZKP_HIP_VERIFY_SHARDS="0")
out["batch_check"] = b

# calls that stay put.  Less than two minimum slices of work: 7 equality envelopes, 7 jobs < 2 * 4; 3 range envelopes, 6 jobs
s = {}
s["light_eq"], s["light_eq_counters"] = counted("equality", eq_envs[:7], [])
s["light_range"], s["light_range_counters"] = counted("range", rg[0][:3], [a[:3] for a in rg[1]])
s["light_range_4"], s["light_range_4_counters"] = counted("range", rg[0][:4], [a[:4] for a in rg[1]])          # 8 jobs: two slices of two envelopes
# a thread that has selected a shard does its own splitting: its call stays on shard 1
def on_shard_1():
    assert L.zkp_hip_use_device(1) == 0
    api.groth16_verify_counters(reset=True)
    s["selected"], s["selected_counters"] = counted("equality", eq_envs, [])
t = threading.Thread(target=on_shard_1); t.start(); t.join()
s["main_thread_after"], s["main_thread_after_counters"] = counted("equality", eq_envs, [])                      # the selection was the other thread's
out["stay"] = s
print(json.dumps(out))
"""

_ONE_SHARD = _COMMON + r"""
_native.init_devices([0])
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "4"
for scheme in ("range", "improvement"):
    envs, args = spoil(scheme, *honest(scheme))
    r = {}
    r["got"], r["counters"] = counted(scheme, envs, args)
    out[scheme] = r
print(json.dumps(out))
"""

# a key that one shard does not hold: possible only with a second HIP device (zkp_hip_init of a device without a shard adds one, keyless)
_KEY_ON_SOME_SHARDS = _COMMON + r"""
import torch
if torch.cuda.device_count() < 2:
    print(json.dumps({"devices": torch.cuda.device_count()})); sys.exit(0)
_native.init_devices([0, 0])
load_key(0)
_native.check(L.zkp_hip_init(1), "zkp_hip_init")                  # shard 2, on device 1, registered after the key was loaded
assert L.zkp_hip_device_count() == 3
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "4"
envs, args = spoil("equality", *honest("equality"))
out["devices"] = torch.cuda.device_count()
out["fanned"], out["fanned_counters"] = counted("equality", envs, args)
out["one_shard"], out["one_shard_counters"] = counted("equality", envs, args, ZKP_HIP_VERIFY_SHARDS="0")
out["three_slices_fit"], out["three_slices_fit_counters"] = counted("equality", envs, args, ZKP_HIP_VERIFY_SHARD_MIN="3")      # 13 / 3 = 4 slices wanted, two shards hold the key
print(json.dumps(out))
"""


def _child(script):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    out = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def two_shards():
    r = _child(_TWO_SHARDS)
    print(json.dumps(r))
    return r


def slices(c):
    return {"launches": c["launches"], "point_adds": c["point_adds"]}


@pytest.mark.parametrize("scheme", SCHEMES)
def test_a_fanned_out_call_gives_the_verdicts_of_one_shard_and_counts_its_slices(two_shards, scheme):
    r = two_shards[scheme]
    assert r["honest"] == [True] * N and slices(r["honest_counters"]) == {"launches": 2, "point_adds": N}
    assert r["fanned"] == WANT                                                         # by construction
    assert r["fanned"] == r["one_shard"]                                               # and what the same call gives on one shard
    assert slices(r["fanned_counters"]) == {"launches": 2, "point_adds": N} and r["fanned_counters"]["ms_positive"]
    assert slices(r["one_shard_counters"]) == ZERO and not r["one_shard_counters"]["ms_positive"]


def test_every_slice_makes_its_own_batch_check(two_shards):
    b = two_shards["batch_check"]
    # all honest: with the per-job pass switched off the call succeeds, so both slices were accepted as batches
    assert b["honest_check_only"] == [True] * N and slices(b["honest_check_only_counters"]) == {"launches": 2, "point_adds": N}
    # one forged envelope (row 3, refused by the equation alone): its slice falls back to the per-job pass, the verdicts are the per-job ones
    assert b["forged"] == [i != 3 for i in range(N)] == b["forged_one_shard"] and slices(b["forged_counters"]) == {"launches": 2, "point_adds": N}
    # ... and that was a fallback of slice 0 only: with the per-job pass off the call fails with that slice's message, slice 1 stands alone
    assert b["forged_check_only_error"] and "the batch check did not stand" in b["forged_check_only_error"]
    assert b["other_slice_alone"] == [True] * 6


def test_a_call_below_two_minimum_slices_stays_put(two_shards):
    s = two_shards["stay"]
    assert s["light_eq"] == WANT[:7] and slices(s["light_eq_counters"]) == ZERO
    assert s["light_range"] == WANT[:3] and slices(s["light_range_counters"]) == ZERO
    assert s["light_range_4"] == WANT[:4] and slices(s["light_range_4_counters"]) == {"launches": 2, "point_adds": 4}          # the threshold between the two paths


def test_a_thread_that_selected_a_shard_stays_on_it(two_shards):
    s = two_shards["stay"]
    assert s["selected"] == WANT and slices(s["selected_counters"]) == ZERO
    assert s["main_thread_after"] == WANT and slices(s["main_thread_after_counters"]) == {"launches": 2, "point_adds": N}


def test_one_registered_shard_stays_put():
    r = _child(_ONE_SHARD)
    for scheme in ("range", "improvement"):
        assert r[scheme]["got"] == WANT and slices(r[scheme]["counters"]) == ZERO


def test_groth16_runs_on_the_shards_that_hold_the_key():
    r = _child(_KEY_ON_SOME_SHARDS)
    if r["devices"] < 2:
        pytest.skip("needs a second HIP device: on one device every registered shard gets every key, a keyless shard cannot be made through the C ABI")
    assert r["fanned"] == WANT == r["one_shard"] == r["three_slices_fit"]
    assert slices(r["fanned_counters"]) == {"launches": 2, "point_adds": N} and slices(r["one_shard_counters"]) == ZERO
    assert slices(r["three_slices_fit_counters"]) == {"launches": 2, "point_adds": N}


def test_the_python_name_is_exported():
    import libzkp_amd as z
    import libzkp_amd.api as api
    from libzkp_amd import _native
    assert z.verify_fanout_counters is api.verify_fanout_counters and "verify_fanout_counters" in z.__all__ and _native.COUNTER_VERIFY_FANOUT == 5
