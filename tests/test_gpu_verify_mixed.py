"""One verify call for a mixed envelope list (include/libzkp_hip_verify.h; libzkp_amd/csrc/venv_steps.h, venv_impl.inc) on the MI355X.

Reference verdicts never come from the call under test: they come from the six public per-scheme verify_*_batch calls behind a copy of the
bucketing that composite.verify_proof_cryptographic_batch did in Python before the mixed call existed (`reference_verdicts` below), each
envelope verified against its own parameters.  Envelopes come from process_ops under fixed seeds (the 8-bit range envelopes, which
process_ops cannot make, from prove_range_batch under fixed seeds).  Every scenario runs in a child process (its own shard registration
and switches); the children run once per module and the tests read their results."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("ZKP_HIP_VERIFY_SHARDS", "ZKP_HIP_VERIFY_SHARD_MIN", "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_G16_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY",
            "ZKP_HIP_BP_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_VERIFY_VM")

_COMMON = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native, composite
L = _native.lib()
GOLD = os.path.join(sys.argv[1], "tests", "golden")
VP = ctypes.c_void_p

def P(a):
    return a.ctypes.data_as(VP)

def load_keys():
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        api.install_proving_key(kind, open(os.path.join(GOLD, name), "rb").read())

def seeds_for(n, salt):
    return bytes(np.random.default_rng(1000 + salt).integers(0, 256, 32 * n, dtype=np.uint8))

# ---- the reference: today's Python bucketing (composite.verify_proof_cryptographic_batch before the mixed call) over the PUBLIC per-scheme calls
def reference_verdicts(envelopes, expect=None):
    out = [False] * len(envelopes)
    groups = {1: [], 2: [], 3: [], 4: [], 5: [], 6: []}
    for i, env in enumerate(envelopes):
        try:
            version, scheme, payload, commitment = composite.parse_proof(env)
        except composite.ProofFormatError:
            continue
        if version != composite.PROOF_VERSION:
            continue
        if expect is not None and expect[i] not in (0, scheme):          # verify_single_proof: the type must match (performance.rs:282-286)
            continue
        if scheme == 2 and len(commitment) == 32:
            groups[2].append((i, env))
        elif scheme == 4 and len(commitment) == 32 and len(payload) > 4:
            groups[4].append((i, env))
        elif scheme == 1 and len(payload) >= 20 and len(commitment) == 32:
            mn, mx = int.from_bytes(payload[:8], "little"), int.from_bytes(payload[8:16], "little")
            if mn <= mx:
                groups[1].append((i, env, mn, mx))
        elif scheme == 3 and len(payload) >= 12 and len(commitment) == 32:
            groups[3].append((i, env, int.from_bytes(payload[:8], "little")))
        elif scheme == 5 and len(payload) >= 16 and len(commitment) == 32:
            groups[5].append((i, env, int.from_bytes(payload[:8], "little")))
        elif scheme == 6:
            groups[6].append((i, env))
    def put(group, verdicts):
        for (i, *_), ok in zip(group, verdicts):
            out[i] = bool(ok)
    if groups[1]:
        put(groups[1], z.verify_range_batch([g[1] for g in groups[1]], [g[2] for g in groups[1]], [g[3] for g in groups[1]]))
    if groups[2]:          # the envelope's own commitment: the pairing check under it is all that is asked
        put(groups[2], z.verify_equality_with_commitment_batch([g[1] for g in groups[2]], [g[1][-32:] for g in groups[2]]))
    if groups[4]:          # the envelope's own embedded set
        sets = []
        for _, env in groups[4]:
            cnt = int.from_bytes(env[10:14], "little")
            sets.append([int.from_bytes(env[14 + 8 * k:22 + 8 * k], "little") for k in range(cnt)] if len(env) == 10 + 4 + 8 * cnt + 256 + 32 else [])
        put(groups[4], z.verify_membership_batch([g[1] for g in groups[4]], sets))
    if groups[3]:
        put(groups[3], z.verify_threshold_batch([g[1] for g in groups[3]], [g[2] for g in groups[3]]))
    if groups[5]:
        put(groups[5], z.verify_improvement_batch([g[1] for g in groups[5]], [g[2] for g in groups[5]]))
    if groups[6]:
        put(groups[6], z.verify_consistency_batch([g[1] for g in groups[6]]))
    return out

def mixed_ops(counts, salt):
    # interleaved ops: counts = (range64, threshold, equality, membership, improvement, consistency); sets of 1, 5, 64; lists of 2 and 5
    rng = np.random.default_rng(salt)
    per = {
        "range": [("range", int(v), 1000, 1000 + 2**20) for v in rng.integers(1000, 1000 + 2**20, counts[0])],
        "threshold": [],
        "equality": [("equality", int(v), int(v)) for v in rng.integers(0, 2**63, counts[2])],
        "membership": [],
        "improvement": [("improvement", int(o), int(o) + 1 + i) for i, o in enumerate(rng.integers(0, 2**62, counts[4]))],
        "consistency": [("consistency", sorted(int(x) for x in rng.integers(0, 2**50, (2, 5)[i % 2]))) for i in range(counts[5])],
    }
    for i in range(counts[1]):
        vals = [int(x) for x in rng.integers(0, 2**30, 1 + i % 4)]
        per["threshold"].append(("threshold", vals, max(sum(vals) - i, 0)))
    for i in range(counts[3]):
        s = [int(x) for x in rng.choice(2**32, (1, 5, 64)[i % 3], replace=False)]
        per["membership"].append(("membership", s[i % len(s)], s))
    ops, queues = [], [list(v) for v in per.values()]
    while any(queues):
        for q in queues:
            if q:
                ops.append(q.pop(0))
    return ops

def base_list():
    # about 40 interleaved envelopes: range at 64 and 8 bits, threshold, equality, membership (sets of 1, 5, 64), improvement, consistency (k = 2, 5)
    ops = mixed_ops((6, 5, 6, 6, 5, 6), 7)
    envs = api.process_ops(ops, seeds_for(len(ops), 1))
    narrow = z.prove_range_batch([3, 77, 200, 255], [0, 50, 100, 250], [255, 100, 300, 255], seeds=seeds_for(4, 2), n_bits=8)
    assert len(narrow[0]) < len(envs[0])
    for k, e in enumerate(narrow):
        envs.insert(3 + 9 * k, e)
    return envs

def flip(b, off, bit=0):
    b = bytearray(b); b[off] ^= 1 << bit
    return bytes(b)

def first(envs, scheme, pred=lambda e: True):
    return next(e for e in envs if e[1] == scheme and pred(e))

def header(scheme, payload, commitment, version=2):
    return bytes([version, scheme]) + len(payload).to_bytes(4, "little") + len(commitment).to_bytes(4, "little") + payload + commitment

def mixed_counters():
    c = api.verify_mixed_counters(reset=True)
    return {"launches": c["launches"], "point_adds": c["point_adds"], "ms_positive": c["ms"] > 0}

out = {}
"""

_MAIN = _COMMON + r"""
import torch
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
# ---- 7c: an equality envelope while no key is loaded: the per-scheme call's error (before any key exists in this process)
eq_like = header(2, bytes(256), bytes(32))
blob = np.frombuffer(eq_like, dtype=np.uint8); off = np.array([0, 298], dtype=np.uint64); ok1 = np.zeros(1, dtype=np.uint8); lens = np.array([298], dtype=np.uint32)
rc_mixed = L.zkp_hip_verify_envelopes(1, P(blob), P(off), None, P(ok1)); msg_mixed = _native.last_error()
rc_single = L.zkp_hip_verify_equality_batch(1, P(blob), 298, P(lens), P(ok1)); msg_single = _native.last_error()
out["no_key"] = {"mixed": [rc_mixed, msg_mixed], "single": [rc_single, msg_single]}
# a list whose only Groth16-looking envelope is rejected by the classification needs no key
junk_eq = header(2, bytes(256), bytes(31))
blob = np.frombuffer(junk_eq, dtype=np.uint8); off = np.array([0, len(junk_eq)], dtype=np.uint64); ok1[0] = 9
out["no_key_rejected"] = [L.zkp_hip_verify_envelopes(1, P(blob), P(off), None, P(ok1)), int(ok1[0])]

load_keys()
base = base_list()
schemes = [e[1] for e in base]
out["base_schemes"] = schemes
ref_base = reference_verdicts(base)
out["ref_base"] = ref_base

# ---- 1: all valid, with expect NULL, all 0, and the true schemes
api.verify_mixed_counters(reset=True)
out["valid_null"] = z.verify_envelopes(base)
out["valid_null_counters"] = mixed_counters()
out["valid_any"] = z.verify_envelopes(base, [0] * len(base))
out["valid_true"] = z.verify_envelopes(base, schemes)

# ---- 2: damage; every damaged envelope stands between two good ones
rg, th, eq, im = first(base, 1, lambda e: len(e) == 1478), first(base, 3), first(base, 2), first(base, 5)
me5, me64 = first(base, 4, lambda e: e[10] == 5), first(base, 4, lambda e: e[10] == 64)
co2 = first(base, 6, lambda e: e[10] == 2)
rnd = np.random.default_rng(99)
def filler(n):
    return bytes(rnd.integers(0, 256, n, dtype=np.uint8))
damaged = {
    "flip_range": flip(rg, 100), "flip_threshold": flip(th, 100), "flip_equality": flip(eq, 100), "flip_membership": flip(me5, 100),
    "flip_improvement": flip(im, 100), "flip_consistency": flip(co2, 150),
    "version_1": bytes([1]) + rg[1:], "scheme_0": rg[:1] + bytes([0]) + rg[2:], "scheme_7": eq[:1] + bytes([7]) + eq[2:],
    "length_plus_1": th + b"\0", "length_minus_1": eq[:-1],
    "commitment_31": header(1, rg[10:-32], rg[-32:-1]),
    "nine_bytes": rg[:9], "empty": b"",
    "range_min_gt_max": rg[:10] + (int.from_bytes(rg[18:26], "little") + 1).to_bytes(8, "little") + rg[18:],
    "range_payload_19": header(1, rg[10:29], rg[-32:]),
    "membership_count_0": me5[:10] + (0).to_bytes(4, "little") + me5[14:],
    "membership_count_65": me64[:10] + (65).to_bytes(4, "little") + me64[14:],
    "long_range": header(1, rg[10:26] + filler(4200), rg[-32:]), "long_threshold": header(3, th[10:18] + filler(4200), th[-32:]),
    "long_equality": header(2, filler(4200), eq[-32:]), "long_membership": header(4, me5[10:54] + filler(4200), me5[-32:]),
    "long_improvement": header(5, im[10:26] + filler(8300), im[-32:]),
    "long_consistency": co2 + bytes((1 << 20) + 1 - len(co2)),
    "range_expected_as_equality": rg, "expect_9": th,
}
assert len(damaged["range_min_gt_max"]) == 1478 and len(damaged["long_consistency"]) == (1 << 20) + 1
goods = [e for e in base]
lst, expect, where = [goods[0]], [0], {}
for k, (name, env) in enumerate(damaged.items()):
    where[name] = len(lst)
    lst.append(env); expect.append(2 if name == "range_expected_as_equality" else 9 if name == "expect_9" else 0 if k % 2 else env[1] if len(env) > 1 and 1 <= env[1] <= 6 else 0)
    g = goods[(k + 1) % len(goods)]
    lst.append(g); expect.append(g[1] if k % 3 else 0)
out["damage_where"] = where
out["damage_ref"] = reference_verdicts(lst, expect)
out["damage_got"] = z.verify_envelopes(lst, expect)
out["damage_ref_no_expect"] = reference_verdicts(lst)
out["damage_got_no_expect"] = z.verify_envelopes(lst)

# ---- 3: alignment: the list behind 0..15 one-byte envelopes
out["aligned"] = [z.verify_envelopes([b"\x02"] * k + base) for k in range(16)]

# ---- 7a / 7b: n = 0; a list of rejected envelopes only runs no scheme pass
out["empty_list"] = z.verify_envelopes([])
ok0 = np.zeros(1, dtype=np.uint8)
out["n0_rc"] = [L.zkp_hip_verify_envelopes(0, None, None, None, None), L.zkp_hip_verify_envelopes_device(0, None, None, None, None)]
api.verify_mixed_counters(reset=True)
rejected = [damaged[k] for k in ("version_1", "scheme_0", "scheme_7", "length_plus_1", "commitment_31", "nine_bytes", "empty", "range_min_gt_max", "membership_count_0")]
out["rejected_only"] = z.verify_envelopes(rejected)
out["rejected_only_counters"] = mixed_counters()

# ---- 8: the Python front ends go through the mixed call
names = {v: k for k, v in composite.SCHEME_BY_NAME.items()}
api.verify_mixed_counters(reset=True)
out["parallel"] = z.verify_proofs_parallel([(e, names[e[1]]) for e in base[:12]] + [(base[0], "nope"), (b"junk", "range"), (flip(rg, 700), "range"), (rg, "threshold")])
out["parallel_counters"] = mixed_counters()
out["composite"] = [z.verify_composite_proof(z.create_composite_proof(base[:9])), z.verify_composite_proof(z.create_composite_proof(base[:4] + [flip(eq, 100)]))]
out["composite_counters"] = mixed_counters()

# ---- 5: the device form on what zkp_hip_batch_device_results left in torch buffers
from libzkp_amd import workloads as wl
ops12 = mixed_ops((2, 2, 2, 2, 2, 2), 21)
assert len(ops12) == 12
code = {"range": 1, "equality": 2, "threshold": 3, "membership": 4, "improvement": 5, "consistency": 6}
arr = np.zeros(12, dtype=wl.OP_DTYPE); lists = []
for i, o in enumerate(ops12):
    arr["kind"][i] = code[o[0]]
    if o[0] == "range": arr["a"][i], arr["b"][i], arr["c"][i] = o[1], o[2], o[3]
    elif o[0] in ("equality", "improvement"): arr["a"][i], arr["b"][i] = o[1], o[2]
    elif o[0] == "threshold": arr["a"][i], arr["count"][i], arr["list_off"][i] = o[2], len(o[1]), len(lists); lists += o[1]
    elif o[0] == "membership": arr["a"][i], arr["count"][i], arr["list_off"][i] = o[1], len(o[2]), len(lists); lists += o[2]
    else: arr["count"][i], arr["list_off"][i] = len(o[1]), len(lists); lists += o[1]
la = np.array(lists, dtype=np.uint64); sd = np.frombuffer(seeds_for(12, 3), dtype=np.uint8)
B = VP()
_native.check(L.zkp_hip_batch_stage(12, P(arr), P(la), P(sd), ctypes.byref(B)), "zkp_hip_batch_stage")
_native.check(L.zkp_hip_batch_prove(B), "zkp_hip_batch_prove")
cap = int(L.zkp_hip_batch_max_bytes(B))
d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda"); d_off = torch.zeros(13, dtype=torch.int64, device="cuda"); d_ok = torch.full((12,), 9, dtype=torch.uint8, device="cuda")
nops = ctypes.c_uint64()
_native.check(L.zkp_hip_batch_device_results(B, 0, VP(d_out.data_ptr()), cap, VP(d_off.data_ptr()), ctypes.byref(nops), None), "zkp_hip_batch_device_results")
L.zkp_hip_batch_free(B)
torch.cuda.synchronize()
dev = {"nops": int(nops.value)}
dev["rc"] = L.zkp_hip_verify_envelopes_device(12, VP(d_out.data_ptr()), VP(d_off.data_ptr()), None, VP(d_ok.data_ptr()))
dev["ok"] = d_ok.cpu().tolist()
offs = d_off.cpu().tolist()
d_out[offs[7] + 100] ^= 1                                   # one byte of op 7, flipped where it lies
torch.cuda.synchronize()
d_expect = torch.tensor([int(k) for k in arr["kind"]], dtype=torch.uint8, device="cuda")
dev["rc_flipped"] = L.zkp_hip_verify_envelopes_device(12, VP(d_out.data_ptr()), VP(d_off.data_ptr()), VP(d_expect.data_ptr()), VP(d_ok.data_ptr()))
dev["ok_flipped"] = d_ok.cpu().tolist()
out["device"] = dev
print(json.dumps(out))
"""

_BATCH_CHECKS = _COMMON + r"""
# started with ZKP_HIP_BATCH_VERIFY_MIN=8 and ZKP_HIP_G16_BATCH_VERIFY_MIN=8: every scheme of a 64-envelope list takes its batch check
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
load_keys()
ops = mixed_ops((16, 8, 12, 10, 8, 10), 33)
assert len(ops) == 64
clean = api.process_ops(ops, seeds_for(64, 4))
bad = list(clean)
i_range = next(i for i, e in enumerate(bad) if e[1] == 1 and i > 20); i_eq = next(i for i, e in enumerate(bad) if e[1] == 2 and i > 30)
bad[i_range] = flip(bad[i_range], 700); bad[i_eq] = flip(bad[i_eq], 100)
out["bad_at"] = [i_range, i_eq]
out["ref_bad"] = reference_verdicts(bad)
out["got_bad"] = z.verify_envelopes(bad)
os.environ["ZKP_HIP_BP_BATCH_VERIFY_ONLY"] = "1"; os.environ["ZKP_HIP_G16_BATCH_VERIFY_ONLY"] = "1"
out["got_clean_checks_only"] = z.verify_envelopes(clean)                              # no per-envelope pass behind a check that stands
try:
    z.verify_envelopes(bad)
    out["bad_checks_only_error"] = None
except _native.NativeError as e:
    out["bad_checks_only_error"] = str(e)
print(json.dumps(out))
"""

_TWO_SHARDS = _COMMON + r"""
_native.init_devices([0, 0])                                     # two shards of the library on one GPU
load_keys()
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "8"
base = base_list()
lst = (base + base[:10])[:48]
assert len(lst) == 48
bad = (0, 24, 47)
for i in bad:
    lst[i] = flip(lst[i], 150 if lst[i][1] == 6 else 100)
out["bad"] = list(bad)
out["ref"] = reference_verdicts(lst)
def counted(**env):
    os.environ.update(env)
    api.verify_fanout_counters(reset=True); api.verify_mixed_counters(reset=True)
    try:
        got = z.verify_envelopes(lst)
    finally:
        f = api.verify_fanout_counters(reset=True); m = api.verify_mixed_counters(reset=True)
        for k in env: del os.environ[k]
    return got, {"launches": f["launches"], "point_adds": f["point_adds"]}, {"launches": m["launches"], "point_adds": m["point_adds"]}
out["fanned"], out["fanned_fanout"], out["fanned_mixed"] = counted()
out["one_shard"], out["one_shard_fanout"], out["one_shard_mixed"] = counted(ZKP_HIP_VERIFY_SHARDS="0")
print(json.dumps(out))
"""


def _child(script, **extra_env):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra_env)
    r = subprocess.run([sys.executable, "-c", script, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def main():
    return _child(_MAIN)


def test_all_valid_under_every_form_of_expect(main):
    n = len(main["base_schemes"])
    assert 36 <= n <= 44 and sorted(set(main["base_schemes"])) == [1, 2, 3, 4, 5, 6]
    assert main["ref_base"] == [True] * n                                               # the per-scheme calls accept every envelope
    assert main["valid_null"] == [True] * n and main["valid_any"] == [True] * n and main["valid_true"] == [True] * n
    assert main["valid_null_counters"] == {"launches": 6, "point_adds": n, "ms_positive": True}


def test_damaged_envelopes_get_the_reference_verdicts_and_neighbours_stay_accepted(main):
    got, ref, where = main["damage_got"], main["damage_ref"], main["damage_where"]
    print(json.dumps({k: got[v] for k, v in where.items()}))
    assert got == ref and main["damage_got_no_expect"] == main["damage_ref_no_expect"]
    assert len(where) == 26
    for name, at in where.items():
        assert got[at] is False, name                                                   # (what the reference says too: see above)
        assert got[at - 1] is True and got[at + 1] is True, name
    plain = main["damage_got_no_expect"]
    assert plain[where["range_expected_as_equality"]] is True and plain[where["expect_9"]] is True      # the envelopes themselves are valid


def test_every_source_alignment(main):
    n = len(main["base_schemes"])
    for k, got in enumerate(main["aligned"]):
        assert got == [False] * k + main["ref_base"], k
    assert len(main["aligned"]) == 16 and len(main["aligned"][15]) == n + 15


def test_degenerate_calls(main):
    assert main["empty_list"] == [] and main["n0_rc"] == [0, 0]
    assert main["rejected_only"] == [False] * 9
    assert main["rejected_only_counters"] == {"launches": 0, "point_adds": 0, "ms_positive": True}
    mixed, single = main["no_key"]["mixed"], main["no_key"]["single"]
    assert mixed[0] == single[0] == -3 and mixed[1] == single[1] and "no (usable) key loaded" in mixed[1]
    assert main["no_key_rejected"] == [0, 0]


def test_python_front_ends_go_through_the_mixed_call(main):
    assert main["parallel"] == [True] * 12 + [False] * 4
    assert main["parallel_counters"]["launches"] >= 1 and main["parallel_counters"]["point_adds"] == 13      # 12 valid + the bit-flipped range envelope
    assert main["composite"] == [True, False]
    assert main["composite_counters"]["launches"] >= 2 and main["composite_counters"]["point_adds"] == 9 + 5


def test_device_form(main):
    d = main["device"]
    assert d["nops"] == 12 and d["rc"] == 0 and d["ok"] == [1] * 12
    assert d["rc_flipped"] == 0 and d["ok_flipped"] == [0 if i == 7 else 1 for i in range(12)]


def test_batch_check_paths():
    r = _child(_BATCH_CHECKS, ZKP_HIP_BATCH_VERIFY_MIN="8", ZKP_HIP_G16_BATCH_VERIFY_MIN="8")
    want = [i not in r["bad_at"] for i in range(64)]
    assert r["ref_bad"] == want and r["got_bad"] == want
    assert r["got_clean_checks_only"] == [True] * 64
    assert r["bad_checks_only_error"] and "the batch check did not stand" in r["bad_checks_only_error"]


def test_two_shards_on_one_gpu():
    r = _child(_TWO_SHARDS)
    want = [i not in r["bad"] for i in range(48)]
    assert r["ref"] == want and r["fanned"] == want and r["one_shard"] == want
    assert r["fanned_fanout"] == {"launches": 2, "point_adds": 48}
    assert r["one_shard_fanout"] == {"launches": 0, "point_adds": 0}
    assert r["fanned_mixed"]["point_adds"] == 48 == r["one_shard_mixed"]["point_adds"]
    assert r["one_shard_mixed"]["launches"] == 6 and 6 < r["fanned_mixed"]["launches"] <= 12


def test_the_python_names_are_exported():
    import libzkp_amd as z
    import libzkp_amd.api as api
    from libzkp_amd import _native
    assert z.verify_envelopes is api.verify_envelopes and z.verify_mixed_counters is api.verify_mixed_counters
    assert "verify_envelopes" in z.__all__ and "verify_mixed_counters" in z.__all__ and _native.COUNTER_VERIFY_MIXED == 6
