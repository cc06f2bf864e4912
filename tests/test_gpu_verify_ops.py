"""Envelopes against the caller's statements in one call (include/libzkp_hip_statements.h; libzkp_amd/csrc/vst_steps.h, vst_impl.inc) on
the MI355X.

Expected verdicts never come from the call under test: they come from the public per-scheme functions WITH the statement
(`reference_verdicts` below) -- verify_range_batch(p, mins, maxs), verify_threshold_batch, verify_improvement_batch,
verify_consistency_batch, verify_membership_batch(p, sets), and verify_equality_with_commitment_batch(p, [snark_commit_value(v)]) together
with val1 == val2.  Envelopes come from process_ops under fixed seeds.  Every scenario runs in a child process (its own shard registration
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
ACCEPTED, ENVELOPE, STATEMENT, PROOF = 0, 1, 2, 3

_COMMON = r"""
import ctypes, json, os, sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native
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

# ---- the reference: the PUBLIC per-scheme calls, each with the statement of its op
def reference_verdicts(ops, envs):
    out = [False] * len(ops)
    groups = {}
    for i, o in enumerate(ops):
        groups.setdefault(o[0], []).append(i)
    def put(idx, verdicts):
        for i, ok in zip(idx, verdicts):
            out[i] = bool(ok)
    for kind, idx in groups.items():
        p = [envs[i] for i in idx]
        if kind == "range":
            put(idx, [a and ops[i][2] <= ops[i][3] for a, i in zip(z.verify_range_batch(p, [ops[i][2] for i in idx], [ops[i][3] for i in idx]), idx)])
        elif kind == "threshold":
            put(idx, z.verify_threshold_batch(p, [ops[i][2] for i in idx]))
        elif kind == "improvement":
            put(idx, z.verify_improvement_batch(p, [ops[i][1] for i in idx]))
        elif kind == "consistency":
            put(idx, z.verify_consistency_batch(p))
        elif kind == "membership":
            put(idx, z.verify_membership_batch(p, [ops[i][2] for i in idx]))
        elif kind == "equality":
            got = z.verify_equality_with_commitment_batch(p, [z.snark_commit_value(ops[i][1]) for i in idx])
            put(idx, [a and ops[i][1] == ops[i][2] for a, i in zip(got, idx)])
        elif kind == "equality_commitment":
            put(idx, z.verify_equality_with_commitment_batch(p, [ops[i][1] for i in idx]))
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

REPEATED = [2**40 + 5] * 2 + [2**40 + 9] + [7000 + k for k in range(61)]          # a 64-set with a repeated element (membership_ok admits one)
def base_ops():
    # the interleaved list of the mixed verifier's tests, a second range op with other bounds, and a membership op over REPEATED
    return mixed_ops((6, 5, 6, 6, 5, 6), 7) + [("range", 77, 50, 100), ("membership", 2**40 + 9, list(REPEATED))]

def at(ops, kind, pred=lambda o: True, skip=0):
    return [i for i, o in enumerate(ops) if o[0] == kind and pred(o)][skip]

def wrong_statements(ops):
    # one wrong statement of each kind on a copy of ops; (ops, {index: expected accepted?})
    ops = list(ops); touched = {}
    r0, r1 = at(ops, "range", lambda o: o[2] == 1000), at(ops, "range", lambda o: o[2] == 50)
    ops[r0], ops[r1] = ops[r1], ops[r0]; touched[r0] = touched[r1] = False                      # two range ops with different bounds swapped
    t = at(ops, "threshold"); ops[t] = ("threshold", ops[t][1], ops[t][2] + 1); touched[t] = False
    i = at(ops, "improvement"); ops[i] = ("improvement", ops[i][1] + 1, ops[i][2]); touched[i] = False
    e = at(ops, "equality"); v = ops[e][1]; ops[e] = ("equality", v + 1, v + 1); touched[e] = False
    e = at(ops, "equality", skip=1); v = ops[e][1]; ops[e] = ("equality", v, v + 1); touched[e] = False
    e = at(ops, "equality", skip=2); ops[e] = ("equality_commitment", z.snark_commit_value(ops[e][1])); touched[e] = True
    e = at(ops, "equality", skip=2); c = bytearray(z.snark_commit_value(ops[e][1])); c[31] ^= 0x10; ops[e] = ("equality_commitment", bytes(c)); touched[e] = False
    m = at(ops, "membership", lambda o: len(o[2]) == 5); ops[m] = ("membership", ops[m][1], list(reversed(ops[m][2]))); touched[m] = True
    m = at(ops, "membership", lambda o: len(o[2]) == 5, skip=1); s = list(ops[m][2]); s[3] ^= 1 << 33; ops[m] = ("membership", ops[m][1], s); touched[m] = False
    m = at(ops, "membership", lambda o: o[2] == REPEATED)
    ops[m] = ("membership", ops[m][1], [2**40 + 5] + [2**40 + 9] * 2 + REPEATED[3:]); touched[m] = False      # two multiplicities exchanged
    m = at(ops, "membership", lambda o: len(o[2]) == 64 and o[2] != REPEATED and len(set(o[2])) == 64)
    ops[m] = ("membership", ops[m][1], ops[m][2][32:] + ops[m][2][:32]); touched[m] = True
    return ops, touched

def flip(b, off, bit=0):
    b = bytearray(b); b[off] ^= 1 << bit
    return bytes(b)

def flip_proof(env):
    # a byte inside the scheme's proof, outside everything a statement is compared with
    return flip(env, {4: len(env) - 100, 6: 150}.get(env[1], 100))

def counters():
    c = api.verify_statements_counters(reset=True)
    c["ms_positive"] = c.pop("ms") > 0
    return c

def split(pairs):
    return [bool(a) for a, _ in pairs], [int(w) for _, w in pairs]

def raw_call(ops, envs, device=False):
    # (rc, ok, why) of the C call itself, host or device form
    n = len(ops)
    arr, lists, _ = api.statement_ops(ops)
    la = np.array(lists if lists else [0], dtype=np.uint64)
    blob = np.frombuffer(b"".join(envs) + b"\0", dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(e) for e in envs]))).astype(np.uint64)
    ok, why = np.full(n, 9, dtype=np.uint8), np.full(n, 9, dtype=np.uint8)
    if not device:
        rc = L.zkp_stmt_verify(n, ctypes.byref(arr), P(la), len(lists), P(blob), P(off), P(ok), P(why))
        return rc, ok.tolist(), why.tolist()
    import torch
    up = lambda a: torch.from_numpy(np.frombuffer(bytes(a), dtype=np.uint8).copy()).cuda()
    d_ops, d_lists, d_blob, d_off = up(arr), up(la.tobytes()), up(blob.tobytes()), up(off.tobytes())
    d_ok, d_why = torch.full((n,), 9, dtype=torch.uint8, device="cuda"), torch.full((n,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.zkp_stmt_verify_device(n, VP(d_ops.data_ptr()), VP(d_lists.data_ptr()), len(lists), VP(d_blob.data_ptr()), VP(d_off.data_ptr()), VP(d_ok.data_ptr()), VP(d_why.data_ptr()))
    return rc, d_ok.cpu().tolist(), d_why.cpu().tolist()

out = {}
"""

_MAIN = _COMMON + r"""
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
# ---- before any key exists in this process: only an equality envelope that is LEFT after the envelope and statement steps needs the key
v = 31337
def eq_like(c):
    return bytes([2, 2]) + (256).to_bytes(4, "little") + (32).to_bytes(4, "little") + bytes(256) + c
from oracle.py import groth16
cm = groth16.commit_value_snark(v)
out["no_key"] = {
    "other_kind": raw_call([("range", 1, 0, 9)], [eq_like(cm)]),
    "wrong_statement": raw_call([("equality", v + 1, v + 1)], [eq_like(cm)]),
    "live": raw_call([("equality", v, v)], [eq_like(cm)])[0], "live_msg": _native.last_error(),
}
load_keys()
ops = base_ops()
envs = api.process_ops(ops, seeds_for(len(ops), 1))
out["kinds"] = [o[0] for o in ops]
out["ref_base"] = reference_verdicts(ops, envs)

# ---- round trip
api.verify_statements_counters(reset=True)
out["base"] = split(z.verify_ops(ops, envs, reasons=True))
out["base_counters"] = counters()
out["base_plain"] = z.verify_ops(ops, envs)
out["empty"] = z.verify_ops([], [])

# ---- the mixed verifier before and after: unchanged
api.verify_mixed_counters(reset=True)
out["mixed_after"] = z.verify_envelopes(envs)
m = api.verify_mixed_counters(reset=True)
out["mixed_after_counters"] = [m["launches"], m["point_adds"]]

# ---- wrong statements on valid proofs
wops, touched = wrong_statements(ops)
out["touched"] = {str(k): v for k, v in touched.items()}
out["wrong_ref"] = reference_verdicts(wops, envs)
api.verify_statements_counters(reset=True)          # (the plain round trip above counted too)
out["wrong"] = split(z.verify_ops(wops, envs, reasons=True))
out["wrong_counters"] = counters()

# ---- wrong proofs under right statements: one flipped byte per scheme
bad = list(envs); flipped = []
for scheme in range(1, 7):
    i = next(i for i, e in enumerate(envs) if e[1] == scheme)
    bad[i] = flip_proof(bad[i]); flipped.append(i)
out["flipped"] = flipped
out["bad_ref"] = reference_verdicts(ops, bad)
out["bad"] = split(z.verify_ops(ops, bad, reasons=True))
out["bad_counters"] = counters()

# ---- envelope refusals beside statement refusals: another scheme's envelope, a truncated one, an empty one
mis = list(envs); mis[0], mis[1] = envs[1], envs[0]; mis[5] = envs[5][:-1]; mis[6] = b""
out["mis_ref"] = reference_verdicts(wops, mis)
out["mis"] = split(z.verify_ops(wops, mis, reasons=True))

# ---- the device form on the same lists
out["device_base"] = raw_call(ops, envs, device=True)
out["device_wrong"] = raw_call(wops, bad, device=True)
out["host_wrong"] = raw_call(wops, bad)
print(json.dumps(out))
"""

_BATCH_CHECKS = _COMMON + r"""
# started with ZKP_HIP_BATCH_VERIFY_MIN=8 and ZKP_HIP_G16_BATCH_VERIFY_MIN=8: every scheme of a 64-envelope list takes its batch check
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
load_keys()
ops = mixed_ops((16, 8, 12, 10, 8, 10), 33)
assert len(ops) == 64
envs = api.process_ops(ops, seeds_for(64, 4))
wops = list(ops); wrong = []
for kind, change in (("range", lambda o: ("range", o[1], o[2], o[3] + 1)), ("threshold", lambda o: ("threshold", o[1], o[2] + 1)),
                     ("equality", lambda o: ("equality", o[1] + 1, o[2] + 1)), ("membership", lambda o: ("membership", o[1], [x ^ 2 for x in o[2]])),
                     ("improvement", lambda o: ("improvement", o[1] + 1, o[2]))):
    i = at(wops, kind, skip=2); wops[i] = change(wops[i]); wrong.append(i)
out["wrong"] = wrong
def checks():
    b, g = api.bp_verify_counters(reset=True), api.groth16_verify_counters(reset=True)
    return [b["failed_checks"], g["launches"], g["point_adds"]]
checks()
out["ref"] = reference_verdicts(wops, envs)
checks()
out["got"] = split(z.verify_ops(wops, envs, reasons=True))
out["checks_statements_only"] = checks()
bad = list(envs); i_range = at(ops, "range", skip=5); bad[i_range] = flip(bad[i_range], 700)
out["flipped"] = i_range
out["got_flipped"] = split(z.verify_ops(wops, bad, reasons=True))
out["checks_flipped"] = checks()
print(json.dumps(out))
"""

_TWO_SHARDS = _COMMON + r"""
_native.init_devices([0, 0])                                     # two shards of the library on one GPU
load_keys()
os.environ["ZKP_HIP_VERIFY_SHARD_MIN"] = "4"
ops = base_ops()
envs = api.process_ops(ops, seeds_for(len(ops), 1))
wops, touched = wrong_statements(ops)
bad = list(envs); i = at(ops, "consistency", skip=3); bad[i] = flip_proof(bad[i])
out["n"] = len(ops); out["flipped"] = i
out["ref"] = reference_verdicts(wops, bad)
def counted(**env):
    os.environ.update(env)
    api.verify_fanout_counters(reset=True); api.verify_statements_counters(reset=True)
    try:
        got = split(z.verify_ops(wops, bad, reasons=True))
    finally:
        f = api.verify_fanout_counters(reset=True); s = api.verify_statements_counters(reset=True)
        for k in env: del os.environ[k]
    return got, [f["launches"], f["point_adds"]], [s["envelopes"], s["refused_envelope"], s["refused_statement"], s["refused_proof"]]
out["fanned"], out["fanned_fanout"], out["fanned_statements"] = counted()
out["one_shard"], out["one_shard_fanout"], out["one_shard_statements"] = counted(ZKP_HIP_VERIFY_SHARDS="0")
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


def test_round_trip_of_a_proved_list(main):
    n = len(main["kinds"])
    assert 34 <= n <= 44 and set(main["kinds"]) == {"range", "threshold", "equality", "membership", "improvement", "consistency"}
    assert main["ref_base"] == [True] * n                                               # the per-scheme calls accept every proof for its statement
    assert main["base"] == [[True] * n, [ACCEPTED] * n] and main["base_plain"] == [True] * n and main["empty"] == []
    assert main["base_counters"] == {"envelopes": n, "refused_envelope": 0, "refused_statement": 0, "refused_proof": 0, "ms_positive": True}


def test_wrong_statements_on_valid_proofs_are_refused_as_statements(main):
    n = len(main["kinds"])
    touched = {int(k): v for k, v in main["touched"].items()}
    assert len(touched) == 12 and sum(touched.values()) == 3          # the right commitment and the two permuted sets stay accepted
    want = [touched.get(i, True) for i in range(n)]
    assert main["wrong_ref"] == want
    ok, why = main["wrong"]
    print(json.dumps({"refused": [i for i in range(n) if not ok[i]]}))
    assert ok == want and why == [ACCEPTED if w else STATEMENT for w in want]
    assert main["wrong_counters"] == {"envelopes": n, "refused_envelope": 0, "refused_statement": 9, "refused_proof": 0, "ms_positive": True}


def test_wrong_proofs_under_right_statements_are_refused_as_proofs(main):
    n = len(main["kinds"])
    want = [i not in main["flipped"] for i in range(n)]
    assert len(set(main["flipped"])) == 6 and main["bad_ref"] == want
    assert main["bad"] == [want, [ACCEPTED if w else PROOF for w in want]]
    assert main["bad_counters"] == {"envelopes": n, "refused_envelope": 0, "refused_statement": 0, "refused_proof": 6, "ms_positive": True}


def test_envelope_refusals_come_before_statement_refusals(main):
    n = len(main["kinds"])
    touched = {int(k): v for k, v in main["touched"].items()}
    ok, why = main["mis"]
    assert ok == main["mis_ref"]
    for i in (0, 1, 5, 6):
        assert why[i] == ENVELOPE and not ok[i]
    for i in range(n):
        if i not in (0, 1, 5, 6):
            assert why[i] == (ACCEPTED if touched.get(i, True) else STATEMENT)


def test_device_form_gives_the_host_forms_verdicts_and_reasons(main):
    n = len(main["kinds"])
    assert main["device_base"] == [0, [1] * n, [ACCEPTED] * n]
    assert main["device_wrong"] == main["host_wrong"] and main["host_wrong"][0] == 0
    why = main["host_wrong"][2]
    assert why.count(PROOF) >= 1 and why.count(STATEMENT) == 9 and 9 not in why and 9 not in main["host_wrong"][1]


def test_the_mixed_verifier_is_unchanged_by_statement_calls(main):
    n = len(main["kinds"])
    assert main["mixed_after"] == [True] * n and main["mixed_after_counters"] == [6, n]


def test_a_key_is_needed_only_for_envelopes_that_reach_their_verifier(main):
    k = main["no_key"]
    assert k["other_kind"] == [0, [0], [ENVELOPE]] and k["wrong_statement"] == [0, [0], [STATEMENT]]
    assert k["live"] == -3 and "no (usable) key loaded" in k["live_msg"]


def test_statement_mismatches_make_no_batch_check_fail():
    r = _child(_BATCH_CHECKS, ZKP_HIP_BATCH_VERIFY_MIN="8", ZKP_HIP_G16_BATCH_VERIFY_MIN="8")
    want = [i not in r["wrong"] for i in range(64)]
    assert len(set(r["wrong"])) == 5 and r["ref"] == want
    assert r["got"] == [want, [ACCEPTED if w else STATEMENT for w in want]]
    assert r["checks_statements_only"] == [0, 0, 0]                     # no failed Bulletproofs check, no Groth16 localisation
    want[r["flipped"]] = False
    why = [ACCEPTED if w else STATEMENT for w in want]; why[r["flipped"]] = PROOF
    assert r["flipped"] not in r["wrong"] and r["got_flipped"] == [want, why]
    assert r["checks_flipped"] == [1, 0, 0]                             # the one flipped range proof: one failed check


def test_two_shards_on_one_gpu_carry_rebased_list_spans():
    r = _child(_TWO_SHARDS)
    n = r["n"]
    ok, why = r["fanned"]
    assert ok == r["ref"] and r["one_shard"] == r["fanned"]
    assert why[r["flipped"]] == PROOF and why.count(STATEMENT) == 9 and why.count(PROOF) == 1
    assert r["fanned_fanout"] == [2, n] and r["one_shard_fanout"] == [0, 0]
    assert r["fanned_statements"] == [n, 0, 9, 1] == r["one_shard_statements"]


def test_the_python_names_are_exported():
    import libzkp_amd as z
    import libzkp_amd.api as api
    assert z.verify_ops is api.verify_ops and z.verify_statements_counters is api.verify_statements_counters
    assert "verify_ops" in z.__all__ and "verify_statements_counters" in z.__all__
