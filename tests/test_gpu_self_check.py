"""Self-check of a staged batch (ZKP_HIP_OP_SELF_CHECK, include/libzkp_hip.h): every scheme's verifier runs over the proofs where they lie
in HBM, against the op's own staged parameters, before lengths, offsets and the packed output exist; a refused op leaves as a failed op.
Several of the switches involved are read once per process, so every case runs in a fresh child process (this file run as a script) that
prints one JSON line; the children force the smallest table radices (proof bytes do not depend on them) to keep their start-up short."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
KNOBS = ("ZKP_HIP_SELF_CHECK_FLIP", "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_G16_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY", "ZKP_HIP_G16_LOCALISE", "ZKP_HIP_G16_LOCALISE_SEGMENT",
         "ZKP_HIP_BP_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_VERIFY_VM")
FLAG = 0x100
REFUSED, INVALID = 2, 1


def run_child(case, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update({"ZKP_HIP_ED_WBITS": "10", "ZKP_HIP_G16_WBITS": "8"})
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (case, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------- the tests (one child at a time)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solo():
    """the 13-op batch on one shard: unflagged, flagged, and flagged with one flipped bit (the reference of the cases below)"""
    return run_child("solo")


def test_all_accepted_is_byte_identical(solo):
    plain, checked = solo["plain"], solo["checked"]
    assert plain["rc"] == 1 and checked["rc"] == 1                                # the invalid equality op fails either batch
    assert checked["proofs"] == plain["proofs"] and checked["off"] == plain["off"] and checked["st"] == plain["st"]
    assert plain["st"] == [0] * 6 + [INVALID] + [0] * 6 and plain["lens"][6] == 0 and all(plain["lens"][i] > 0 for i in range(13) if i != 6)
    assert solo["plain_counters"]["launches"] == 0 and solo["plain_counters"]["point_adds"] == 0      # an unflagged batch is not checked
    assert solo["checked_counters"]["launches"] == 12 and solo["checked_counters"]["point_adds"] == 0 and solo["checked_counters"]["ms"] > 0


def test_one_refusal_per_scheme():
    r = run_child("refusals")
    assert r["failures"] == [], r
    assert sorted(r["kinds_refused"]) == ["consistency", "equality", "improvement", "membership", "range", "range-framing", "threshold"]


def test_batch_check_paths_through_the_device_cores():
    r = run_child("batch_paths", ZKP_HIP_BATCH_VERIFY_MIN="1", ZKP_HIP_G16_BATCH_VERIFY_MIN="1", ZKP_HIP_G16_LOCALISE_SEGMENT="8")
    assert r["failures"] == [], r
    assert r["clean"]["refused"] == [] and r["clean"]["counters"]["launches"] == 80 and r["clean"]["g16_after_failed_checks"] == 0
    assert r["flipped"]["refused"] == r["flipped"]["targets"] and r["flipped"]["counters"]["point_adds"] == 2
    assert r["flipped"]["g16_segment_checks"] == 5 and r["flipped"]["g16_after_failed_checks"] == 8      # localisation ran on the arena's rows


def test_two_shards_on_one_gpu(solo):
    r = run_child("two_shards")
    assert r["shards"] == 2
    for k in ("checked", "flipped"):
        assert r[k]["rc"] == solo[k]["rc"] == 1
        assert r[k]["proofs"] == solo[k]["proofs"] and r[k]["off"] == solo[k]["off"] and r[k]["st"] == solo[k]["st"], k
    assert r["flipped"]["st"][0] == REFUSED and r["flipped_counters"]["launches"] == 12 and r["flipped_counters"]["point_adds"] == 1
    assert r["one_op"]["rc"] == 0 and r["one_op"]["st"] == [0] and r["one_op"]["lens"] == [1478] and r["one_op_counters"]["launches"] == 1


def test_two_batches_in_flight():
    r = run_child("in_flight")
    assert r["failures"] == [], r
    assert r["a"] == r["a_solo"] and r["b"] == r["b_solo"] and r["a"]["proofs"] != r["b"]["proofs"]
    assert r["counters"]["launches"] == 24 and r["counters"]["point_adds"] == 0


def test_repeated_prove_checks_each_time(solo):
    r = run_child("repeat")
    assert r["first"] == r["second"] and r["first"]["proofs"] == solo["checked"]["proofs"] and r["first"]["st"] == solo["checked"]["st"]
    assert r["counters"]["launches"] == 24 and r["flip_then_clean"] == [1, 0]      # the switch is read on every prove


def test_bad_switch_values_and_mixed_flags():
    r = run_child("bad_values")
    for value, (rc, err) in r["flip"].items():
        assert rc == -3 and "ZKP_HIP_SELF_CHECK_FLIP" in err, (value, rc, err)
    assert r["unflagged_with_bad_switch"] == 1          # (the invalid op's 1: the switch has no effect on an unflagged batch)
    assert r["mixed"][0] == -3 and "self-check is a property of the whole batch" in r["mixed"][1]
    assert r["staged_mixed"][0] == -3


def test_python_surface():
    r = run_child("python")
    assert r["same"] is True and r["n"] == 12 and r["counters"]["launches"] == 12 and r["counters"]["point_adds"] == 0
    assert r["registry_same"] is True and r["refused_raises"] is True and r["exported"] is True


# ---------------------------------------------------------------------------------------------------- child side
def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _setup(shards=None):
    sys.path.insert(0, ROOT)
    from libzkp_amd import _native, api
    L = _native.lib()
    if shards:
        _native.init_devices(shards)
    else:
        _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        blob = open(os.path.join(GOLD, name), "rb").read()
        assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, _native.last_error()
    with api._snark_lock:
        api._keys_loaded[0] = api._keys_loaded[1] = True
    return L, _native, api


NAMES = {1: "range", 2: "equality", 3: "threshold", 4: "membership", 5: "improvement", 6: "consistency"}


def _ops(tuples):
    """api-style tuples -> (zkp_hip_op array, lists)"""
    from libzkp_amd import workloads as wl
    ops = np.zeros(len(tuples), dtype=wl.OP_DTYPE)
    lists = []
    for i, o in enumerate(tuples):
        k = o[0]
        if k == "range":
            ops[i] = (1, 0, o[1], o[2], o[3], 0)
        elif k == "equality":
            ops[i] = (2, 0, o[1], o[2], 0, 0)
        elif k == "improvement":
            ops[i] = (5, 0, o[1], o[2], 0, 0)
        elif k == "threshold":
            ops[i] = (3, len(o[1]), o[2], 0, 0, len(lists)); lists.extend(o[1])
        elif k == "membership":
            ops[i] = (4, len(o[2]), o[1], 0, 0, len(lists)); lists.extend(o[2])
        else:
            ops[i] = (6, len(o[1]), 0, 0, 0, len(lists)); lists.extend(o[1])
    return ops, np.array(lists if lists else [0], dtype=np.uint64)


def batch13(small_set=1):
    """two ops of each kind and one invalid op (equality with a != b, op 6); membership sets of `small_set` and 64 elements, consistency
    lists of 1 value (no range proof inside) and 4 values"""
    s0 = tuple(range(9, 9 + small_set))
    s1 = tuple(1000 + 3 * i for i in range(64))
    return [("range", 7, 0, 100), ("equality", 42, 42), ("threshold", (10, 20, 30), 50), ("membership", s0[-1], s0), ("improvement", 3, 9), ("consistency", (5,)),
            ("equality", 1, 2), ("range", 2**32, 0, 2**32), ("equality", 2**63, 2**63), ("threshold", (2**40,), 1), ("membership", s1[37], s1), ("improvement", 10, 2**40),
            ("consistency", (1, 5, 5, 9))]


def _seeds(n, tag=5):
    return np.frombuffer(b"".join(hashlib.sha256(tag.to_bytes(8, "little") + i.to_bytes(8, "little")).digest() for i in range(n)), dtype=np.uint8).copy()


def _result(rc, out, off, st):
    n = len(st)
    proofs = [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    return {"rc": rc, "proofs": [hashlib.sha256(p).hexdigest() if p else "" for p in proofs], "off": [int(x) for x in off], "st": [int(x) for x in st],
            "lens": [len(p) for p in proofs]}, proofs


def _process(L, tuples, seeds, flagged, flip=None, cap=None):
    from libzkp_amd import workloads as wl
    ops, lists = _ops(tuples)
    if flagged:
        ops["kind"] |= FLAG
    n = len(ops)
    cap = cap or wl.max_output_bytes(_ops(tuples)[0])
    out, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    if flip is None:
        os.environ.pop("ZKP_HIP_SELF_CHECK_FLIP", None)
    else:
        os.environ["ZKP_HIP_SELF_CHECK_FLIP"] = flip
    rc = L.zkp_hip_process_batch(n, _P(ops), _P(lists), _P(seeds), _P(out), cap, _P(off), _P(st))
    os.environ.pop("ZKP_HIP_SELF_CHECK_FLIP", None)
    assert rc >= 0, L.zkp_hip_last_error()
    return _result(rc, out, off, st)


def _stage(L, tuples, seeds, flagged=True):
    ops, lists = _ops(tuples)
    if flagged:
        ops["kind"] |= FLAG
    h = ctypes.c_void_p()
    rc = L.zkp_hip_batch_stage(len(ops), _P(ops), _P(lists), _P(seeds), ctypes.byref(h))
    return rc, h


def _fetch(L, h, n):
    cap = int(L.zkp_hip_batch_max_bytes(h))
    out, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_batch_fetch(h, _P(out), cap, _P(off), _P(st))
    assert rc >= 0, L.zkp_hip_last_error()
    return _result(rc, out, off, st)[0]


def _compact(res):
    return res["off"][0] == 0 and all(res["off"][i + 1] - res["off"][i] == res["lens"][i] for i in range(len(res["lens"])))


def child_solo():
    L, _native, api = _setup()
    t, sd = batch13(), _seeds(13)
    api.batch_self_check_counters(reset=True)
    out = {"plain": _process(L, t, sd, False)[0]}
    out["plain_counters"] = api.batch_self_check_counters(reset=True)
    out["checked"] = _process(L, t, sd, True)[0]
    out["checked_counters"] = api.batch_self_check_counters(reset=True)
    out["flipped"] = _process(L, t, sd, True, flip="0:100")[0]
    return out


def _host_verdict(api, o, proof):
    k = o[0]
    if k == "range":
        return api.verify_range(proof, o[2], o[3])
    if k == "equality":
        return api.verify_equality(proof, o[1], o[2])
    if k == "threshold":
        return api.verify_threshold(proof, o[2])
    if k == "membership":
        return api.verify_membership(proof, list(o[2]))
    if k == "improvement":
        return api.verify_improvement(proof, o[1])
    return api.verify_consistency(proof)


def child_refusals():
    L, _native, api = _setup()
    t, sd = batch13(small_set=16), _seeds(13)
    fails, kinds = [], []
    clean, clean_proofs = _process(L, t, sd, True)
    if clean["rc"] != 1 or clean["st"] != [0] * 6 + [INVALID] + [0] * 6:
        fails.append(("clean", clean["rc"], clean["st"]))
    for op, byte, name in ((0, 100, "range"), (1, 100, "equality"), (2, 100, "threshold"), (3, 100, "membership"), (4, 100, "improvement"), (12, 100, "consistency"),
                           (7, 5, "range-framing")):
        api.batch_self_check_counters(reset=True)
        got, _ = _process(L, t, sd, True, flip="%d:%d" % (op, byte))
        c = api.batch_self_check_counters(reset=True)
        want_st = list(clean["st"]); want_st[op] = REFUSED
        ok = got["rc"] == 1 and got["st"] == want_st and got["lens"][op] == 0 and _compact(got)
        ok = ok and all(got["proofs"][i] == clean["proofs"][i] for i in range(13) if i != op)
        ok = ok and c["launches"] == 12 and c["point_adds"] == 1
        tampered = bytearray(clean_proofs[op]); tampered[byte] ^= 1
        host_accepts_clean, host_accepts_tampered = _host_verdict(api, t[op], clean_proofs[op]), _host_verdict(api, t[op], bytes(tampered))
        if not ok or not host_accepts_clean or host_accepts_tampered:
            fails.append((name, got["rc"], got["st"], got["lens"], c, host_accepts_clean, host_accepts_tampered))
        else:
            kinds.append(name)
    return {"failures": fails, "kinds_refused": kinds}


def child_batch_paths():
    L, _native, api = _setup()
    t = [("range", 1000 + i, 0, 2**32) if i % 2 == 0 else ("equality", 77 + i, 77 + i) for i in range(80)]
    sd = _seeds(80, tag=9)
    fails = []
    out = {}
    plain, _ = _process(L, t, sd, False)
    for name, flip_ops in (("clean", []), ("flipped", [34, 51])):          # (one flip per call: two calls, their refusals together)
        api.batch_self_check_counters(reset=True); api.groth16_verify_counters(reset=True)
        refused = []
        for f in flip_ops or [None]:
            # a range op: a proof byte; an equality op: a commitment byte, so the points still parse and the weighted pairing check is what fails
            got, _ = _process(L, t, sd, True, flip=None if f is None else "%d:%d" % (f, 100 if f % 2 == 0 else 270))
            bad = [i for i in range(80) if got["st"][i] != 0]
            refused += bad
            if bad != ([] if f is None else [f]) or not _compact(got) or any(got["proofs"][i] != plain["proofs"][i] for i in range(80) if i not in bad):
                fails.append((name, f, bad))
        c, g16 = api.batch_self_check_counters(reset=True), api.groth16_verify_counters(reset=True)
        out[name] = {"refused": refused, "targets": flip_ops, "counters": c, "g16_segment_checks": g16["launches"], "g16_after_failed_checks": g16["point_adds"]}
    out["failures"] = fails
    return out


def child_two_shards():
    L, _native, api = _setup(shards=[0, 0])
    t, sd = batch13(), _seeds(13)
    out = {"shards": int(L.zkp_hip_device_count())}
    out["checked"] = _process(L, t, sd, True)[0]
    api.batch_self_check_counters(reset=True)
    out["flipped"] = _process(L, t, sd, True, flip="0:100")[0]
    out["flipped_counters"] = api.batch_self_check_counters(reset=True)
    out["one_op"] = _process(L, t[:1], sd[:32], True)[0]          # one shard is left without ops
    out["one_op_counters"] = api.batch_self_check_counters(reset=True)
    return out


def child_in_flight():
    L, _native, api = _setup()
    ta, tb = batch13(), batch13(small_set=3)
    sa, sb = _seeds(13, tag=21), _seeds(13, tag=22)
    out = {"a_solo": _process(L, ta, sa, True)[0], "b_solo": _process(L, tb, sb, True)[0]}
    api.batch_self_check_counters(reset=True)
    (rca, ha), (rcb, hb) = _stage(L, ta, sa), _stage(L, tb, sb)
    rcs = [rca, rcb, L.zkp_hip_batch_prove_async(ha), L.zkp_hip_batch_prove_async(hb), L.zkp_hip_batch_wait(ha), L.zkp_hip_batch_wait(hb)]
    out["a"], out["b"] = _fetch(L, ha, 13), _fetch(L, hb, 13)
    L.zkp_hip_batch_free(ha); L.zkp_hip_batch_free(hb)
    out["counters"] = api.batch_self_check_counters(reset=True)
    out["failures"] = [] if rcs == [0] * 6 else [rcs, _native.last_error()]
    return out


def child_repeat():
    L, _native, api = _setup()
    t, sd = batch13(), _seeds(13)
    rc, h = _stage(L, t, sd)
    assert rc == 0, _native.last_error()
    api.batch_self_check_counters(reset=True)
    out = {}
    for name in ("first", "second"):
        assert L.zkp_hip_batch_prove(h) == 0, _native.last_error()
        out[name] = _fetch(L, h, 13)
    out["counters"] = api.batch_self_check_counters(reset=True)
    flips = []
    for flip in ("4:100", None):
        if flip:
            os.environ["ZKP_HIP_SELF_CHECK_FLIP"] = flip
        else:
            os.environ.pop("ZKP_HIP_SELF_CHECK_FLIP", None)
        assert L.zkp_hip_batch_prove(h) == 0, _native.last_error()
        _fetch(L, h, 13)
        flips.append(api.batch_self_check_counters(reset=True)["point_adds"])
    out["flip_then_clean"] = flips
    L.zkp_hip_batch_free(h)
    return out


def child_bad_values():
    L, _native, api = _setup()
    t, sd = batch13(), _seeds(13)
    rc, h = _stage(L, t, sd)
    assert rc == 0, _native.last_error()
    out = {"flip": {}}
    for value in ("13:0", "0:1478", "1:298", "6:0", "abc", "3", "3:", ":5", "-1:5", "1:2:3", "4:0x10"):
        os.environ["ZKP_HIP_SELF_CHECK_FLIP"] = value
        rc = L.zkp_hip_batch_prove(h)
        out["flip"][value] = [rc, _native.last_error() if rc < 0 else ""]
    L.zkp_hip_batch_free(h)
    os.environ["ZKP_HIP_SELF_CHECK_FLIP"] = "99:99"
    rc, h = _stage(L, t, sd, flagged=False)
    assert rc == 0, _native.last_error()
    assert L.zkp_hip_batch_prove(h) == 0, _native.last_error()
    out["unflagged_with_bad_switch"] = _fetch(L, h, 13)["rc"]
    L.zkp_hip_batch_free(h)
    os.environ.pop("ZKP_HIP_SELF_CHECK_FLIP", None)
    ops, lists = _ops(t)
    ops["kind"][[0, 5]] |= FLAG
    cap = 1 << 16
    o, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(14, dtype=np.uint64), np.zeros(13, dtype=np.int32)
    rc = L.zkp_hip_process_batch(13, _P(ops), _P(lists), _P(sd), _P(o), cap, _P(off), _P(st))
    out["mixed"] = [rc, _native.last_error()]
    h = ctypes.c_void_p()
    out["staged_mixed"] = [L.zkp_hip_batch_stage(13, _P(ops), _P(lists), _P(sd), ctypes.byref(h)), _native.last_error()]
    return out


def child_python():
    L, _native, api = _setup()
    t = [o for i, o in enumerate(batch13()) if i != 6]
    sd = bytes(_seeds(12, tag=31))
    api.batch_self_check_counters(reset=True)
    checked = api.process_ops(t, sd, self_check=True)
    c = api.batch_self_check_counters(reset=True)
    plain = api.process_ops(t, sd)
    import libzkp_amd as z
    b = z.create_proof_batch()
    z.batch_add_range_proof(b, 7, 0, 100); z.batch_add_improvement_proof(b, 3, 9); z.batch_add_consistency_proof(b, [1, 5, 5, 9])
    via_registry = z.process_batch(b, seeds=sd[:96], self_check=True)
    direct = api.process_ops([("range", 7, 0, 100), ("improvement", 3, 9), ("consistency", (1, 5, 5, 9))], sd[:96])
    os.environ["ZKP_HIP_SELF_CHECK_FLIP"] = "1:100"
    try:
        api.process_ops(t, sd, self_check=True)
        raised = False
    except api.ZkpBackendError as e:
        raised = "operation 1 (equality) failed with status 2" in str(e)
    os.environ.pop("ZKP_HIP_SELF_CHECK_FLIP", None)
    return {"same": checked == plain and all(len(p) > 0 for p in plain), "n": len(plain), "counters": c, "registry_same": via_registry == direct, "refused_raises": raised,
            "exported": z.batch_self_check_counters is api.batch_self_check_counters}


if __name__ == "__main__":
    print(json.dumps({"solo": child_solo, "refusals": child_refusals, "batch_paths": child_batch_paths, "two_shards": child_two_shards, "in_flight": child_in_flight,
                      "repeat": child_repeat, "bad_values": child_bad_values, "python": child_python}[sys.argv[1]]()))
