"""What the self-check (ZKP_HIP_OP_SELF_CHECK) costs: the mixed batch (C5's i mod 4 mix) staged in HBM twice, once flagged and once not,
zkp_hip_batch_prove timed on the two alternately.  Prints one JSON line: medians of the runs, and the self-check counter's ms per batch.
Usage: bench_self_check.py [ops = 4096] [runs of each = 9]"""
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libzkp_amd import _native, api, workloads as wl  # noqa: E402

L = _native.lib()
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
runs = int(sys.argv[2]) if len(sys.argv) > 2 else 9
_native.check(L.zkp_hip_init(0), "init")
for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
    blob = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, _native.last_error()
ops, lists, seeds = wl.mixed_ops(n, 5)
flagged = ops.copy()
flagged["kind"] |= _native.OP_SELF_CHECK
handles = {}
for name, o in (("plain", ops), ("self_check", flagged)):
    h = ctypes.c_void_p()
    assert L.zkp_hip_batch_stage(n, P(o), P(lists), P(seeds), ctypes.byref(h)) == 0, _native.last_error()
    handles[name] = h
    for _ in range(2):                                   # warm-up: workspaces, the verifiers' tables
        assert L.zkp_hip_batch_prove(h) == 0, _native.last_error()
api.batch_self_check_counters(reset=True)
ms = {"plain": [], "self_check": []}
for _ in range(runs):
    for name in ("plain", "self_check"):
        t0 = time.perf_counter()
        rc = L.zkp_hip_batch_prove(handles[name])
        ms[name].append((time.perf_counter() - t0) * 1e3)
        assert rc == 0, _native.last_error()
c = api.batch_self_check_counters(reset=True)
for h in handles.values():
    L.zkp_hip_batch_free(h)
med = lambda xs: sorted(xs)[len(xs) // 2]  # noqa: E731
print(json.dumps({"ops": n, "runs_each": runs, "plain_ms_median": round(med(ms["plain"]), 3), "self_check_ms_median": round(med(ms["self_check"]), 3),
                  "plain_ms": [round(x, 3) for x in ms["plain"]], "self_check_ms": [round(x, 3) for x in ms["self_check"]],
                  "counter_ms_per_batch": round(c["ms"] / runs, 3), "ops_verified_per_batch": c["launches"] // runs, "ops_refused": c["point_adds"]}))
L.zkp_hip_shutdown()
