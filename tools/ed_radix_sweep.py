"""Bulletproofs work at one generator-table radix (ZKP_HIP_ED_WBITS, include/libzkp_hip.h): init time (the table build is most of it),
4096 x prove_range through the host-buffer entry, the staged 4096-op mixed batch, and 4096 range verifications; medians of REPS, one JSON
line.  Run one process per radix: python tools/ed_radix_sweep.py WBITS [REPS]"""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["ZKP_HIP_ED_WBITS"] = sys.argv[1]
from libzkp_amd import _native, workloads as wl  # noqa: E402

reps = int(sys.argv[2]) if len(sys.argv) > 2 else 7
L = _native.lib()
P = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731


def med(f):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); ts.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(ts), 3)


t0 = time.perf_counter()
_native.check(L.zkp_hip_init(0), "init")
init_ms = (time.perf_counter() - t0) * 1e3
w, u, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
L.zkp_hip_groth16_key_info(2, ctypes.byref(w), ctypes.byref(u), ctypes.byref(b))
n = 4096
ops, lists, seeds = wl.range_ops(n)
v, mn, mx = ops["a"].copy(), ops["b"].copy(), ops["c"].copy()
out, ln, st = np.zeros((n, 1478), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
prove = lambda: L.zkp_hip_prove_range_batch(n, P(v), P(mn), P(mx), 64, P(seeds), P(out), 1478, P(ln), P(st))  # noqa: E731
assert prove() == 0
ok = np.zeros(n, dtype=np.uint8)
verify = lambda: L.zkp_hip_verify_range_batch(n, P(out), 1478, P(ln), P(mn), P(mx), P(ok))  # noqa: E731
assert verify() == 0 and ok.all()
for k, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
    blob = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    assert L.zkp_hip_groth16_load_key(k, blob, len(blob)) == 0, _native.last_error()
mops, mlists, mseeds = wl.mixed_ops(n, 5)
h = ctypes.c_void_p()
assert L.zkp_hip_batch_stage(n, P(mops), P(mlists), P(mseeds), ctypes.byref(h)) == 0
for _ in range(3):
    assert L.zkp_hip_batch_prove(h) == 0
res = {"wbits": w.value, "table_bytes": b.value, "init_ms": round(init_ms, 1), "prove_range_4096_ms": med(prove),
       "mixed_4096_staged_ms": med(lambda: L.zkp_hip_batch_prove(h)), "verify_range_4096_ms": med(verify)}
L.zkp_hip_batch_free(h)
L.zkp_hip_shutdown()
print(json.dumps(res), flush=True)
