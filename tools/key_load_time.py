"""Time zkp_hip_groth16_load_key for both circuits (window-table construction on the GPU): python tools/key_load_time.py [reps] [--verifying-key] [--json]
--verifying-key loads the VerifyingKey prefix of each golden proving key (the content of a `{prefix}_vk.bin`) instead of the proving key.
--json prints ONE line for the process: wall time and device memory taken (hipMemGetInfo before - after) of the first load of each circuit
-- the equality key, loaded first, carries the HIP runtime's one-time allocations -- and what zkp_hip_groth16_key_info reports; run it in
as many processes as medians are wanted.  ZKP_HIP_LIB selects another build of the library (the parent commit's)."""
import ctypes, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libzkp_amd import _native
L = _native.lib()
_native.check(L.zkp_hip_init(0), "init")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
reps = int(args[0]) if args else 3
verifier, as_json = "--verifying-key" in sys.argv, "--json" in sys.argv


def free_bytes():
    a, b = ctypes.c_size_t(), ctypes.c_size_t()
    f = L.hipMemGetInfo; f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]; f.restype = ctypes.c_int
    assert f(ctypes.byref(a), ctypes.byref(b)) == 0
    return a.value


def key_blob(name):
    blob = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
    return blob[:64 + 3 * 128 + 8 + 64 * int.from_bytes(blob[448:456], "little")] if verifier else blob


if as_json:          # the MiMC constants and the first kernel launch of the process are not the key's
    assert L.zkp_hip_snark_commit_value_batch(1, np.array([7], dtype=np.uint64).ctypes.data_as(ctypes.c_void_p), np.zeros(32, dtype=np.uint8).ctypes.data_as(ctypes.c_void_p)) == 0
    reps = 1
out = {"key": "verifying" if verifier else "proving", "wbits_env": os.environ.get("ZKP_HIP_G16_WBITS", "")}
for r in range(reps):
    ts = []
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        blob = key_blob(name)
        f0 = free_bytes()
        t0 = time.perf_counter(); assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, _native.last_error(); ts.append(time.perf_counter() - t0)
        if r == 0:
            w, u, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
            L.zkp_hip_groth16_key_info(kind, ctypes.byref(w), ctypes.byref(u), ctypes.byref(b))
            out["load_s_%d" % kind] = round(ts[-1], 4); out["taken_%d" % kind] = f0 - free_bytes(); out["key_info_%d" % kind] = [w.value, u.value, b.value]
    if not as_json:
        print("load_key: equality %.3f s, membership %.3f s, both %.3f s" % (ts[0], ts[1], sum(ts)))
if as_json:
    print(json.dumps(out))
L.zkp_hip_shutdown()
