"""Cost of one bad envelope in a range batch that takes the batch check (zkp_hip_verify_range_batch, host buffers in, verdicts out), with
the localisation pass (bp_localise.h) at several segment sizes and without it (ZKP_HIP_BP_LOCALISE=0: the per-job pass over the whole
batch, what the call did before the pass existed), beside the clean batch.  One process, one GPU; the configurations of a size are timed in
alternation, every one warmed first; host wall clock around the call, which ends in a device synchronise.  Prints one JSON object
(profiles/bp_localise.json is this output).

  python tools/bench_bp_localise.py [--sizes 2048,4096,16384] [--rounds 15] [--lib other/libzkp_hip.so] [--out file.json]

--lib: another build of the library, such as the parent commit's, for the clean batch and the whole-batch pass on the same box in the
same session; a build without the counters entry point runs only the configurations it knows."""
import argparse, ctypes, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from libzkp_amd import _native, workloads as wl

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="2048,4096,16384")
ap.add_argument("--rounds", type=int, default=15)
ap.add_argument("--lib", default=None)
ap.add_argument("--out", default=None)
args = ap.parse_args()

_native._preload_hip_runtime()
L = ctypes.CDLL(args.lib or _native.LIB_PATH)
u64, vp = ctypes.c_uint64, ctypes.c_void_p
L.zkp_hip_init.argtypes = [ctypes.c_int]
L.zkp_hip_prove_range_batch.argtypes = [u64, vp, vp, vp, ctypes.c_uint32, vp, vp, u64, vp, vp]
L.zkp_hip_verify_range_batch.argtypes = [u64, vp, u64, vp, vp, vp, vp]
L.zkp_hip_last_error.restype = ctypes.c_char_p
has_pass = hasattr(L, "zkp_hip_bp_localise_counters")
P = lambda a: a.ctypes.data_as(vp)
SWITCHES = ("ZKP_HIP_BP_LOCALISE", "ZKP_HIP_BP_LOCALISE_SEGMENT", "ZKP_HIP_BATCH_VERIFY_MIN", "ZKP_HIP_NO_BATCH_VERIFY")
assert L.zkp_hip_init(0) == 0, L.zkp_hip_last_error()


def counters():
    if not has_pass:
        return None
    ms, a, b, c = ctypes.c_double(), u64(), u64(), u64()
    assert L.zkp_hip_bp_localise_counters(ctypes.byref(ms), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), 1) == 0
    return {"failed_checks": a.value, "segment_checks": b.value, "jobs_again": c.value}


def call(cfg, n, buf, ln, lo, hi, ok):
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ["ZKP_HIP_BATCH_VERIFY_MIN"] = "1"                        # the batch check at every size (2048 envelopes are its default threshold)
    os.environ.update(cfg)
    t0 = time.perf_counter()
    rc = L.zkp_hip_verify_range_batch(n, P(buf), 1478, P(ln), P(lo), P(hi), P(ok))
    dt = time.perf_counter() - t0
    assert rc == 0, L.zkp_hip_last_error()
    return dt * 1e3


rows = []
for n in [int(a) for a in args.sizes.split(",")]:
    ops, _, seeds = wl.range_ops(n, 1)
    v, lo, hi = ops["a"].copy(), ops["b"].copy(), ops["c"].copy()
    out = np.zeros((n, 1478), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32); st = np.zeros(n, dtype=np.int32)
    assert L.zkp_hip_prove_range_batch(n, P(v), P(lo), P(hi), 64, P(seeds), P(out), 1478, P(ln), P(st)) == 0
    ok = np.zeros(n, dtype=np.uint8)
    bad = out.copy(); bad[n // 2, 700] ^= 4                              # a scalar of the first inner proof: reaches the equations
    configs = [("clean", out, {})]
    if has_pass:
        configs += [("one_bad_segment_%d" % s, bad, {"ZKP_HIP_BP_LOCALISE_SEGMENT": str(s)}) for s in (16, 32, 64, 128)]
        configs += [("one_bad_default", bad, {}), ("one_bad_no_localise", bad, {"ZKP_HIP_BP_LOCALISE": "0"})]
    else:
        configs += [("one_bad_no_localise", bad, {})]
    times, did = {c[0]: [] for c in configs}, {}
    for name, buf, cfg in configs:                                       # warm-up, verdicts, what the call did
        call(cfg, n, buf, ln, lo, hi, ok); counters()
        call(cfg, n, buf, ln, lo, hi, ok)
        did[name] = counters()
        assert ok.sum() == (n if buf is out else n - 1) and (buf is out or ok[n // 2] == 0), name
    for _ in range(args.rounds):
        for name, buf, cfg in configs:
            times[name].append(call(cfg, n, buf, ln, lo, hi, ok))
    row = {"envelopes": n, "jobs": 2 * n}
    for name, _, _ in configs:
        t = sorted(times[name])
        row[name] = {"ms_median": round(t[len(t) // 2], 3), "ms_min": round(t[0], 3), "ms_max": round(t[-1], 3)}
        if did[name] is not None:
            row[name].update(did[name])
    rows.append(row)
res = {"tool": "tools/bench_bp_localise.py", "entry": "zkp_hip_verify_range_batch", "library": args.lib or "this tree's",
       "timing": "host wall clock around the call, median / min / max of %d, configurations alternating, host buffers" % args.rounds, "rows": rows}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
L.zkp_hip_shutdown()
