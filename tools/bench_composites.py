"""Cost of verifying a list of composite proofs in one call (libzkp_amd.verify_composite_proofs -> zkp_hip_verify_composites) beside the
loop of verify_composite_proof over the same containers, which is all there was before.  Shapes:

  a256, a4096   256 / 4096 containers of one range envelope and three metadata entries each
  b8x1000       8 containers of 1000 range envelopes each
  c4mib         one container of exactly 4 MiB, digest only (integrity_only): the worst case of the lane-per-container digest kernel

Per shape: the new call (Python front end, and the C entry point alone), the digest kernel alone (between two events:
ZKP_HIP_COMPOSITES_DIGEST_LOG), the loop of verify_composite_proof (shape c: verify_composite_proof_integrity_only) in a child process --
on another build of the library when --parent-lib names one, such as the parent commit's -- and one-thread hashlib over the same hashed
bytes.  Medians of --reps timed repetitions (at least 20) after two warm-up calls; host wall clock around calls that end in a device
synchronise.  One process per library, one GPU.  Prints one JSON object (profiles/composites.json is this output).

  python tools/bench_composites.py [--reps 20] [--shapes a256,a4096,b8x1000,c4mib] [--parent-lib other/libzkp_hip.so] [--out file.json]"""
import argparse, ctypes, hashlib, json, os, pickle, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", default="a256,a4096,b8x1000,c4mib")
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--loop", default=None, help=argparse.SUPPRESS)          # the child: the per-container loop over the containers pickled in this file
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps: at least 20")


def median_ms(ts):
    ts = sorted(ts)
    return {"ms_median": round(1e3 * ts[len(ts) // 2], 4), "ms_min": round(1e3 * ts[0], 4), "ms_max": round(1e3 * ts[-1], 4)}


def timed(fn, reps):
    for _ in range(2):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    return median_ms(ts)


import libzkp_amd as z
from libzkp_amd import _native, composite

if args.loop:
    shapes = pickle.load(open(args.loop, "rb"))
    _native.check(_native.lib().zkp_hip_init(0), "zkp_hip_init")
    res = {}
    for name, (containers, integrity_only) in shapes.items():
        one = z.verify_composite_proof_integrity_only if integrity_only else z.verify_composite_proof
        assert all(one(c) for c in containers), name
        res[name] = timed(lambda: [one(c) for c in containers], args.reps)
    print(json.dumps(res))
    z.shutdown()
    sys.exit(0)

import numpy as np
L = _native.lib()
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
VP = ctypes.c_void_p
u32 = lambda x: int(x).to_bytes(4, "little")


def range_envelopes(n, salt):
    rng = np.random.default_rng(salt)
    v = [int(x) for x in rng.integers(0, 2**32, n)]
    return z.prove_range_batch(v, [0] * n, [2**32] * n, seeds=bytes(rng.integers(0, 256, 32 * n, dtype=np.uint8)))


def build(name):
    if name.startswith("a"):
        n = int(name[1:])
        envs = range_envelopes(n, n)
        return [composite._serialize_composite([e], {"issuer": b"bench", "index": u32(i), "note": bytes(i % 50)}) for i, e in enumerate(envs)], False
    if name == "b8x1000":
        envs = range_envelopes(8000, 8)
        return [composite._serialize_composite(envs[1000 * i:1000 * i + 1000], {}) for i in range(8)], False
    if name == "c4mib":
        fake = lambda n, s: bytes([2, 9]) + u32(n - 10) + u32(0) + bytes((s + 7 * k) & 0xff for k in range(n - 10))          # noqa: E731
        proofs = [fake(900000, s) for s in range(4)] + [fake((4 << 20) - 12 - 5 * 4 - 32 - 4 * 900000 - 500, 4)]
        room = (4 << 20) - (12 + sum(4 + len(p) for p in proofs) + 32)
        c = composite._serialize_composite(proofs, {"k": bytes(room - 9)})
        assert len(c) == 4 << 20
        return [c], True
    raise SystemExit("unknown shape " + name)


def hashed_stream(c):
    proofs, meta = composite.parse_composite(c)
    return b"COMPOSITE_PROOF:" + u32(len(proofs)) + b"".join(proofs) + b"".join(u32(len(k.encode())) + k.encode() + u32(len(meta[k])) + meta[k] for k in sorted(meta))


names = args.shapes.split(",")
shapes = {name: build(name) for name in names}
rows = {}
for name, (containers, integrity_only) in shapes.items():
    n = len(containers)
    row = {"containers": n, "envelopes": sum(len(composite.parse_composite(c)[0]) for c in containers), "bytes": sum(len(c) for c in containers), "integrity_only": integrity_only}
    assert z.verify_composite_proofs(containers, integrity_only=integrity_only) == [True] * n, name
    row["new_call_python"] = timed(lambda: z.verify_composite_proofs(containers, integrity_only=integrity_only), args.reps)
    blob = np.frombuffer(b"".join(containers), dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(c) for c in containers]))).astype(np.uint64)
    status = np.zeros(n, dtype=np.uint8)
    call = lambda: _native.check(L.zkp_hip_verify_composites(n, blob.ctypes.data_as(VP), off.ctypes.data_as(VP), 1 if integrity_only else 0, status.ctypes.data_as(VP)), "zkp_hip_verify_composites")  # noqa: E731
    row["new_call_c"] = timed(call, args.reps)
    with tempfile.NamedTemporaryFile("r", suffix=".jsonl") as log:          # the digest kernel alone, in repetitions of their own
        os.environ["ZKP_HIP_COMPOSITES_DIGEST_LOG"] = log.name
        for _ in range(args.reps + 2):
            call()
        del os.environ["ZKP_HIP_COMPOSITES_DIGEST_LOG"]
        lines = [json.loads(ln) for ln in log.read().splitlines()][2:]
    row["hashed_bytes"] = lines[0]["hashed_bytes"]
    row["digest_kernel"] = median_ms([1e-3 * ln["digest_kernel_ms"] for ln in lines])
    streams = [hashed_stream(c) for c in containers]
    assert sum(len(s) for s in streams) == row["hashed_bytes"]
    row["hashlib_one_thread"] = timed(lambda: [hashlib.sha256(s).digest() for s in streams], args.reps)
    row["counters"] = z.verify_composites_counters(reset=True)
    rows[name] = row

with tempfile.NamedTemporaryFile("wb", suffix=".pkl") as f:
    pickle.dump(shapes, f); f.flush()
    env = dict(os.environ)
    if args.parent_lib:
        env["ZKP_HIP_LIB"] = os.path.abspath(args.parent_lib)
    z.shutdown()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop", f.name, "--reps", str(args.reps)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    loop = json.loads(r.stdout.strip().splitlines()[-1])
for name, row in rows.items():
    row["per_container_loop"] = loop[name]
    row["loop_over_new_call"] = round(loop[name]["ms_median"] / row["new_call_python"]["ms_median"], 3)
lib_hash = lambda p: hashlib.sha256(open(p, "rb").read()).hexdigest()[:16]          # noqa: E731
res = {"tool": "tools/bench_composites.py", "build": lib_hash(_native.LIB_PATH),
       "loop_library": {"path": args.parent_lib or "this tree's", "build": lib_hash(args.parent_lib or _native.LIB_PATH)},
       "timing": "host wall clock around the call, median / min / max of %d after 2 warm-up calls; digest_kernel: hipEventElapsedTime around k_comp_digest" % args.reps,
       "rows": rows}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
