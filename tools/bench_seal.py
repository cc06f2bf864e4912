"""Cost of sealing a list of composite proofs in one call (libzkp_amd.create_composite_proofs -> libzkp_seal_composites;
libzkp_amd.process_ops_sealed -> libzkp_seal_batch) beside the path that was all there was before: the Python loop of
create_proof_with_metadata / _serialize_composite with hashlib, behind process_ops where the proofs come from a batch.  Shapes:

  c256, c4096     256 / 4096 containers of one range envelope and two metadata entries, envelopes already on the host:
                  create_composite_proofs against the loop of create_proof_with_metadata
  b4096x4096      4096 mixed ops sealed into 4096 containers of one proof with two metadata entries: process_ops_sealed against process_ops
                  followed by the loop
  b4096x64        the same ops sealed into 64 containers of 64 proofs
  w4mib           one container of exactly 4 MiB (fake envelopes): the worst case of the lane-per-container digest
  w8x1000         8 containers of 1000 range envelopes each

Per shape both paths run on the same inputs in this process, alternating, and their outputs are compared byte for byte before anything
is timed.  Medians of --reps timed repetitions (at least 20) after two warm-up calls of each; host wall clock around calls that end in a
device synchronise.  One GPU.  Prints one JSON object (profiles/composites_seal.json is this output).

  python tools/bench_seal.py [--reps 20] [--shapes c256,c4096,b4096x4096,b4096x64,w4mib,w8x1000] [--out file.json]"""
import argparse, hashlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--shapes", default="c256,c4096,b4096x4096,b4096x64,w4mib,w8x1000")
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.reps < 20:
    ap.error("--reps: at least 20")

import numpy as np
import libzkp_amd as z
from libzkp_amd import _native, api, composite

L = _native.lib()
_native.check(L.zkp_hip_init(0), "zkp_hip_init")
u32 = lambda x: int(x).to_bytes(4, "little")  # noqa: E731


def stats(ts):
    ts = sorted(ts)
    return {"ms_median": round(1e3 * ts[len(ts) // 2], 4), "ms_min": round(1e3 * ts[0], 4), "ms_max": round(1e3 * ts[-1], 4)}


def timed_pair(new, old, reps):
    """both paths alternating: (new, old)"""
    for _ in range(2):
        new(); old()
    tn, to = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); new(); tn.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); old(); to.append(time.perf_counter() - t0)
    return stats(tn), stats(to)


def range_envelopes(n, salt):
    rng = np.random.default_rng(salt)
    v = [int(x) for x in rng.integers(0, 2**32, n)]
    return z.prove_range_batch(v, [0] * n, [2**32] * n, seeds=bytes(rng.integers(0, 256, 32 * n, dtype=np.uint8)))


def mixed_ops(n, salt):
    """the flagship mix as op tuples: range, equality, membership, improvement in turn"""
    rng = np.random.default_rng(salt)
    ops = []
    for i in range(n):
        v = int(rng.integers(1000, 1000 + 2**20))
        if i % 4 == 0:
            ops.append(("range", v, 1000, 1000 + 2**20))
        elif i % 4 == 1:
            ops.append(("equality", v, v))
        elif i % 4 == 2:
            s = [int(x) for x in rng.choice(2**32, 8, replace=False)]
            ops.append(("membership", s[i % 8], s))
        else:
            ops.append(("improvement", v, v + 1 + i % 7))
    return ops, bytes(rng.integers(0, 256, 32 * n, dtype=np.uint8))


def loop(lists, metas):
    return [composite.create_proof_with_metadata(p[0], m) if len(p) == 1 else composite._serialize_composite(p, m) for p, m in zip(lists, metas)]


rows = {}
for name in args.shapes.split(","):
    if name in ("c256", "c4096"):
        n = int(name[1:])
        lists = [[e] for e in range_envelopes(n, n)]
        metas = [{"issuer": b"bench", "index": u32(i)} for i in range(n)]
        new, old = (lambda: z.create_composite_proofs(lists, metas)), (lambda: loop(lists, metas))
    elif name in ("b4096x4096", "b4096x64"):
        for kind, key in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
            api.install_proving_key(kind, open(os.path.join(ROOT, "tests", "golden", key), "rb").read())
        m = int(name.split("x")[1])
        ops, seeds = mixed_ops(4096, 4096)
        counts = [4096 // m] * m
        metas = [{"issuer": b"bench", "index": u32(i)} for i in range(m)]
        lists = None

        def old(ops=ops, seeds=seeds, counts=counts, metas=metas):
            envs = api.process_ops(ops, seeds)
            k = counts[0]
            return loop([envs[k * i:k * i + k] for i in range(len(counts))], metas)
        new = lambda ops=ops, seeds=seeds, counts=counts, metas=metas: z.process_ops_sealed(ops, counts, metas, seeds=seeds)  # noqa: E731
    elif name == "w4mib":
        fake = lambda n, s: bytes([2, 9]) + u32(n - 10) + u32(0) + bytes((s + 7 * k) & 0xff for k in range(n - 10))          # noqa: E731
        proofs = [fake(900000, s) for s in range(4)] + [fake((4 << 20) - 12 - 5 * 4 - 32 - 4 * 900000 - 500, 4)]
        room = (4 << 20) - (12 + sum(4 + len(p) for p in proofs) + 32)
        lists, metas = [proofs], [{"k": bytes(room - 9)}]
        new, old = (lambda: z.create_composite_proofs(lists, metas)), (lambda: loop(lists, metas))
    elif name == "w8x1000":
        envs = range_envelopes(8000, 8)
        lists, metas = [envs[1000 * i:1000 * i + 1000] for i in range(8)], [{} for _ in range(8)]
        new, old = (lambda: z.create_composite_proofs(lists, metas)), (lambda: loop(lists, metas))
    else:
        raise SystemExit("unknown shape " + name)
    z.seal_counters(reset=True)
    a, b = new(), old()
    assert a == b and all(x is not None for x in a), name          # the same bytes at the size that is timed
    c = z.seal_counters(reset=True)
    row = {"containers": len(a), "envelopes": c["envelopes"], "bytes": sum(len(x) for x in a), "sha256_of_all": hashlib.sha256(b"".join(a)).hexdigest()[:16]}
    row["new_call"], row["parent_path"] = timed_pair(new, old, args.reps)
    row["parent_over_new"] = round(row["parent_path"]["ms_median"] / row["new_call"]["ms_median"], 3)
    if name.startswith("b"):                                        # what the proving alone costs, for scale: the same ops, proofs fetched, nothing sealed
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter(); api.process_ops(ops, seeds); ts.append(time.perf_counter() - t0)
        row["process_ops_alone"] = stats(ts)
    row["counters_of_the_timed_calls"] = z.seal_counters(reset=True)
    rows[name] = row

lib_hash = hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16]
res = {"tool": "tools/bench_seal.py", "build": lib_hash,
       "new_call": "c*, w*: libzkp_amd.create_composite_proofs; b*: libzkp_amd.process_ops_sealed",
       "parent_path": "c*, w*: the Python loop of create_proof_with_metadata / _serialize_composite (hashlib); b*: process_ops followed by that loop",
       "timing": "host wall clock around the call (Python front end included on both sides), both paths alternating in one process, median / min / max of %d after 2 warm-up calls" % args.reps,
       "rows": rows}
print(json.dumps(res))
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
z.shutdown()
