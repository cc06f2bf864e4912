#!/usr/bin/env python3
"""Time of the mixed verifier (zkp_hip_verify_envelopes, include/libzkp_hip_verify.h) on the metric's 4096-op mixed batch, proved once.

  C level   new:      the batch's envelopes, packed as zkp_hip_process_batch wrote them, through ONE zkp_hip_verify_envelopes call
            baseline: the SUM of the per-scheme zkp_hip_verify_*_batch calls on the same envelopes ALREADY bucketed into rows (the
                      bucketing, which a caller of the per-scheme calls has to do on the host, is not timed: that favours the baseline)
  Python    verify_proofs_parallel of this build against the parent commit's: a checkout of the parent with its library built
            (--parent-tree DIR), run in a process of its own under ZKP_HIP_LIB=DIR/libzkp_amd/lib/libzkp_hip.so with DIR's composite.py.
            Without --parent-tree that comparison is left out and the result says so.

Protocol: the two sides alternate on one box, one untimed call each first, medians of --reps (9) timed calls.
Writes one JSON object to --out (profiles/verify_mixed.json) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_SERVER = r"""
import json, os, sys, time
sys.path.insert(0, sys.argv[1])
import libzkp_amd as z
import libzkp_amd.api as api
from libzkp_amd import _native
gold = os.path.join(sys.argv[2], "tests", "golden")
for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
    api.install_proving_key(kind, open(os.path.join(gold, name), "rb").read())
envs = [bytes.fromhex(h) for h in json.load(open(sys.argv[3]))]
names = {1: "range", 2: "equality", 3: "threshold", 4: "membership", 5: "improvement", 6: "consistency"}
pairs = [(e, names[e[1]]) for e in envs]
rel = lambda p: os.path.relpath(p, sys.argv[1])          # inside the tree this process imports from
print(json.dumps({"lib": rel(_native.LIB_PATH), "composite": rel(z.composite.__file__)}), flush=True)
for line in sys.stdin:
    t0 = time.perf_counter()
    ok = z.verify_proofs_parallel(pairs)
    dt = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"ms": dt, "all": all(ok), "n": len(ok)}), flush=True)
"""


class Server:
    """verify_proofs_parallel of one tree in a process of its own: one timed call per request"""

    def __init__(self, tree, env_file, lib=None):
        env = dict(os.environ)
        if lib:
            env["ZKP_HIP_LIB"] = lib
        self.p = subprocess.Popen([sys.executable, "-c", _SERVER, tree, ROOT, env_file], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env=env)
        self.info = json.loads(self.p.stdout.readline())

    def call(self):
        self.p.stdin.write("go\n"); self.p.stdin.flush()
        r = json.loads(self.p.stdout.readline())
        assert r["all"], "verify_proofs_parallel rejected an honest envelope"
        return r["ms"]

    def close(self):
        self.p.stdin.close()
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="checkout of the parent commit with libzkp_amd/lib/libzkp_hip.so built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_mixed.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import libzkp_amd.api as api
    from libzkp_amd import _native, workloads as wl
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "zkp_hip_init")
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        api.install_proving_key(kind, open(os.path.join(ROOT, "tests", "golden", name), "rb").read())
    P = lambda x: x.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    n = a.ops
    ops, lists, seeds = wl.mixed_ops(n, 5)
    cap = wl.max_output_bytes(ops)
    blob, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    assert L.zkp_hip_process_batch(n, P(ops), P(lists), P(seeds), P(blob), cap, P(off), P(st)) == 0 and not st.any(), _native.last_error()
    envs = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]

    # the baseline's rows, bucketed here, outside the timed region (api._rows is what the per-scheme Python front ends use)
    def rows(scheme, cap_):
        sel = [e for e in envs if e[1] == scheme]
        buf, lens, stride = api._rows(sel, cap_)
        return sel, buf, lens, stride, np.zeros(len(sel), dtype=np.uint8)
    rg, eq, me, im = rows(1, 4096), rows(2, 4096), rows(4, 4096), rows(5, 8192)
    mins = np.array([int.from_bytes(e[10:18], "little") for e in rg[0]], dtype=np.uint64)
    maxs = np.array([int.from_bytes(e[18:26], "little") for e in rg[0]], dtype=np.uint64)
    olds = np.array([int.from_bytes(e[10:18], "little") for e in im[0]], dtype=np.uint64)

    def baseline():
        t0 = time.perf_counter()
        rcs = (L.zkp_hip_verify_range_batch(len(rg[0]), P(rg[1]), rg[3], P(rg[2]), P(mins), P(maxs), P(rg[4])),
               L.zkp_hip_verify_equality_batch(len(eq[0]), P(eq[1]), eq[3], P(eq[2]), P(eq[4])),
               L.zkp_hip_verify_membership_batch(len(me[0]), P(me[1]), me[3], P(me[2]), P(me[4])),
               L.zkp_hip_verify_improvement_batch(len(im[0]), P(im[1]), im[3], P(im[2]), P(olds), P(im[4])))
        dt = (time.perf_counter() - t0) * 1e3
        assert rcs == (0, 0, 0, 0) and all((r[4] == 1).all() for r in (rg, eq, me, im)), (rcs, _native.last_error())
        return dt

    packed = np.ascontiguousarray(blob[:int(off[n])])
    ok = np.zeros(n, dtype=np.uint8)

    def mixed():
        ok[:] = 0
        t0 = time.perf_counter()
        rc = L.zkp_hip_verify_envelopes(n, P(packed), P(off), None, P(ok))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and (ok == 1).all(), (rc, _native.last_error())
        return dt

    baseline(); mixed()
    api.verify_mixed_counters(reset=True)
    tb, tm = [], []
    for _ in range(a.reps):
        tb.append(baseline()); tm.append(mixed())
    counters = api.verify_mixed_counters(reset=True)
    res = {
        "workload": "%d-op mixed batch (workloads.mixed_ops(n, 5)): range / equality / membership(16) / improvement, proved once" % n,
        "protocol": "one box, the two sides alternating, one untimed call each, medians of %d timed calls" % a.reps,
        "c_level": {
            "mixed_ms": statistics.median(tm), "baseline_sum_ms": statistics.median(tb), "ratio": statistics.median(tm) / statistics.median(tb),
            "mixed_all_ms": tm, "baseline_all_ms": tb,
            "baseline": "sum of the four per-scheme zkp_hip_verify_*_batch calls on rows bucketed outside the timed region",
            "mixed_counters_over_the_timed_calls": counters,
        },
    }
    if a.parent_tree:
        import tempfile
        parent = os.path.abspath(a.parent_tree)
        with tempfile.NamedTemporaryFile("w", suffix=".json", delete=False) as f:
            json.dump([e.hex() for e in envs], f)
        api.shutdown()                                   # this process lets go of the GPU's tables before two more processes build theirs
        this, old = Server(ROOT, f.name), Server(parent, f.name, os.path.join(parent, "libzkp_amd", "lib", "libzkp_hip.so"))
        this.call(); old.call()
        tt, to = [], []
        for _ in range(a.reps):
            to.append(old.call()); tt.append(this.call())
        this.close(); old.close()
        os.unlink(f.name)
        res["python_level"] = {"this_build_ms": statistics.median(tt), "parent_ms": statistics.median(to), "ratio": statistics.median(tt) / statistics.median(to),
                               "this_build_all_ms": tt, "parent_all_ms": to, "this_build": this.info, "parent": old.info,
                               "call": "verify_proofs_parallel on the %d (envelope, type name) pairs" % n}
    else:
        res["python_level"] = "not measured: no --parent-tree given"
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
