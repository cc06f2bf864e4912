#!/usr/bin/env python3
"""Time of the statement verifier (zkp_stmt_verify, include/libzkp_hip_statements.h) on the metric's 4096-op mixed batch, proved once.

  (a)  zkp_stmt_verify on the clean list: the prover's ops and its packed output, one call
  (b)  zkp_hip_verify_envelopes on the same list: THE YARDSTICK -- the same spine without the statements (unchanged code)
  (c)  today's way to (a)'s answer: the per-scheme Python calls with their host comparisons -- verify_range_batch(p, mins, maxs),
       verify_equality_with_commitment_batch(p, snark_commit_value_batch(values)), verify_membership_batch(p, sets),
       verify_improvement_batch(p, olds) -- on envelopes bucketed by scheme outside the timed region (that favours (c))
  (a') (a) with every statement wrong: every envelope is refused before it gets a row, so this is the classification and the binds alone

Protocol: one process, the four alternating, one untimed call each first, medians of --reps (7) timed calls.
Writes one JSON object to --out (profiles/verify_ops.json) and prints it."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_ops.json"))
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
    packed = np.ascontiguousarray(blob[:int(off[n])])
    envs = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    ok, why = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)

    def statements(the_ops, the_lists, want_ok, want_why):
        ok[:] = 9; why[:] = 9
        t0 = time.perf_counter()
        rc = L.zkp_stmt_verify(n, P(the_ops), P(the_lists), len(the_lists), P(packed), P(off), P(ok), P(why))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and (ok == want_ok).all() and (why == want_why).all(), (rc, _native.last_error())
        return dt

    def envelopes():
        ok[:] = 0
        t0 = time.perf_counter()
        rc = L.zkp_hip_verify_envelopes(n, P(packed), P(off), None, P(ok))
        dt = (time.perf_counter() - t0) * 1e3
        assert rc == 0 and (ok == 1).all(), (rc, _native.last_error())
        return dt

    # every statement wrong: max + 1, (v + 1, v + 1), every set element with bit 40 set, old + 1
    wrong_ops, wrong_lists = ops.copy(), lists.copy()
    wrong_ops["c"][ops["kind"] == wl.OP_RANGE] += np.uint64(1)
    for f in ("a", "b"):
        wrong_ops[f][ops["kind"] == wl.OP_EQUALITY] += np.uint64(1)
    wrong_ops["a"][ops["kind"] == wl.OP_IMPROVEMENT] += np.uint64(1)
    wrong_lists |= np.uint64(1 << 40)

    # (c): bucketed here, outside the timed region
    by = {k: [i for i in range(n) if ops["kind"][i] == k] for k in (wl.OP_RANGE, wl.OP_EQUALITY, wl.OP_MEMBERSHIP, wl.OP_IMPROVEMENT)}
    pr = {k: [envs[i] for i in idx] for k, idx in by.items()}
    mins, maxs = ops["b"][by[wl.OP_RANGE]].copy(), ops["c"][by[wl.OP_RANGE]].copy()
    values, olds = ops["a"][by[wl.OP_EQUALITY]].copy(), ops["a"][by[wl.OP_IMPROVEMENT]].copy()
    sets = [[int(x) for x in lists[int(ops["list_off"][i]): int(ops["list_off"][i]) + int(ops["count"][i])]] for i in by[wl.OP_MEMBERSHIP]]

    def per_scheme():
        t0 = time.perf_counter()
        got = (api.verify_range_batch(pr[wl.OP_RANGE], mins, maxs),
               api.verify_equality_with_commitment_batch(pr[wl.OP_EQUALITY], api.snark_commit_value_batch(values)),
               api.verify_membership_batch(pr[wl.OP_MEMBERSHIP], sets),
               api.verify_improvement_batch(pr[wl.OP_IMPROVEMENT], olds))
        dt = (time.perf_counter() - t0) * 1e3
        assert all(all(g) for g in got)
        return dt

    sides = {"stmt_verify_ms": lambda: statements(ops, lists, 1, 0), "verify_envelopes_ms": envelopes, "per_scheme_python_ms": per_scheme,
             "stmt_verify_all_statements_wrong_ms": lambda: statements(wrong_ops, wrong_lists, 0, _native.STMT_STATEMENT)}
    for f in sides.values():
        f()
    api.verify_statements_counters(reset=True)
    times = {k: [] for k in sides}
    for _ in range(a.reps):
        for k, f in sides.items():
            times[k].append(f())
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {
        "workload": "%d-op mixed batch (workloads.mixed_ops(n, 5)): range / equality / membership(16) / improvement, proved once" % n,
        "protocol": "one process, the four sides alternating, one untimed call each, medians of %d timed calls" % a.reps,
        "medians": med, "all": times,
        "stmt_minus_envelopes_ms": med["stmt_verify_ms"] - med["verify_envelopes_ms"],
        "stmt_over_envelopes": med["stmt_verify_ms"] / med["verify_envelopes_ms"],
        "per_scheme_python_over_stmt": med["per_scheme_python_ms"] / med["stmt_verify_ms"],
        "statement_counters_over_the_timed_calls": api.verify_statements_counters(reset=True),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
