"""Groth16 verification through the C ABI at several batch sizes, with the batch check (g16_rlc.h: one pairing check per call) and with
the per-envelope check: where the default threshold (ZKP_HIP_G16_BATCH_VERIFY_MIN) belongs and what the batch check buys above it.  Each mode
runs in a child process.  Prints one JSON object (profiles/r04_verify_g16_batch.json).
Usage: verify_g16_batch_sweep.py [sizes ...] [--bad K ...] [--segment S ...] [--circuits equality,membership_16]

--bad K (repeatable; K an integer or "n/3"): K envelopes at fixed pseudo-random positions carry their neighbour's commitment (equality) or a
flipped set element (membership), so the batch check does not stand and the localisation pass runs (g16_localise.h); every row then also
carries the library's counters for one call (segment checks run, envelopes verified again, host ms after the failed check) when the library
has them.  --segment S sets ZKP_HIP_G16_LOCALISE_SEGMENT for the batch-check mode.  ZKP_HIP_LIB=<path> loads another build of the library,
such as the parent commit's, to compare against (profiles/verify_g16_localise.json)."""
import json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(argv):
    sizes, bad, segs, circuits, it = [], [], [], ["equality", "membership_16"], iter(argv)
    for a in it:
        if a == "--bad":
            bad.append(next(it))
        elif a == "--segment":
            segs.append(int(next(it)))
        elif a == "--circuits":
            circuits = next(it).split(",")
        elif a.isdigit():
            sizes.append(int(a))
    return sizes or [2048, 4096, 8192, 10240, 12288, 16384, 32768, 65536], bad or ["0"], segs, circuits


SIZES, BAD, SEGMENTS, CIRCUITS = _args(sys.argv[1:])


def bad_positions(m, k):
    """k distinct positions in [0, m): fixed for (m, k), the same in every build and mode"""
    import numpy as np
    return np.sort(np.random.default_rng(1000003 * m + k).choice(m, k, replace=False)) if k else np.zeros(0, dtype=np.int64)


if "--child" in sys.argv:
    import ctypes
    import numpy as np
    sys.path.insert(0, ROOT)
    import libzkp_amd as z
    from libzkp_amd import _native, api
    L = _native.lib()
    _native.check(L.zkp_hip_init(0), "init")
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        api.install_proving_key(kind, open(os.path.join(ROOT, "tests", "golden", name), "rb").read())
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rng = np.random.default_rng(3)
    n0 = 4096
    vals = [int(x) for x in rng.integers(0, 2**63, n0)]
    ep = z.prove_equality_batch(vals, vals)
    buf = np.zeros((n0, 298), dtype=np.uint8)
    for i, e in enumerate(ep): buf[i] = np.frombuffer(e, dtype=np.uint8)
    sets = [[int(x) for x in rng.choice(2**40, 16, replace=False)] for _ in range(1024)]
    mp = z.prove_membership_batch([s[3] for s in sets], sets)
    ml = len(mp[0]); mbuf = np.zeros((1024, ml), dtype=np.uint8)
    for i, e in enumerate(mp): mbuf[i] = np.frombuffer(e, dtype=np.uint8)

    def counters():
        ms, la, ad = ctypes.c_double(), ctypes.c_uint64(), ctypes.c_uint64()
        if L.zkp_hip_profile_read_kernel(3, ctypes.byref(ms), ctypes.byref(la), ctypes.byref(ad), 1) != 0:
            return None                                                   # a build without ZKP_HIP_COUNTER_G16_VERIFY
        return {"segment_checks": int(la.value), "envelopes_verified_again": int(ad.value), "ms_after_failed_check": round(ms.value, 2)}

    out = {c: {} for c in CIRCUITS}
    for name, src, width, fn in (("equality", buf, 298, L.zkp_hip_verify_equality_batch), ("membership_16", mbuf, ml, L.zkp_hip_verify_membership_batch)):
        if name not in CIRCUITS:
            continue
        for m in SIZES:
            for kb in BAD:
                k = m // 3 if kb == "n/3" else int(kb)
                big = np.ascontiguousarray(src[np.arange(m) % src.shape[0]]); bl = np.full(m, width, dtype=np.uint32); ok = np.zeros(m, dtype=np.uint8)
                pos = bad_positions(m, k)
                if name == "equality":
                    big[pos, 266:298] = big[(pos + 1) % m, 266:298]          # the neighbour's commitment (4096 distinct values, cycled: never its own)
                else:
                    big[pos, 14] ^= 1                                        # a set element
                ts = []
                for _ in range(6):
                    t0 = time.perf_counter(); _native.check(fn(m, P(big), width, P(bl), P(ok)), "verify"); ts.append(time.perf_counter() - t0)
                    c = counters()
                want = np.ones(m, dtype=bool); want[pos] = False
                assert (ok.astype(bool) == want).all()
                ts = sorted(t * 1e3 for t in ts[1:])
                row = {"ms": round(ts[0], 2), "median_ms": round(ts[2], 2), "max_ms": round(ts[-1], 2)}
                if c is not None and k:
                    row["last_call"] = c
                out[name]["%d/%s" % (m, kb)] = row
    print(json.dumps(out))
    sys.exit(0)

modes = [("batch_check", {"ZKP_HIP_G16_BATCH_VERIFY_MIN": "1"})]
modes += [("batch_check_segment_%d" % s, {"ZKP_HIP_G16_BATCH_VERIFY_MIN": "1", "ZKP_HIP_G16_LOCALISE_SEGMENT": str(s)}) for s in SEGMENTS]
modes += [("per_envelope", {"ZKP_HIP_NO_BATCH_VERIFY": "1"})]
res = {}
child = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
for mode, env in modes:
    o = subprocess.run(child, env=dict(os.environ, **env), capture_output=True, text=True, timeout=1100)
    if o.returncode != 0:
        sys.stderr.write(o.stderr[-3000:]); sys.exit(1)
    res[mode] = json.loads(o.stdout.strip().splitlines()[-1])
rows = []
for kind in CIRCUITS:
    for s in SIZES:
        for kb in BAD:
            key = "%d/%s" % (s, kb)
            b, p = res["batch_check"][kind][key], res["per_envelope"][kind][key]
            row = {"circuit": kind, "envelopes": s, "batch_check_ms": b["ms"], "per_envelope_ms": p["ms"], "batch_check_envelopes_per_s": round(s / b["ms"] * 1e3), "per_envelope_envelopes_per_s": round(s / p["ms"] * 1e3)}
            if BAD != ["0"]:
                row.update({"bad": kb, "batch_check_median_ms": b["median_ms"], "batch_check_max_ms": b["max_ms"], "per_envelope_median_ms": p["median_ms"], "per_envelope_max_ms": p["max_ms"]})
                if "last_call" in b:
                    row["batch_check_last_call"] = b["last_call"]
                for sg in SEGMENTS:
                    r = res["batch_check_segment_%d" % sg][kind][key]
                    row["segment_%d_ms" % sg] = r["ms"]
                    if "last_call" in r:
                        row["segment_%d_last_call" % sg] = r["last_call"]
            rows.append(row)
print(json.dumps({"tool": "tools/verify_g16_batch_sweep.py", "library": os.environ.get("ZKP_HIP_LIB", "this tree's build"), "entry": "zkp_hip_verify_equality_batch / zkp_hip_verify_membership_batch",
                  "timing": "host wall clock, best / median / worst of 5 after one warm-up call, host buffers in, verdict bytes out; --bad K envelopes tampered (default: all valid)", "rows": rows}))
