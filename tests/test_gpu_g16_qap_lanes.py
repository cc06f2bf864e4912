"""The Groth16 QAP step with one lane per proof row (libzkp_amd/csrc/g16_steps.h: g16_qap_pass_pair / g16_qap_pass_single, k_g16_qap_pass
in g16_kernels.hip) on the GPU: prove_equality and prove_membership through the host-buffer entry points at 1, 65 and 257 rows -- a lone
lane, a partial second wave, a partial second 256-lane workgroup -- must give the bytes of oracle/c's prover for every proof.  Keys at radix
2^10 (ZKP_HIP_G16_WBITS=10: small tables, a short key load).  Every case runs in a fresh child process (this file run as a script) that
prints one JSON line.  Both pass shapes (ZKP_HIP_G16_QAP_SHAPE=2 | 3) and the default are run."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KNOBS = ("ZKP_HIP_G16_SHARE_AB", "ZKP_HIP_G16_WBITS", "ZKP_HIP_G16_TABLE_BUDGET_MB", "ZKP_HIP_G16_UNEVEN", "ZKP_HIP_ED_TABLES", "ZKP_HIP_G16_QAP_SHAPE")
ROWS = (1, 65, 257)
SET_SIZES = (1, 64, 7)            # row i of a membership batch has a set of SET_SIZES[i % 3] elements
OP_EQUALITY, OP_MEMBERSHIP = 2, 4
OP_DTYPE = np.dtype([("kind", "<u4"), ("count", "<u4"), ("a", "<u8"), ("b", "<u8"), ("c", "<u8"), ("list_off", "<u8")])

pytestmark = pytest.mark.gpu


def run_child(case, shape):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["ZKP_HIP_ED_TABLES"] = "lazy"          # no Bulletproofs call here: the generator tables are not built
    e["ZKP_HIP_G16_WBITS"] = "10"
    if shape:
        e["ZKP_HIP_G16_QAP_SHAPE"] = shape          # the most stages a pass fuses (g16_qap_lane_schedule); unset: the default shape
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (case, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("shape", ["", "2", "3"])
@pytest.mark.parametrize("case", ["equality", "membership"])
def test_proofs_at_1_65_257_rows_are_the_oracles_bytes(case, shape):
    r = run_child(case, shape)
    assert r["radix"] == [10, 10], r
    assert sorted(r["rows"]) == sorted(str(n) for n in ROWS), r
    for n in ROWS:
        got = r["rows"][str(n)]
        assert got["failures"] == [], (case, n, got)
        assert got["compared"] == n and got["differ"] == [], (case, n, got)


# ---------------------------------------------------------------------------------------------------- child side
def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _oracle_batch(orc, ops, lists, seeds):
    n = len(ops)
    cap = int(sum(298 if o["kind"] == OP_EQUALITY else 10 + 4 + 8 * int(o["count"]) + 256 + 32 for o in ops))
    out, off, st = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
    rc = orc.zkp_oracle_process_batch(ctypes.c_uint64(n), _P(ops), _P(lists), _P(seeds), _P(out), ctypes.c_uint64(cap), _P(off), _P(st), 16)
    assert rc == 0 and not st.any(), (rc, st)
    return [out[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]


def _equality(L, orc, n, fails):
    rng = np.random.default_rng(300 + n)
    v = rng.integers(0, 2**64, n, dtype=np.uint64)
    v[0] = 2**64 - 1
    if n > 1:
        v[1] = 0
    sd = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, 298), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_equality_batch(n, _P(v), _P(v), _P(sd), _P(out), 298, _P(lens), _P(st)) != 0 or st.any() or not (lens == 298).all():
        fails.append("equality rows=%d failed" % n)
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["kind"], ops["a"], ops["b"] = OP_EQUALITY, v, v
    want = _oracle_batch(orc, ops, np.zeros(1, dtype=np.uint64), sd)
    return [i for i in range(n) if out[i].tobytes() != want[i]]


def _membership(L, orc, n, fails):
    rng = np.random.default_rng(400 + n)
    cnt = np.array([SET_SIZES[i % 3] for i in range(n)], dtype=np.uint32)
    sets = [rng.choice(2**40, int(c), replace=False).astype(np.uint64) for c in cnt]
    sets[0][0] = 2**64 - 1                                           # a 64-bit extreme as the value of the first row
    vals = np.array([s[i % len(s)] for i, s in enumerate(sets)], dtype=np.uint64)
    flat = np.ascontiguousarray(np.concatenate(sets))
    sd = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    stride = 10 + 4 + 8 * 64 + 256 + 32
    out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_membership_batch(n, _P(vals), _P(flat), _P(cnt), _P(sd), _P(out), stride, _P(lens), _P(st)) != 0 or st.any():
        fails.append("membership rows=%d failed" % n)
    ops = np.zeros(n, dtype=OP_DTYPE)
    ops["kind"], ops["count"], ops["a"] = OP_MEMBERSHIP, cnt, vals
    ops["list_off"] = np.concatenate(([0], np.cumsum(cnt)[:-1])).astype(np.uint64)
    want = _oracle_batch(orc, ops, flat, sd)
    return [i for i in range(n) if out[i, :int(lens[i])].tobytes() != want[i]]


def child(case):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    from libzkp_amd import _native
    L = _native.lib()
    orc = ctypes.CDLL(ge.ORACLE_LIB)
    orc.zkp_oracle_init()
    assert L.zkp_hip_init(0) == 0, L.zkp_hip_last_error()
    radix = []
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        blob = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
        assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, L.zkp_hip_last_error()
        assert orc.zkp_oracle_g16_load_key(kind, blob, ctypes.c_uint64(len(blob))) == 0
        w, u, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        assert L.zkp_hip_groth16_key_info(kind, ctypes.byref(w), ctypes.byref(u), ctypes.byref(b)) == 0
        radix.append(w.value)
    out = {"radix": radix, "rows": {}}
    for n in ROWS:
        fails = []
        differ = (_equality if case == "equality" else _membership)(L, orc, n, fails)
        out["rows"][str(n)] = {"failures": fails, "compared": n, "differ": differ[:8]}
    L.zkp_hip_shutdown()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    child(sys.argv[1])
