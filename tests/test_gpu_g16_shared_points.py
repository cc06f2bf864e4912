"""The key points the Groth16 sums A and B1 share (libzkp_amd/csrc/g16_share.h) on the GPU: with one slot and one table per shared
variable the proofs are the bytes they were with ZKP_HIP_G16_SHARE_AB=0 and the bytes of the oracle's toxic-waste prover, and a key
holds exactly 110 points' tables less.  The switch is read when a key is loaded, so a case loads the keys with it off, proves, loads
them again with it on and proves again.  Every case runs in a fresh child process (this file run as a script) that prints one JSON line."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KNOBS = ("ZKP_HIP_G16_SHARE_AB", "ZKP_HIP_G16_WBITS", "ZKP_HIP_G16_TABLE_BUDGET_MB", "ZKP_HIP_G16_UNEVEN", "ZKP_HIP_ED_TABLES")
SHARED = 110                      # variables of either committed key whose a_query and b_g1_query points are one point
ROWS = (1, 65, 257)               # one lane | a second wave | a second 256-lane row group with one live lane
SS = bytes(range(32))             # setup seed of the committed keys (tests/golden/gen_groth16_keys.py)


def run_child(case, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["ZKP_HIP_ED_TABLES"] = "lazy"          # no Bulletproofs call here: the generator tables are not built
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (case, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def table_bytes_of_shared_points(wbits, uneven):
    nwin, nent = (254 + wbits) // wbits, 1 << (wbits - 1)
    slot_ent = 18 * nent + 25088 if uneven else nwin * nent          # g16_steps.h: g16_radix
    return SHARED * slot_ent * 64                                     # 16 words per G1 entry of the MSM tables


def check_info(r, kinds=(0, 1)):
    for k in kinds:
        off, on = r["info"]["0"][str(k)], r["info"]["1"][str(k)]
        assert off[0] == 0 and on[0] == 0 and off[1:3] == on[1:3], (off, on)
        assert off[3] - on[3] == table_bytes_of_shared_points(on[1], on[2]), (k, off, on)


# ---------------------------------------------------------------------------------------------------- the tests (one child at a time)
pytestmark = pytest.mark.gpu


def test_rows_1_65_257_at_radix_2_10_match_the_switch_off_and_the_oracle():
    r = run_child("rows", ZKP_HIP_G16_WBITS="10")
    assert r["failures"] == [], r
    assert set(r["digest"]["0"]) == {"eq%d" % n for n in ROWS} | {"mem%d_set%d" % (n, s) for n in ROWS for s in (1, 64)}
    assert r["digest"]["0"] == r["digest"]["1"], r                   # byte-identical with ZKP_HIP_G16_SHARE_AB=0 and without it
    assert r["info"]["1"]["0"][1:3] == [10, 0]
    check_info(r)
    # the cases of tests/test_gpu_groth16.py against the oracle's toxic-waste prover (no MSM, no FFT); its keys are derived once per session
    from oracle.py import groth16 as g
    c = r["oracle_cases"]
    assert len(c["equality"]) == 13 and len(c["membership"]) == 6 and c["membership_status"] == [0, 0, 0, 0, 0, 0, 1, 1]
    rs = lambda seed: (g.draw_fr(seed, 0x47313600, 0), g.draw_fr(seed, 0x47313600, 1))  # noqa: E731
    for value, seed, got in c["equality"]:
        cm = g.commit_value_snark(value)
        cs = g.equality_circuit(value, value, int.from_bytes(cm, "little"))
        assert bytes.fromhex(got) == g.envelope(2, g.prove_with_trapdoor(g.equality_key(SS), cs, *rs(bytes.fromhex(seed))), cm), value
    for value, the_set, seed, got in c["membership"]:
        cm = g.commit_value_snark(value)
        sel, sv, ir = g.membership_inputs(value, the_set)
        cs = g.membership_circuit(value, sel, sv, ir, int.from_bytes(cm, "little"))
        pr = g.prove_with_trapdoor(g.membership_key(SS), cs, *rs(bytes.fromhex(seed)))
        assert bytes.fromhex(got) == g.envelope(4, len(the_set).to_bytes(4, "little") + b"".join(x.to_bytes(8, "little") for x in the_set) + pr, cm), value


def test_uneven_radix_2_14_under_a_table_budget():
    r = run_child("uneven", ZKP_HIP_G16_TABLE_BUDGET_MB="40000")          # the equality key alone: ~19 GB of tables
    assert r["info"]["0"]["0"][1:3] == [14, 1] and r["info"]["1"]["0"][1:3] == [14, 1], r
    assert r["failures"] == [] and r["digest"]["0"] == r["digest"]["1"] and len(r["digest"]["1"]) == 1, r
    check_info(r, kinds=(0,))


def test_default_radix_on_two_shards_of_one_gpu_that_share_the_tables():
    """The one case at the default radix, and the two-shard case, in one child: at 2^10 both keys' tables (a few GB) are no larger than what a
    shard holds of its own, so what a key load takes from the GPU could not tell one copy of the tables from two; at the default radix a
    second copy is tens of GB.  (The issue asks for 2^10 everywhere but one case; this is that case.)"""
    r = run_child("shards")                                             # no forced radix: the second shard adopts the first one's tables and radix
    assert r["failures"] == [], r
    assert r["digest"]["0"]["shard0"] == r["digest"]["0"]["shard1"] == r["digest"]["1"]["shard0"] == r["digest"]["1"]["shard1"], r
    assert r["info"]["1"]["shard0"] == r["info"]["1"]["shard1"] and r["info"]["0"]["shard0"] == r["info"]["0"]["shard1"], r
    for k in (0, 1):
        off, on = r["info"]["0"]["shard0"][k], r["info"]["1"]["shard0"][k]
        assert off[0] == 0 and on[0] == 0 and off[1:3] == on[1:3] and off[3] - on[3] == table_bytes_of_shared_points(on[1], on[2]), (off, on)
    # What loading the two keys into both shards took from the GPU: one copy of the tables and what each shard holds of its own (circuit,
    # verifier tables, the runtime's reservations for the streams the table builder first uses) -- the 8 GB that tests/test_gpu_groth16.py
    # allows a second shard.  A second copy would be another `tables` bytes: ~34 GB at 2^13.
    tables = r["info"]["1"]["shard0"][0][3] + r["info"]["1"]["shard0"][1][3]
    assert r["load_drop"] < tables + (8 << 30), r


# ---------------------------------------------------------------------------------------------------- child side
def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _lib():
    sys.path.insert(0, ROOT)
    from libzkp_amd import _native
    return _native.lib(), _native


def _keys():
    return [(kind, open(os.path.join(ROOT, "tests", "golden", name), "rb").read()) for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin"))]


def _load(L, share, kinds=(0, 1)):
    if share:
        os.environ.pop("ZKP_HIP_G16_SHARE_AB", None)
    else:
        os.environ["ZKP_HIP_G16_SHARE_AB"] = "0"
    for kind, blob in _keys():
        if kind in kinds:
            assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, L.zkp_hip_last_error()


def _info(L, kind):
    w, u, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = L.zkp_hip_groth16_key_info(kind, ctypes.byref(w), ctypes.byref(u), ctypes.byref(b))
    return [rc, w.value, u.value, b.value]


def _free(L):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    f = L.hipMemGetInfo
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_int
    assert f(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _equality(L, n, seed, fails):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 2**64, n, dtype=np.uint64)
    sd = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, 298), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_equality_batch(n, _P(v), _P(v), _P(sd), _P(out), 298, _P(lens), _P(st)) != 0 or st.any() or not (lens == 298).all():
        fails.append("equality rows=%d failed" % n)
    return out.tobytes()


def _membership(L, n, set_size, seed, fails):
    rng = np.random.default_rng(seed)
    sets = np.stack([rng.choice(2**40, set_size, replace=False) for _ in range(n)]).astype(np.uint64)
    vals = sets[np.arange(n), np.arange(n) % set_size].copy()
    cnt = np.full(n, set_size, dtype=np.uint32)
    sd = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    stride = 10 + 4 + 8 * set_size + 256 + 32
    out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    flat = np.ascontiguousarray(sets.ravel())
    if L.zkp_hip_prove_membership_batch(n, _P(vals), _P(flat), _P(cnt), _P(sd), _P(out), stride, _P(lens), _P(st)) != 0 or st.any() or not (lens == stride).all():
        fails.append("membership rows=%d set=%d failed" % (n, set_size))
    return out.tobytes()


def _digest(b):
    return hashlib.sha256(b).hexdigest()


def _oracle_cases(L, fails):
    """The inputs of tests/test_gpu_groth16.py's bit-exact cases and the proofs of the shared layout for them: the parent compares"""
    rng = np.random.default_rng(11)
    n = 70
    v = rng.integers(0, 2**63, n, dtype=np.uint64)
    v[:4] = [42, 0, 2**64 - 1, 1]
    seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, 320), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_equality_batch(n, _P(v), _P(v), _P(seeds), _P(out), 320, _P(lens), _P(st)) != 0:
        fails.append("equality cases failed")
    res = {"equality": [[int(v[i]), seeds[32 * i: 32 * i + 32].tobytes().hex(), out[i, :298].tobytes().hex()] for i in list(range(12)) + [n - 1]]}
    cases = [(25, [10, 20, 25, 30, 40]), (5, [5]), (9, [7, 9, 9]), (63, list(range(64))), (0, [3, 0]), (2**64 - 1, [1, 2**64 - 1]), (4, [1, 2, 3]), (1, [])]
    vals = np.array([c[0] for c in cases], dtype=np.uint64)
    flat = np.array([x for c in cases for x in c[1]] + [0], dtype=np.uint64)
    cnt = np.array([len(c[1]) for c in cases], dtype=np.uint32)
    n = len(cases)
    seeds = (np.arange(32 * n, dtype=np.uint32) * 5 + 2).astype(np.uint8)
    stride = 10 + 4 + 8 * 64 + 256 + 32
    out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_membership_batch(n, _P(vals), _P(flat), _P(cnt), _P(seeds), _P(out), stride, _P(lens), _P(st)) != 1:
        fails.append("membership cases: unexpected return value")
    res["membership_status"] = [int(x) for x in st]
    res["membership"] = [[cases[i][0], cases[i][1], seeds[32 * i: 32 * i + 32].tobytes().hex(), out[i, : lens[i]].tobytes().hex()] for i in range(6)]
    return res


def child(case):
    L, native = _lib()
    fails, out = [], {"digest": {"0": {}, "1": {}}, "info": {"0": {}, "1": {}}}
    if case == "shards":
        devs = (ctypes.c_int * 2)(0, 0)
        assert L.zkp_hip_init_devices(2, devs) == 0, L.zkp_hip_last_error()
        for share in (1, 0):
            before = _free(L)
            _load(L, bool(share))
            if share:
                out["load_drop"] = before - _free(L)
            for s in (0, 1):
                L.zkp_hip_use_device(s)
                out["info"][str(share)]["shard%d" % s] = [_info(L, 0), _info(L, 1)]
                out["digest"][str(share)]["shard%d" % s] = _digest(_equality(L, 65, 5, fails) + _membership(L, 65, 16, 6, fails))
            L.zkp_hip_use_device(0)
    else:
        assert L.zkp_hip_init(0) == 0, L.zkp_hip_last_error()
        kinds = (0,) if case == "uneven" else (0, 1)          # uneven 2^14: the equality key alone
        for share in (0, 1):
            _load(L, bool(share), kinds)
            for k in kinds:
                out["info"][str(share)][str(k)] = _info(L, k)
            d = out["digest"][str(share)]
            if case == "rows":
                for n in ROWS:
                    d["eq%d" % n] = _digest(_equality(L, n, 100 + n, fails))
                    for s in (1, 64):
                        d["mem%d_set%d" % (n, s)] = _digest(_membership(L, n, s, 200 + n + s, fails))
            else:
                d["eq65"] = _digest(_equality(L, 65, 165, fails))
        if case == "rows":
            out["oracle_cases"] = _oracle_cases(L, fails)
    out["failures"] = fails
    L.zkp_hip_shutdown()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    child(sys.argv[1])
