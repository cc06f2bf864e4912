"""The Bulletproofs generator tables sized to free HBM (radix 2^10 .. 2^16, include/libzkp_hip.h: zkp_hip_init): the radix is chosen once
per process, so every case runs in a fresh child process (this file run as a script) with its knobs in the environment, one at a time;
the child prints one JSON line.  At a forced smaller radix the proofs, verdicts and mixed batches are byte-identical to the oracle's."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TABLE_BYTES = {16: 8724152320, 15: 4634705920, 14: 2589982720, 13: 1363148800, 12: 749731840, 11: 408944640, 10: 221511680}
KNOBS = ("ZKP_HIP_ED_WBITS", "ZKP_HIP_ED_TABLE_BUDGET_MB", "ZKP_HIP_ED_TABLES")


def run_child(case, timeout=600, **env):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), case], env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (case, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------- the tests (one child at a time)
pytestmark = pytest.mark.gpu


def test_default_radix_is_2_16():
    r = run_child("info")
    assert r["init"] == 0 and r["info"] == [0, 16, 0, TABLE_BYTES[16]], r


@pytest.mark.parametrize("wbits", [13, 10])
def test_forced_radix_matches_the_oracle(wbits):
    r = run_child("parity", timeout=900, ZKP_HIP_ED_WBITS=str(wbits))
    assert r["info"] == [0, wbits, 0, TABLE_BYTES[wbits]], r
    assert r["failures"] == [], r


def test_budget_and_bad_knobs():
    assert run_child("info", ZKP_HIP_ED_TABLE_BUDGET_MB="1500")["info"] == [0, 13, 0, TABLE_BYTES[13]]
    assert run_child("info", ZKP_HIP_ED_TABLE_BUDGET_MB="300")["info"] == [0, 10, 0, TABLE_BYTES[10]]
    r = run_child("info", ZKP_HIP_ED_TABLE_BUDGET_MB="100")
    assert r["init"] == -1 and "not enough device memory for the generator tables" in r["error"] and "2^10" in r["error"], r
    r = run_child("info", ZKP_HIP_ED_WBITS="9")
    assert r["init"] == -3 and "ZKP_HIP_ED_WBITS" in r["error"], r
    r = run_child("info", ZKP_HIP_ED_TABLES="sometimes")
    assert r["init"] == -3 and "ZKP_HIP_ED_TABLES" in r["error"], r


def test_lazy_build():
    r = run_child("lazy", ZKP_HIP_ED_TABLES="lazy")
    assert r["failures"] == [], r
    assert r["init_drop"] < (512 << 20), r
    assert r["info_after_init"][:2] == [0, 0] and r["info_after_init"][3] == 0, r
    assert r["info_after_g16_stark"][:2] == [0, 0] and r["info_after_g16_stark"][3] == 0, r
    assert r["info_after_prove"] == [0, 16, 0, TABLE_BYTES[16]], r
    assert r["free_after_shutdown"] + (64 << 20) >= r["free_before"], r


def test_two_shards_on_one_gpu_share_one_table():
    r = run_child("share")
    assert r["init"] == 0 and r["info"] == [[0, 16, 0, TABLE_BYTES[16]]] * 2, r
    assert r["drop"] < TABLE_BYTES[16] + (4 << 30), r          # one table (plus workspaces), not two


# ---------------------------------------------------------------------------------------------------- child side
def _lib():
    sys.path.insert(0, ROOT)
    from libzkp_amd import _native
    return _native.lib(), _native


def _info(L, shard=None):
    w, u, b = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    rc = L.zkp_hip_groth16_key_info(2, ctypes.byref(w), ctypes.byref(u), ctypes.byref(b))
    return [rc, w.value, u.value, b.value]


def _free(L):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    f = L.hipMemGetInfo
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    f.restype = ctypes.c_int
    assert f(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _oracle():
    import __graft_entry__ as ge
    orc = ctypes.CDLL(ge.ORACLE_LIB)
    orc.zkp_oracle_init()
    return orc


def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _flat(lists):
    return np.array([x for l in lists for x in l], dtype=np.uint64), np.array([len(l) for l in lists], dtype=np.uint32)


def _range_parity(L, orc, fails):
    """257 ops per width through the host-buffer prover, byte-compared; the verifiers' verdicts against the oracle's on them and on
    tampered copies"""
    U64 = ctypes.c_uint64
    for bits in (8, 16, 32, 64):
        n = 257
        rng = np.random.default_rng(bits)
        hi = 2**bits - 1 if bits < 64 else 2**64 - 1
        mn = np.zeros(n, dtype=np.uint64)
        mx = np.full(n, hi, dtype=np.uint64)
        v = rng.integers(0, hi, n, dtype=np.uint64, endpoint=True)
        v[0], v[1] = 0, hi
        seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
        stride = int(L.zkp_hip_range_proof_bytes(bits))
        out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        o2, l2, s2 = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
        rc = L.zkp_hip_prove_range_batch(n, _P(v), _P(mn), _P(mx), bits, _P(seeds), _P(out), stride, _P(lens), _P(st))
        orc.zkp_oracle_prove_range_batch(U64(n), _P(v), _P(mn), _P(mx), bits, _P(seeds), _P(o2), U64(stride), _P(l2), _P(s2), 16)
        if rc != 0 or not (out == o2).all() or not (lens == l2).all():
            fails.append("range %d-bit bytes differ from the oracle (rc %d)" % (bits, rc))
            continue
        t = out.copy()
        t[np.arange(0, n, 2), rng.integers(0, stride, (n + 1) // 2)] ^= 4
        for name, buf in (("good", out), ("tampered", t)):
            ok, ok2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
            if L.zkp_hip_verify_range_batch(n, _P(buf), stride, _P(lens), _P(mn), _P(mx), _P(ok)) != 0:
                fails.append("verify_range %s %d-bit failed: %s" % (name, bits, L.zkp_hip_last_error()))
                continue
            orc.zkp_oracle_verify_range_batch(U64(n), _P(buf), U64(stride), _P(lens), _P(mn), _P(mx), _P(ok2), 16)
            if not (ok == ok2).all() or (name == "good" and not ok.all()):
                fails.append("verify_range %s %d-bit verdicts differ from the oracle" % (name, bits))
    # 4096 envelopes, one tampered: the random-linear-combination check fails and the per-job path names the envelope
    n = 4096
    rng = np.random.default_rng(77)
    v = rng.integers(0, 2**32, n, dtype=np.uint64, endpoint=True)
    mn, mx = np.zeros(n, dtype=np.uint64), np.full(n, 2**32, dtype=np.uint64)
    seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, 1478), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_range_batch(n, _P(v), _P(mn), _P(mx), 64, _P(seeds), _P(out), 1478, _P(lens), _P(st)) != 0:
        fails.append("prove_range 4096 failed")
        return
    out[1234, 700] ^= 1
    ok, ok2 = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    L.zkp_hip_verify_range_batch(n, _P(out), 1478, _P(lens), _P(mn), _P(mx), _P(ok))
    orc.zkp_oracle_verify_range_batch(U64(n), _P(out), U64(1478), _P(lens), _P(mn), _P(mx), _P(ok2), 16)
    if not (ok == ok2).all() or ok[1234] or ok.sum() != n - 1:
        fails.append("batch verification of 4096 envelopes with one tampered differs from the oracle")


def _threshold_consistency_parity(L, orc, fails):
    U64 = ctypes.c_uint64
    rng = np.random.default_rng(5)
    lists = [[int(x) for x in rng.integers(0, 2**40, int(k))] for k in rng.integers(1, 6, 24)]
    thr = np.array([int(rng.integers(0, sum(l) + 1)) for l in lists], dtype=np.uint64)
    flat, counts = _flat(lists)
    n = len(lists)
    seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, 762), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_threshold_batch(n, _P(flat), _P(counts), _P(thr), 64, _P(seeds), _P(out), 762, _P(lens), _P(st)) != 0:
        fails.append("prove_threshold failed")
        return
    orc.zkp_oracle_verify_threshold.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64]
    ref, ol = ctypes.create_string_buffer(1024), ctypes.c_uint32()
    for i in range(n):
        vals = (ctypes.c_uint64 * len(lists[i]))(*lists[i])
        orc.zkp_oracle_prove_threshold(vals, len(lists[i]), U64(int(thr[i])), 64, seeds[32 * i: 32 * i + 32].tobytes(), ref, 1024, ctypes.byref(ol))
        if out[i, :762].tobytes() != ref.raw[:762]:
            fails.append("threshold op %d differs from the oracle" % i)
            break
    t = out.copy()
    t[np.arange(0, n, 2), rng.integers(0, 762, (n + 1) // 2)] ^= 2
    ok = np.zeros(n, dtype=np.uint8)
    L.zkp_hip_verify_threshold_batch(n, _P(t), 762, _P(lens), _P(thr), _P(ok))
    want = [orc.zkp_oracle_verify_threshold(t[i].tobytes(), 762, int(thr[i])) for i in range(n)]
    if list(ok) != want or not all(want[1::2]):
        fails.append("threshold verdicts differ from the oracle")
    data = [sorted(int(x) for x in rng.integers(0, 2**50, k)) for k in (1, 2, 3, 5, 8, 4)]
    flat, counts = _flat(data)
    n = len(data)
    stride = max(int(L.zkp_hip_consistency_proof_bytes(len(d))) for d in data)
    seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_consistency_batch(n, _P(flat), _P(counts), _P(seeds), _P(out), stride, _P(lens), _P(st)) != 0:
        fails.append("prove_consistency failed")
        return
    orc.zkp_oracle_verify_consistency.argtypes = [ctypes.c_char_p, ctypes.c_uint32]
    ref = ctypes.create_string_buffer(stride + 16)
    for i in range(n):
        d = (ctypes.c_uint64 * len(data[i]))(*data[i])
        orc.zkp_oracle_prove_consistency(d, len(data[i]), seeds[32 * i: 32 * i + 32].tobytes(), ref, stride + 16, ctypes.byref(ol))
        if lens[i] != ol.value or out[i, :lens[i]].tobytes() != ref.raw[:ol.value]:
            fails.append("consistency op %d differs from the oracle" % i)
            break
    t = out.copy()
    for i in range(1, n, 2):
        t[i, int(lens[i]) // 2] ^= 8
    ok = np.zeros(n, dtype=np.uint8)
    L.zkp_hip_verify_consistency_batch(n, _P(t), stride, _P(lens), _P(ok))
    want = [orc.zkp_oracle_verify_consistency(t[i, :lens[i]].tobytes(), int(lens[i])) for i in range(n)]
    if list(ok) != want or not all(want[0::2]):
        fails.append("consistency verdicts differ from the oracle")


def _load_golden_keys(L, orc):
    for kind, name in ((0, "equality_mimc_pk.bin"), (1, "membership_mimc_pk.bin")):
        blob = open(os.path.join(ROOT, "tests", "golden", name), "rb").read()
        assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0
        if orc is not None:
            assert orc.zkp_oracle_g16_load_key(kind, blob, ctypes.c_uint64(len(blob))) == 0


def _mixed_parity(L, orc, fails):
    from libzkp_amd import workloads as wl
    _load_golden_keys(L, orc)
    ops, lists, sd = wl.mixed_ops(512, 9)
    cap = wl.max_output_bytes(ops)
    res = []
    for fn, extra in ((L.zkp_hip_process_batch, ()), (orc.zkp_oracle_process_batch, (16,))):
        ob, off, stt = np.zeros(cap, dtype=np.uint8), np.zeros(513, dtype=np.uint64), np.zeros(512, dtype=np.int32)
        rc = fn(ctypes.c_uint64(512), _P(ops), _P(lists), _P(sd), _P(ob), ctypes.c_uint64(cap), _P(off), _P(stt), *extra)
        res.append((rc, ob[:int(off[512])].tobytes(), off.tolist(), stt.tolist()))
    if res[0] != res[1]:
        fails.append("512-op mixed batch differs from the oracle")


def _lazy_cycle(L, err, fails, out):
    free0 = _free(L)
    assert L.zkp_hip_init(0) == 0, err()
    out["init_drop"] = free0 - _free(L)
    out["info_after_init"] = _info(L)
    # Groth16 (golden key: prove and verify an equality proof) and a STARK prove: no generator tables
    _load_golden_keys(L, None)
    v1 = np.array([5, 9], dtype=np.uint64)
    eo, el, es = np.zeros((2, 298), dtype=np.uint8), np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.int32)
    if L.zkp_hip_prove_equality_batch(2, _P(v1), _P(v1), _P(np.zeros(64, dtype=np.uint8)), _P(eo), 298, _P(el), _P(es)) != 0:
        fails.append("equality prove failed: " + err())
    ok = np.zeros(2, dtype=np.uint8)
    if L.zkp_hip_verify_equality_batch(2, _P(eo), 298, _P(el), _P(ok)) != 0 or not ok.all():
        fails.append("equality verify failed")
    stride = int(L.zkp_hip_improvement_max_bytes())
    so, sl, ss = np.zeros((1, stride), dtype=np.uint8), np.zeros(1, dtype=np.uint32), np.zeros(1, dtype=np.int32)
    if L.zkp_hip_prove_improvement_batch(1, _P(np.array([3], dtype=np.uint64)), _P(np.array([8], dtype=np.uint64)), _P(so), stride, _P(sl), _P(ss)) != 0:
        fails.append("improvement prove failed")
    out["info_after_g16_stark"] = _info(L)
    # the first Bulletproofs call builds the tables; its bytes are the oracle's
    orc = _oracle()
    n = 16
    rng = np.random.default_rng(3)
    v = rng.integers(0, 2**32, n, dtype=np.uint64, endpoint=True)
    mn, mx = np.zeros(n, dtype=np.uint64), np.full(n, 2**32, dtype=np.uint64)
    seeds = rng.integers(0, 256, 32 * n, dtype=np.uint8)
    o1, l1, s1 = np.zeros((n, 1478), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    o2, l2, s2 = np.zeros((n, 1478), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    if L.zkp_hip_prove_range_batch(n, _P(v), _P(mn), _P(mx), 64, _P(seeds), _P(o1), 1478, _P(l1), _P(s1)) != 0:
        fails.append("prove_range failed: " + err())
    orc.zkp_oracle_prove_range_batch(ctypes.c_uint64(n), _P(v), _P(mn), _P(mx), 64, _P(seeds), _P(o2), ctypes.c_uint64(1478), _P(l2), _P(s2), 16)
    if not (o1 == o2).all():
        fails.append("lazily built tables: range bytes differ from the oracle")
    out["info_after_prove"] = _info(L)


def child(case):
    L, native = _lib()
    err = lambda: L.zkp_hip_last_error().decode(errors="replace")  # noqa: E731
    out = {}
    if case == "info":
        out["init"] = L.zkp_hip_init(0)
        out["error"] = err() if out["init"] else ""
        if out["init"] == 0:
            out["info"] = _info(L)
    elif case == "parity":
        assert L.zkp_hip_init(0) == 0, err()
        out["info"] = _info(L)
        orc = _oracle()
        fails = []
        _range_parity(L, orc, fails)
        _threshold_consistency_parity(L, orc, fails)
        _mixed_parity(L, orc, fails)
        out["failures"] = fails
    elif case == "lazy":
        # Three whole cycles: the HIP runtime keeps the scratch reservation of the queues the first cycles created (the pairing kernels'
        # 12 KB per lane; test_gpu_zz_lifecycle.py), so the memory figures are those of the third, steady-state cycle
        fails = []
        for _ in range(2):
            _lazy_cycle(L, err, fails, {})
            L.zkp_hip_shutdown()
        out["free_before"] = _free(L)
        _lazy_cycle(L, err, fails, out)
        L.zkp_hip_shutdown()
        out["free_after_shutdown"] = _free(L)
        out["failures"] = fails
    elif case == "share":
        before = _free(L)
        devs = (ctypes.c_int * 2)(0, 0)
        out["init"] = L.zkp_hip_init_devices(2, devs)
        out["drop"] = before - _free(L)
        infos = []
        for s in (0, 1):
            L.zkp_hip_use_device(s)
            infos.append(_info(L))
        out["info"] = infos
    L.zkp_hip_shutdown()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    child(sys.argv[1])
