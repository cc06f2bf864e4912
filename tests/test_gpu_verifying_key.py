"""A verifier-only Groth16 key: zkp_hip_groth16_load_key given the VerifyingKey that leads a proving key file (the content of a
`{prefix}_vk.bin`) loads what verification reads and nothing else.  Keys are process state, so every case runs in a fresh child process
(this file run as a script) under its own timeout, one at a time; the child prints one JSON line.  Envelopes travel between children
through a file in the test's temporary directory."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PK_FILES = {0: "equality_mimc_pk.bin", 1: "membership_mimc_pk.bin"}
N_IC = {0: 2, 1: 2 + 2 * 64}
# libzkp_amd/csrc/g16_steps.h: the verifier's gamma_abc_g1 tables have radix 2^10 = 26 windows of 512 entries, 20 words per affine G1
# entry, and hold one more point than gamma_abc_g1 (alpha, for the batch check)
G16V_WBITS, G16V_NWIN, G16V_NENT, ENTRY_WORDS = 10, 26, 512, 20
KNOBS = ("ZKP_HIP_G16_WBITS", "ZKP_HIP_G16_TABLE_BUDGET_MB", "ZKP_HIP_G16_BATCH_VERIFY_MIN", "ZKP_HIP_G16_BATCH_VERIFY_ONLY", "ZKP_HIP_G16_VERIFY_VM",
         "ZKP_HIP_NO_BATCH_VERIFY", "LIBZKP_SNARK_KEY_DIR")
E_ARGUMENT = -3


def vk_table_bytes(kind):
    return (N_IC[kind] + 1) * G16V_NWIN * G16V_NENT * ENTRY_WORDS * 4


_stop = []          # why no further child may be started: a child that timed out, aborted or crashed may have left the GPU in a bad state


def run_child(case, *args, timeout=600, **env):
    assert not _stop, "no further GPU child is started after: %s" % _stop[0]
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(env)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case] + [str(a) for a in args], env=e, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _stop.append("child %r timed out after %d s" % (case, timeout))
        raise
    if r.returncode in (124, 134, 137, 139) or r.returncode < 0:
        _stop.append("child %r ended with status %d" % (case, r.returncode))
    assert r.returncode == 0, (case, env, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------- the tests (one child at a time)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def proved(tmp_path_factory):
    """Child A: the golden PROVING keys, envelopes under fixed seeds, tampered copies, and the verdicts of all of them."""
    path = str(tmp_path_factory.mktemp("vk") / "envelopes.json")
    r = run_child("prove", path, timeout=900)
    assert r["failures"] == [], r
    return path, r


def test_verdicts_equal_those_under_the_proving_key(proved):
    """Every batch of child A -- valid envelopes, each kind of tampering, points at infinity -- gets the identical verdicts in a process
    that loaded only the key prefixes: through the Fq2 machine and its fallback (default switches), through the one-pairing batch check,
    and through the lane-per-chain kernels alone."""
    path, a = proved
    want = a["verdicts"]
    assert all(v is True for name in a["all_valid"] for v in want[name]) and any(v is False for v in want["eq_mixed"]), want
    assert not any(want["eq_infinity"][:3]), want                    # (checked against the proving-key process below like the rest)
    r = run_child("verify_vk", path)
    assert r["failures"] == [] and r["verdicts"] == want, r
    r = run_child("verify_vk", path, ZKP_HIP_G16_VERIFY_VM="0")
    assert r["failures"] == [] and r["verdicts"] == want, r
    r = run_child("verify_vk", path, ZKP_HIP_G16_BATCH_VERIFY_MIN="1")
    assert r["failures"] == [] and r["verdicts"] == want, r
    # the batch check alone (no per-envelope pass behind it): stands for the all-valid lists, refuses the list with one bad envelope
    r = run_child("verify_vk", path, ZKP_HIP_G16_BATCH_VERIFY_MIN="1", ZKP_HIP_G16_BATCH_VERIFY_ONLY="1")
    for name in a["all_valid"]:
        assert r["verdicts"][name] == want[name], (name, r)
    assert isinstance(r["verdicts"]["eq_one_bad"], str) and "batch check did not stand" in r["verdicts"]["eq_one_bad"], r
    assert isinstance(r["verdicts"]["mem_one_bad"], str) and "batch check did not stand" in r["verdicts"]["mem_one_bad"], r


def test_key_info_and_memory_of_a_verifier_only_key():
    r = run_child("info_vk")
    assert r["failures"] == [], r
    for kind in (0, 1):
        assert r["info"][str(kind)] == [0, G16V_WBITS, 0, vk_table_bytes(kind)], r
    p8 = run_child("info_pk", ZKP_HIP_G16_WBITS="8")
    assert p8["failures"] == [] and p8["info"]["0"][:3] == [0, 8, 0], p8
    print("device memory taken by zkp_hip_groth16_load_key: verifying key %s, proving key at radix 2^8 %s" % (r["taken"], p8["taken"]))
    assert r["taken"]["0"] < p8["taken"]["0"], (r["taken"], p8["taken"])          # equality: less than the smallest prover configuration
    # membership: the 131-point radix-2^10 table of gamma_abc_g1 is larger than the prover's radix-2^8 tables; both figures are printed above


def test_proving_is_refused_and_everything_else_works():
    r = run_child("refuse")
    assert r["failures"] == [], r


def test_upgrade_and_downgrade(proved):
    path, a = proved
    r = run_child("updown", path)
    assert r["failures"] == [], r
    assert r["info_vk"] == [0, G16V_WBITS, 0, vk_table_bytes(0)] and r["info_vk_again"] == r["info_vk"], r
    # the MSM tables of the default radix: 20 x 4096 entries for each of the circuit's hundreds of key points, against 26 x 512 for three
    assert r["info_pk"][0] == 0 and r["info_pk"][3] > 16 * vk_table_bytes(0), r
    assert r["freed_by_downgrade"] > r["info_pk"][3] * 0.9, r                    # ... which the verifying key gives back


def test_two_shards_on_one_gpu(proved):
    path, a = proved
    r = run_child("shards", path)
    assert r["failures"] == [], r
    assert r["info"] == [[0, G16V_WBITS, 0, vk_table_bytes(0)]] * 2, r
    assert r["verdicts_shard1"] == a["verdicts"]["eq_mixed"], r


def test_malformed_verifying_keys(proved):
    path, a = proved
    r = run_child("malformed", path)
    assert r["failures"] == [], r
    for name, (rc, msg) in r["loads"].items():
        assert rc == E_ARGUMENT and msg, (name, rc, msg)
    for name in ("eq_offered_as_membership", "mem_offered_as_equality", "eq_gamma_at_infinity", "eq_abc_at_infinity", "mem_gamma_at_infinity",
                 "mem_abc_at_infinity", "eq_one_byte_fewer", "mem_one_byte_fewer"):
        assert "verifying key" in r["loads"][name][1], (name, r["loads"][name])
    assert r["verdicts_after"] == a["verdicts"]["eq_mixed"], r


def test_python_key_directory_with_only_verifying_keys(proved, tmp_path):
    path, a = proved
    d = tmp_path / "keys"
    d.mkdir()
    r = run_child("python", path, d, timeout=900)
    assert r["failures"] == [], r


def test_python_prove_first_in_a_verifiers_directory_raises_and_leaves_the_files(tmp_path):
    d = tmp_path / "keys"
    d.mkdir()
    r = run_child("python_prove_first", d)
    assert r["failures"] == [], r


# ---------------------------------------------------------------------------------------------------- child side
def _lib():
    sys.path.insert(0, ROOT)
    from libzkp_amd import _native
    return _native.lib(), _native


def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _pk(kind):
    with open(os.path.join(ROOT, "tests", "golden", PK_FILES[kind]), "rb") as f:
        return f.read()


def _vk(kind):
    return _pk(kind)[:64 + 384 + 8 + 64 * N_IC[kind]]


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


def _seeds(tag, n):
    return np.random.default_rng(tag).integers(0, 256, 32 * n, dtype=np.uint8)


def _prove_equality(L, vals, tag):
    n = len(vals)
    v = np.array(vals, dtype=np.uint64)
    out, lens, st = np.zeros((n, 298), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_prove_equality_batch(n, _P(v), _P(v), _P(_seeds(tag, n)), _P(out), 298, _P(lens), _P(st))
    return rc, [out[i, :lens[i]].tobytes() for i in range(n)]


def _prove_membership(L, values, sets, tag):
    n = len(values)
    v = np.array(values, dtype=np.uint64)
    flat = np.array([x for s in sets for x in s], dtype=np.uint64)
    counts = np.array([len(s) for s in sets], dtype=np.uint32)
    stride = 10 + 4 + 8 * 64 + 256 + 32
    out, lens, st = np.zeros((n, stride), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_prove_membership_batch(n, _P(v), _P(flat), _P(counts), _P(_seeds(tag, n)), _P(out), stride, _P(lens), _P(st))
    return rc, [out[i, :lens[i]].tobytes() for i in range(n)]


def _verify(L, kind, envs):
    """verdict list, or the error message of a call that failed"""
    n = len(envs)
    stride = max(max(len(e) for e in envs), 1)
    buf, lens, ok = np.zeros((n, stride), dtype=np.uint8), np.array([len(e) for e in envs], dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    for i, e in enumerate(envs):
        buf[i, :len(e)] = np.frombuffer(e, dtype=np.uint8)
    fn = L.zkp_hip_verify_equality_batch if kind == 0 else L.zkp_hip_verify_membership_batch
    rc = fn(n, _P(buf), stride, _P(lens), _P(ok))
    if rc != 0:
        return "error %d: %s" % (rc, L.zkp_hip_last_error().decode(errors="replace"))
    return [bool(x) for x in ok]


def _flip(env, at, bit=1):
    b = bytearray(env)
    b[at] ^= bit
    return bytes(b)


def _batches(eq, mem):
    """name -> (kind, envelopes).  eq: 40 equality envelopes; mem: membership envelopes of set sizes 1, 5, 64, 5, 64, 1.
    Equality envelope: 10-byte header | A 64 | B 128 | C 64 | commitment 32."""
    inf_a = bytearray(eq[20]); inf_a[10:74] = bytes(63) + b"\x40"
    inf_b = bytearray(eq[21]); inf_b[74:202] = bytes(127) + b"\x40"
    inf_c = bytearray(eq[22]); inf_c[202:266] = bytes(63) + b"\x40"
    scheme = bytearray(eq[9]); scheme[1] = 4
    mixed = list(eq[:8]) + [_flip(eq[8], 10 + 5), _flip(eq[9], 74 + 70, 4), _flip(eq[10], 202 + 33, 2), _flip(eq[11], 266 + 7),
                            eq[12][:266] + eq[13][266:], eq[14][:-1], bytes(scheme), eq[15]]
    one_bad = list(eq)
    one_bad[17] = eq[17][:266] + eq[18][266:]                         # a valid proof under another envelope's commitment
    m5 = mem[1]
    mem_mixed = list(mem) + [_flip(m5, 14 + 9), _flip(m5, 14 + 40 + 100), _flip(m5, len(m5) - 3), m5[:-1], bytes([2, 2]) + m5[2:]]
    mem_one_bad = list(mem)
    mem_one_bad[3] = _flip(mem[3], 14 + 3)                             # a set element
    return {"eq_valid_1": (0, eq[:1]), "eq_valid_40": (0, eq), "mem_valid": (1, mem), "eq_mixed": (0, mixed), "eq_one_bad": (0, one_bad),
            "eq_infinity": (0, [bytes(inf_a), bytes(inf_b), bytes(inf_c)] + list(eq[:5])), "mem_mixed": (1, mem_mixed), "mem_one_bad": (1, mem_one_bad)}


ALL_VALID = ["eq_valid_1", "eq_valid_40", "mem_valid"]
EQ_VALUES = [int(x) for x in np.random.default_rng(2024).integers(0, 2**63, 40, dtype=np.uint64)]
MEM_SETS = [[int(x) for x in np.random.default_rng(2025 + k).choice(2**48, k, replace=False)] for k in (1, 5, 64, 5, 64, 1)]
MEM_VALUES = [s[(3 * i) % len(s)] for i, s in enumerate(MEM_SETS)]


def _load_batches(path):
    with open(path) as f:
        return {name: (kind, [bytes.fromhex(h) for h in hexes]) for name, (kind, hexes) in json.load(f).items()}


def _range_improvement_matches_oracle(L, fails):
    """a range + improvement zkp_hip_process_batch against oracle/c's port"""
    import __graft_entry__ as ge
    from libzkp_amd import workloads as wl
    orc = ctypes.CDLL(ge.ORACLE_LIB)
    orc.zkp_oracle_init()
    r_ops, _, _ = wl.range_ops(6, 31)
    i_ops, _, _ = wl.improvement_ops(4, 32)
    ops = np.concatenate([r_ops[:3], i_ops[:2], r_ops[3:], i_ops[2:]])
    n = len(ops)
    lists, sd = np.zeros(1, dtype=np.uint64), wl.op_seeds(33, n)
    cap = wl.max_output_bytes(ops)
    res = []
    for fn, extra in ((L.zkp_hip_process_batch, ()), (orc.zkp_oracle_process_batch, (4,))):
        ob, off, stt = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        rc = fn(ctypes.c_uint64(n), _P(ops), _P(lists), _P(sd), _P(ob), ctypes.c_uint64(cap), _P(off), _P(stt), *extra)
        res.append((rc, ob[:int(off[n])].tobytes(), off.tolist(), stt.tolist()))
    if res[0] != res[1] or res[0][0] != 0:
        fails.append("range + improvement batch differs from the oracle (rc %d: %s)" % (res[0][0], L.zkp_hip_last_error().decode(errors="replace")))


def child(case, args):
    L, native = _lib()
    err = lambda: L.zkp_hip_last_error().decode(errors="replace")  # noqa: E731
    out, fails = {}, []
    out["failures"] = fails
    if case == "prove":
        assert L.zkp_hip_init(0) == 0, err()
        for kind in (0, 1):
            blob = _pk(kind)
            assert L.zkp_hip_groth16_load_key(kind, blob, len(blob)) == 0, err()
        rc, eq = _prove_equality(L, EQ_VALUES, 1)
        rc2, mem = _prove_membership(L, MEM_VALUES, MEM_SETS, 2)
        if rc or rc2:
            fails.append("proving failed: " + err())
        batches = _batches(eq, mem)
        with open(args[0], "w") as f:
            json.dump({name: [kind, [e.hex() for e in envs]] for name, (kind, envs) in batches.items()}, f)
        out["verdicts"] = {name: _verify(L, kind, envs) for name, (kind, envs) in batches.items()}
        out["all_valid"] = ALL_VALID
    elif case == "verify_vk":
        assert L.zkp_hip_init(0) == 0, err()
        for kind in (0, 1):
            blob = _vk(kind)
            if L.zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
                fails.append("loading the verifying key of circuit %d failed: %s" % (kind, err()))
        out["verdicts"] = {name: _verify(L, kind, envs) for name, (kind, envs) in _load_batches(args[0]).items()} if not fails else {}
    elif case in ("info_vk", "info_pk"):
        assert L.zkp_hip_init(0) == 0, err()
        # one verification-free warm-up of the allocator and the streams the loader uses, so that the figures are the key's own
        if L.zkp_hip_snark_commit_value_batch(1, _P(np.array([7], dtype=np.uint64)), _P(np.zeros(32, dtype=np.uint8))) != 0:
            fails.append("snark_commit_value failed: " + err())
        out["info"], out["taken"] = {}, {}
        for kind in (0, 1):
            blob = _vk(kind) if case == "info_vk" else _pk(kind)
            before = _free(L)
            if L.zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
                fails.append("load_key failed: " + err())
            out["taken"][str(kind)] = before - _free(L)
            out["info"][str(kind)] = _info(L, kind)
    elif case == "refuse":
        from libzkp_amd import workloads as wl
        from oracle.py import groth16 as g
        assert L.zkp_hip_init(0) == 0, err()
        # MiMC commitments in a process that never loaded a proving key
        vals = np.array([0, 1, 2**64 - 1, 123456789], dtype=np.uint64)
        cm = np.zeros((4, 32), dtype=np.uint8)
        if L.zkp_hip_snark_commit_value_batch(4, _P(vals), _P(cm)) != 0 or any(cm[i].tobytes() != g.commit_value_snark(int(vals[i])) for i in range(4)):
            fails.append("snark_commit_value before any key: " + err())
        blob = _vk(0)
        assert L.zkp_hip_groth16_load_key(0, blob, len(blob)) == 0, err()
        blob = _pk(1)                                                  # the other circuit keeps its proving key
        assert L.zkp_hip_groth16_load_key(1, blob, len(blob)) == 0, err()
        want = "only a verifying key is loaded for this circuit"
        rc, _ = _prove_equality(L, EQ_VALUES[:3], 1)
        if rc != E_ARGUMENT or want not in err():
            fails.append("prove_equality_batch on a verifier-only key: rc %d, %s" % (rc, err()))
        e_ops, e_lists, e_sd = wl.equality_ops(4, 7)
        n = len(e_ops); cap = wl.max_output_bytes(e_ops)
        ob, off, stt = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        rc = L.zkp_hip_process_batch(ctypes.c_uint64(n), _P(e_ops), _P(e_lists), _P(e_sd), _P(ob), ctypes.c_uint64(cap), _P(off), _P(stt))
        if rc != E_ARGUMENT or want not in err():
            fails.append("process_batch with an equality op: rc %d, %s" % (rc, err()))
        h = ctypes.c_void_p()
        L.zkp_hip_batch_stage.restype = ctypes.c_int
        rc = L.zkp_hip_batch_stage(ctypes.c_uint64(n), _P(e_ops), _P(e_lists), _P(e_sd), ctypes.byref(h))
        if rc != E_ARGUMENT or want not in err():
            fails.append("batch_stage with an equality op: rc %d, %s" % (rc, err()))
        m_ops, m_lists, m_sd = wl.mixed_ops(8, 5)                       # equality ops among the others: the whole batch is refused
        n = len(m_ops); cap = wl.max_output_bytes(m_ops)
        ob, off, stt = np.zeros(cap, dtype=np.uint8), np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.int32)
        rc = L.zkp_hip_process_batch(ctypes.c_uint64(n), _P(m_ops), _P(m_lists), _P(m_sd), _P(ob), ctypes.c_uint64(cap), _P(off), _P(stt))
        if rc != E_ARGUMENT or want not in err():
            fails.append("process_batch of a mixed batch: rc %d, %s" % (rc, err()))
        # the circuit that has its proving key proves, and its envelopes verify
        rc, mem = _prove_membership(L, MEM_VALUES, MEM_SETS, 2)
        if rc != 0 or _verify(L, 1, mem) != [True] * len(mem):
            fails.append("membership (proving key loaded) beside a verifier-only equality key: rc %d, %s" % (rc, err()))
        _range_improvement_matches_oracle(L, fails)
        if L.zkp_hip_snark_commit_value_batch(4, _P(vals), _P(cm)) != 0 or any(cm[i].tobytes() != g.commit_value_snark(int(vals[i])) for i in range(4)):
            fails.append("snark_commit_value beside a verifier-only key: " + err())
        # now membership verifier-only as well
        blob = _vk(1)
        assert L.zkp_hip_groth16_load_key(1, blob, len(blob)) == 0, err()
        rc, _ = _prove_membership(L, MEM_VALUES, MEM_SETS, 2)
        if rc != E_ARGUMENT or want not in err():
            fails.append("prove_membership_batch on a verifier-only key: rc %d, %s" % (rc, err()))
        if _verify(L, 1, mem) != [True] * len(mem):
            fails.append("membership envelopes proved before the downgrade do not verify after it")
    elif case == "updown":
        batches = _load_batches(args[0])
        assert L.zkp_hip_init(0) == 0, err()
        blob = _vk(0)
        assert L.zkp_hip_groth16_load_key(0, blob, len(blob)) == 0, err()
        out["info_vk"] = _info(L, 0)
        blob = _pk(0)
        assert L.zkp_hip_groth16_load_key(0, blob, len(blob)) == 0, err()           # the process becomes a prover
        out["info_pk"] = _info(L, 0)
        rc, eq = _prove_equality(L, EQ_VALUES, 1)
        if rc != 0 or eq != batches["eq_valid_40"][1]:
            fails.append("proofs after verifying key -> proving key differ from a process that loaded the proving key directly (rc %d)" % rc)
        before = _free(L)
        blob = _vk(0)
        assert L.zkp_hip_groth16_load_key(0, blob, len(blob)) == 0, err()           # ... and a verifier again: the MSM tables go
        out["freed_by_downgrade"] = _free(L) - before
        out["info_vk_again"] = _info(L, 0)
        if _verify(L, 0, eq) != [True] * len(eq):
            fails.append("verification after the downgrade failed")
        rc, _ = _prove_equality(L, EQ_VALUES[:2], 1)
        if rc != E_ARGUMENT:
            fails.append("proving after the downgrade: rc %d" % rc)
    elif case == "shards":
        batches = _load_batches(args[0])
        devs = (ctypes.c_int * 2)(0, 0)
        assert L.zkp_hip_init_devices(2, devs) == 0, err()
        blob = _vk(0)
        assert L.zkp_hip_groth16_load_key(0, blob, len(blob)) == 0, err()
        infos = []
        for s in (0, 1):
            L.zkp_hip_use_device(s)
            infos.append(_info(L, 0))
        out["info"] = infos
        L.zkp_hip_use_device(1)
        out["verdicts_shard1"] = _verify(L, 0, batches["eq_mixed"][1])
        rc, _ = _prove_equality(L, EQ_VALUES[:2], 1)
        if rc != E_ARGUMENT:
            fails.append("proving on shard 1: rc %d" % rc)
    elif case == "malformed":
        batches = _load_batches(args[0])
        assert L.zkp_hip_init(0) == 0, err()

        def inf_at(blob, end):
            b = bytearray(blob)
            b[end - 1] = (b[end - 1] & 0x3F) | 0x40
            return bytes(b)

        e, m = _vk(0), _vk(1)
        bad = {"eq_offered_as_membership": (1, e), "mem_offered_as_equality": (0, m),
               "eq_gamma_at_infinity": (0, inf_at(e, 320)), "eq_abc_at_infinity": (0, inf_at(e, len(e))),
               "mem_gamma_at_infinity": (1, inf_at(m, 320)), "mem_abc_at_infinity": (1, inf_at(m, 456 + 64 * 77)),
               "eq_one_byte_fewer": (0, e[:-1]), "mem_one_byte_fewer": (1, m[:-1]),
               "eq_one_byte_more": (0, _pk(0)[:len(e) + 1]), "mem_one_byte_more": (1, _pk(1)[:len(m) + 1])}
        assert L.zkp_hip_groth16_load_key(0, e, len(e)) == 0, err()
        free0 = _free(L)
        out["loads"] = {}
        for name, (kind, blob) in bad.items():
            rc = L.zkp_hip_groth16_load_key(kind, blob, len(blob))
            out["loads"][name] = [rc, err() if rc else ""]
        # a failed load leaves nothing behind: not the key it replaced either
        got = _verify(L, 0, batches["eq_valid_1"][1])
        if not (isinstance(got, str) and got.startswith("error -3")):
            fails.append("verification after a failed load: %r" % (got,))
        if _free(L) + (2 << 20) < free0:          # (free0 was taken with the 3.2 MB key loaded that the first failed load released)
            fails.append("failed loads left %d bytes of device memory behind" % (free0 - _free(L)))
        assert L.zkp_hip_groth16_load_key(0, e, len(e)) == 0, err()
        out["verdicts_after"] = _verify(L, 0, batches["eq_mixed"][1])
    elif case == "python":
        batches = _load_batches(args[0])
        keydir = args[1]
        files = {}
        for kind, prefix in ((0, "equality_mimc"), (1, "membership_mimc")):
            files[prefix + "_vk.bin"] = _vk(kind)
            with open(os.path.join(keydir, prefix + "_vk.bin"), "wb") as f:
                f.write(_vk(kind))
        import libzkp_amd as z
        from libzkp_amd import api, composite
        api.set_snark_key_dir(keydir)
        eq, mem = batches["eq_valid_40"][1], batches["mem_valid"][1]
        if not all(z.verify_equality(eq[i], EQ_VALUES[i], EQ_VALUES[i]) for i in range(3)):
            fails.append("verify_equality")
        if z.verify_equality(_flip(eq[3], 100), EQ_VALUES[3], EQ_VALUES[3]):
            fails.append("verify_equality accepted a tampered envelope")
        if not all(z.verify_membership(mem[i], MEM_SETS[i]) for i in range(len(mem))):
            fails.append("verify_membership")
        got = composite.verify_proofs_parallel([(eq[0], "equality"), (mem[1], "membership"), (_flip(eq[1], 50), "equality"), (eq[2], "membership")])
        if got != [True, True, False, False]:
            fails.append("verify_proofs_parallel: %r" % (got,))
        if not composite.verify_composite_proof(composite.create_composite_proof([eq[4], mem[2], eq[5]])):
            fails.append("verify_composite_proof")
        if composite.verify_composite_proof(composite.create_composite_proof([eq[4], _flip(mem[2], 300)])):
            fails.append("verify_composite_proof accepted a tampered member")
        if api.export_verifying_key(0) != _vk(0) or api.export_verifying_key(1) != _vk(1):
            fails.append("export_verifying_key")
        try:
            z.prove_equality(5, 5)
            fails.append("prove_equality did not raise")
        except api.ZkpBackendError as ex:
            if "proving key" not in str(ex) or "equality_mimc_pk.bin" not in str(ex):
                fails.append("prove_equality raised: %s" % ex)
        api.shutdown()                                                 # the verifying keys are kept and reinstalled
        if not z.verify_equality(eq[6], EQ_VALUES[6], EQ_VALUES[6]):
            fails.append("verify_equality after shutdown()")
        try:
            z.prove_membership(MEM_SETS[1][0], MEM_SETS[1])
            fails.append("prove_membership did not raise")
        except api.ZkpBackendError:
            pass
        now = {name: open(os.path.join(keydir, name), "rb").read() for name in sorted(os.listdir(keydir))}
        if now != files:
            fails.append("the key directory changed: %s" % sorted(now))
        # install_verifying_key over install_proving_key and back
        api.install_proving_key(0, _pk(0))
        if api.export_verifying_key(0) != _vk(0) or len(z.prove_equality(9, 9)) != 298:
            fails.append("install_proving_key after a verifying key")
        api.install_verifying_key(0, _vk(0))
        if not z.verify_equality(eq[7], EQ_VALUES[7], EQ_VALUES[7]):
            fails.append("verify_equality after install_verifying_key")
    elif case == "python_prove_first":
        keydir = args[0]
        with open(os.path.join(keydir, "equality_mimc_vk.bin"), "wb") as f:
            f.write(_vk(0))
        import libzkp_amd as z
        from libzkp_amd import api
        api.set_snark_key_dir(keydir)
        try:
            z.prove_equality(5, 5)                                     # the first Groth16 call of the process: no setup over the directory's key
            fails.append("prove_equality did not raise")
        except api.ZkpBackendError as ex:
            if "equality_mimc_pk.bin" not in str(ex):
                fails.append("prove_equality raised: %s" % ex)
        if os.listdir(keydir) != ["equality_mimc_vk.bin"] or open(os.path.join(keydir, "equality_mimc_vk.bin"), "rb").read() != _vk(0):
            fails.append("the key directory changed: %s" % sorted(os.listdir(keydir)))
        if len(z.prove_membership(3, [1, 3])) == 0 or sorted(os.listdir(keydir)) != ["equality_mimc_vk.bin", "membership_mimc_pk.bin", "membership_mimc_vk.bin"]:
            fails.append("the circuit without any key file did not get its fresh setup")
    else:
        raise SystemExit("unknown case " + case)
    L.zkp_hip_shutdown()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    child(sys.argv[1], sys.argv[2:])
