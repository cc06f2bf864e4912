"""The Groth16 key check through the product: what zkp_hip_groth16_load_key now refuses and self-checks, and what check_key reports
(include/libzkp_hip_keycheck.h).  Keys are process state, so every case runs in a fresh child process (this file run as a script) under its
own timeout, one at a time; the child prints one JSON line.  Children run under ZKP_HIP_G16_WBITS=8, at which a key's tables are 33 MB.
Forged keys are made here by patching bytes of the golden keys at the offsets of the ark layout and travel to the children through files in
the test's temporary directory."""
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
G2_FINITE = {0: 224, 1: 416}          # 221 + 3 and 413 + 3: the finite b_g2_query points and beta, gamma, delta
KNOBS = ("ZKP_HIP_G16_WBITS", "ZKP_HIP_G16_TABLE_BUDGET_MB", "ZKP_HIP_G16_TABLE_CHECK", "ZKP_HIP_G16_TABLE_FLIP", "ZKP_HIP_G16_SHARE_AB", "LIBZKP_SNARK_KEY_DIR")
E_RUNTIME, E_ARGUMENT = -1, -3
# radix 2^8: 32 windows of 128 entries, 16 words per packed G1 entry; the verifier's tables: radix 2^10, 26 windows of 512 plain entries of 20 words
W8_NWIN, W8_NENT, G1_WORDS = 32, 128, 16
VK_NWIN, VK_NENT, VK_WORDS = 26, 512, 20

_stop = []          # why no further child may be started: a child that timed out, aborted or crashed may have left the GPU in a bad state


def run_child(case, *args, timeout=300, **env):
    assert not _stop, "no further GPU child is started after: %s" % _stop[0]
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e["ZKP_HIP_G16_WBITS"] = "8"
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


def golden(kind):
    with open(os.path.join(ROOT, "tests", "golden", PK_FILES[kind]), "rb") as f:
        return f.read()


def vk_len(kind):
    return 64 + 384 + 8 + 64 * N_IC[kind]


def g1_word(slot, win, ent, word):
    return ((slot * W8_NWIN + win) * W8_NENT + ent) * G1_WORDS + word


def vk_word(slot, win, ent, word):
    return ((slot * VK_NWIN + win) * VK_NENT + ent) * VK_WORDS + word


# ---------------------------------------------------------------------------------------------------- the tests (one child at a time)
pytestmark = pytest.mark.gpu


def test_clean_keys_are_sound_and_every_table_entry_is_counted():
    r = run_child("clean")
    assert r["failures"] == [], r
    for kind in (0, 1):
        rep, info = r["pk"][str(kind)], r["info_pk"][str(kind)]
        assert rep["format"] == "proving_key" and rep["verdict"] == "sound" and rep["stages_run"] == ["points", "twins", "tables"], rep
        assert (rep["g2_checked"], rep["g2_outside"], rep["g2_first_outside"]) == (G2_FINITE[kind], 0, None), rep
        assert (rep["twins_checked"], rep["twin_inf_mismatches"]) == (G2_FINITE[kind] - 3, 0) and rep["twins_query_ok"] is True and rep["twins_beta_delta_ok"] is True, rep
        # zkp_hip_groth16_key_info: radix 2^8, and the bytes of the two MSM tables: 64 per G1 entry, 128 per G2 entry
        assert info[:3] == [0, 8, 0] and 64 * rep["table_entries"]["g1"] + 128 * rep["table_entries"]["g2"] == info[3], (rep, info)
        assert rep["table_entries"]["g1"] % (W8_NWIN * W8_NENT) == 0 and rep["table_entries"]["g2"] == (G2_FINITE[kind] - 1) * W8_NWIN * W8_NENT, rep      # b_g2_query, delta, beta
        assert rep["table_entries"]["vk"] == (N_IC[kind] + 1) * VK_NWIN * VK_NENT and rep["table_bad_pairs"] == 0 and rep["table_first_bad"] is None, rep
        # a verifier-only key: no twins, and its tables are the gamma_abc_g1 / alpha tables alone
        rep, info = r["vk"][str(kind)], r["info_vk"][str(kind)]
        assert rep["format"] == "verifying_key" and rep["verdict"] == "sound" and rep["stages_run"] == ["points", "tables"], rep
        assert (rep["g2_checked"], rep["g2_outside"]) == (3, 0) and rep["twins_query_ok"] is None and rep["twins_beta_delta_ok"] is None and rep["twins_checked"] == 0, rep
        assert rep["table_entries"] == {"g1": 0, "g2": 0, "vk": (N_IC[kind] + 1) * VK_NWIN * VK_NENT} and VK_WORDS * 4 * rep["table_entries"]["vk"] == info[3], (rep, info)
    # a blob that is not the loaded key: points and twins, no tables by default; tables demanded for it is an argument error
    assert r["other"]["stages_run"] == ["points", "twins"] and r["other"]["verdict"] == "sound", r["other"]
    assert "not the key loaded" in r["other_tables_error"], r
    # counters: four loads built and checked tables (two proving keys, two verifying keys); every entry once at load and once in check_key
    once = sum(sum(r[k][str(kind)]["table_entries"].values()) for k in ("pk", "vk") for kind in (0, 1))
    c = r["counters"]
    assert (c["loads_checked"], c["entries_checked"], c["refused"]) == (4, 2 * once, 0) and c["ms"] > 0, (c, once)
    assert r["counters_after_reset"] == {"loads_checked": 0, "entries_checked": 0, "refused": 0, "ms": 0.0}, r
    print("check_key at radix 2^8, ms per stage: %r" % {k: r["pk"][k]["ms"] for k in ("0", "1")})


@pytest.fixture(scope="module")
def forged(tmp_path_factory):
    from oracle.py import bn254 as bn
    from test_emul_g16_keycheck import b_g1_offset, b_g2_offset, finite_b_g2, moved_g2
    d = tmp_path_factory.mktemp("keycheck")
    blob = golden(0)
    j = finite_b_g2(blob, 17)
    out = {"j": j}
    for name, data in (("b2_outside", moved_g2(blob, b_g2_offset(blob, j))), ("vk_gamma_outside", moved_g2(blob, 64 + 128)[:vk_len(0)])):
        out[name] = str(d / (name + ".bin"))
        open(out[name], "wb").write(data)
    # b_g1_query[j] doubled: a valid point, a broken twin.  j = the first index at which both are finite
    j2 = finite_b_g2(blob)
    off = b_g1_offset(blob, j2)
    ok, pt = bn.de_g1(blob[off:off + 64])
    assert ok and pt is not None
    twin = bytearray(blob)
    twin[off:off + 64] = bn.ser_g1(bn.G1C.double(pt))
    out["twin_doubled"], out["j2"] = str(d / "twin_doubled.bin"), j2
    open(out["twin_doubled"], "wb").write(bytes(twin))
    return out


def test_points_outside_the_subgroup_are_refused_at_load_and_named(forged):
    r = run_child("outside", forged["b2_outside"], forged["vk_gamma_outside"])
    assert r["failures"] == [], r
    name = "b_g2_query[%d]" % forged["j"]
    assert name in r["install_pk_error"] and "subgroup" in r["install_pk_error"], r
    assert r["verify_after"][0] == E_ARGUMENT and "no (usable) key loaded" in r["verify_after"][1], r          # no key was left behind
    assert r["info_after"][0] == E_ARGUMENT, r
    rep = r["report_pk"]
    assert (rep["verdict"], rep["g2_first_outside"], rep["g2_outside"], rep["g2_checked"]) == ("subgroup", 3 + forged["j"], 1, 224) and name in rep["message"], rep
    assert rep["stages_run"] == [] and rep["twins_query_ok"] is None, rep
    assert "gamma_g2" in r["install_vk_error"] and "subgroup" in r["install_vk_error"], r
    rep = r["report_vk"]
    assert (rep["format"], rep["verdict"], rep["g2_first_outside"], rep["g2_checked"]) == ("verifying_key", "subgroup", 1, 3), rep
    # two loads and two reports refused; no table was built
    assert r["counters"]["refused"] == 4 and r["counters"]["loads_checked"] == 0 and r["counters"]["entries_checked"] == 0, r
    assert r["memory_left_behind"] < (16 << 20), r          # a refused load frees what it took (a key's tables are 33 MB here)


def test_a_broken_twin_loads_is_reported_and_predicts_refused_proofs(forged):
    r = run_child("twins", forged["twin_doubled"])
    assert r["failures"] == [], r
    rep = r["report"]
    assert rep["verdict"] == "twins" and rep["stages_run"] == ["points"] and rep["g2_outside"] == 0, rep
    assert rep["twins_query_ok"] is False and rep["twins_beta_delta_ok"] is True and rep["twin_inf_mismatches"] == 0 and rep["twins_checked"] == 221, rep
    assert r["proof_verifies"] == [False], r          # today's behaviour, which the check predicts: it loads, it proves, nothing verifies
    assert r["golden_proof_verifies"] == [True], r
    # an infinity flag on one twin only fails the stage before any arithmetic
    rep = r["report_inf"]
    assert rep["verdict"] == "twins" and rep["twin_inf_mismatches"] == 1 and rep["twins_query_ok"] is False and rep["twins_beta_delta_ok"] is None, rep


def test_a_flipped_table_word_fails_the_load_and_is_found_again_by_check_key():
    g1w, vkw = g1_word(5, 7, 50, 3), vk_word(1, 3, 0, 11)
    r = run_child("flip", g1w, vkw)
    assert r["failures"] == [], r
    # entry 50 of (slot 5, window 7) and its right neighbour: one inconsistent window
    rc, msg = r["load_flip_g1"]
    assert rc == E_RUNTIME and msg == "Groth16 key tables failed their self-check (G1 slot 5 window 7, 1 inconsistent windows)", r
    assert r["info_after_flip_g1"][0] == E_ARGUMENT, r          # no key is left
    # entry 0 of window 3 of gamma_abc_g1[1]: the join from window 2 and all of window 3
    rc, msg = r["load_flip_vk"]
    assert rc == E_RUNTIME and msg == "Groth16 key tables failed their self-check (VK slot 1 window 3, 1 inconsistent windows)", r
    rc, msg = r["load_flip_vk_alone"]
    assert rc == E_RUNTIME and "VK slot 1 window 3" in msg, r
    assert r["info_after_flip_vk"][0] == E_ARGUMENT, r
    for name in ("malformed", "no_index", "unknown_table", "beyond"):
        assert r["load_" + name][0] == E_ARGUMENT and "ZKP_HIP_G16_TABLE_FLIP" in r["load_" + name][1], (name, r)
    # with the self-check off the same flips load, and check_key finds them where they are
    assert r["load_unchecked_g1"][0] == 0 and r["load_unchecked_vk"][0] == 0, r
    rep = r["report_unchecked_g1"]
    assert rep["verdict"] == "tables" and rep["table_first_bad"] == {"table": "g1", "slot": 5, "window": 7, "entry": 50} and rep["table_bad_pairs"] == 1, rep
    assert rep["stages_run"] == ["points", "twins"], rep
    rep = r["report_unchecked_vk"]
    assert rep["verdict"] == "tables" and rep["table_first_bad"] == {"table": "vk", "slot": 1, "window": 3, "entry": 0} and rep["table_bad_pairs"] == 1, rep
    # a clean load afterwards is sound: the flip touches only tables that are built under it
    assert r["report_clean_after"]["verdict"] == "sound", r
    c = r["counters"]
    assert c["refused"] == 5 and c["loads_checked"] == 4, c          # three refused loads and two unsound reports; checked loads: the three and the clean one


# ---------------------------------------------------------------------------------------------------- the children
def _child(case, args):
    sys.path.insert(0, ROOT)
    import libzkp_amd as z
    import libzkp_amd.api as api
    from libzkp_amd import _native
    L = _native.lib()
    out = {"failures": []}

    def info(kind):
        wbits, uneven, nbytes = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
        rc = L.zkp_hip_groth16_key_info(kind, ctypes.byref(wbits), ctypes.byref(uneven), ctypes.byref(nbytes))
        return [rc, wbits.value, uneven.value, nbytes.value]

    def load(kind, blob):
        rc = L.zkp_hip_groth16_load_key(kind, blob, len(blob))
        return [rc, _native.last_error() if rc else ""]

    def raises(f, *a):
        try:
            f(*a)
        except z.ZkpBackendError as e:
            return str(e)
        out["failures"].append("%s did not raise" % f.__name__)
        return ""

    def free_bytes():
        free, total = ctypes.c_size_t(), ctypes.c_size_t()
        f = L.hipMemGetInfo
        f.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
        f.restype = ctypes.c_int
        assert f(ctypes.byref(free), ctypes.byref(total)) == 0
        return free.value

    if case == "clean":
        z.key_check_counters()
        out.update(pk={}, vk={}, info_pk={}, info_vk={})
        for kind in (0, 1):
            api.install_proving_key(kind, golden(kind))
            out["info_pk"][kind] = info(kind)
            out["pk"][kind] = z.check_key(kind)
        for kind in (0, 1):
            api.install_verifying_key(kind, golden(kind)[:vk_len(kind)])
            out["info_vk"][kind] = info(kind)
            out["vk"][kind] = z.check_key(kind)
        # the proving key while the verifying key alone is loaded: not the loaded key, so no tables unless they are demanded
        out["other"] = z.check_key(0, golden(0))
        out["other_tables_error"] = raises(z.check_key, 0, golden(0), True, True)
        out["counters"] = z.key_check_counters()
        out["counters_after_reset"] = z.key_check_counters()
    elif case == "outside":
        pk, vk = open(args[0], "rb").read(), open(args[1], "rb").read()
        L.zkp_hip_init(0)
        z.key_check_counters()
        before = free_bytes()
        out["install_pk_error"] = raises(api.install_proving_key, 0, pk)
        out["memory_left_behind"] = before - free_bytes()
        buf, lens, ok = np.zeros((1, 298), dtype=np.uint8), np.full(1, 298, dtype=np.uint32), np.zeros(1, dtype=np.uint8)
        P = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
        rc = L.zkp_hip_verify_equality_batch(1, P(buf), 298, P(lens), P(ok))
        out["verify_after"] = [rc, _native.last_error()]
        out["info_after"] = info(0)
        out["report_pk"] = z.check_key(0, pk)
        out["install_vk_error"] = raises(api.install_verifying_key, 0, vk)
        out["report_vk"] = z.check_key(0, vk)
        out["counters"] = z.key_check_counters()
    elif case == "twins":
        twin = open(args[0], "rb").read()
        api.install_proving_key(0, golden(0))
        good = z.prove_equality_batch([77], [77], seeds=bytes(range(32)))
        api.install_proving_key(0, twin)          # it loads
        out["report"] = z.check_key(0)
        proofs = z.prove_equality_batch([77], [77], seeds=bytes(range(32)))
        out["proof_verifies"] = api._verify_snark_envelopes(0, proofs)          # zkp_hip_verify_equality_batch under the key's own verifying key
        out["golden_proof_verifies"] = api._verify_snark_envelopes(0, good)     # (the verifying key is the golden one: the forged point is not part of it)
        from test_emul_g16_keycheck import b_g1_offset, finite_b_g2
        inf = bytearray(golden(0))
        off = b_g1_offset(inf, finite_b_g2(inf))
        inf[off:off + 64] = bytes(63) + b"\x40"
        out["report_inf"] = z.check_key(0, bytes(inf))
    elif case == "flip":
        g1w, vkw = int(args[0]), int(args[1])
        pk, vk = golden(0), golden(0)[:vk_len(0)]
        L.zkp_hip_init(0)
        z.key_check_counters()
        os.environ["ZKP_HIP_G16_TABLE_FLIP"] = "g1:%d" % g1w
        out["load_flip_g1"] = load(0, pk)
        out["info_after_flip_g1"] = info(0)
        os.environ["ZKP_HIP_G16_TABLE_FLIP"] = "vk:%d" % vkw
        out["load_flip_vk"] = load(0, pk)
        out["load_flip_vk_alone"] = load(0, vk)
        out["info_after_flip_vk"] = info(0)
        for name, value in (("malformed", "g1"), ("no_index", "g2:"), ("unknown_table", "g3:5"), ("beyond", "g1:%d" % (1 << 40))):
            os.environ["ZKP_HIP_G16_TABLE_FLIP"] = value
            out["load_" + name] = load(0, pk)
        os.environ["ZKP_HIP_G16_TABLE_CHECK"] = "0"
        os.environ["ZKP_HIP_G16_TABLE_FLIP"] = "g1:%d" % g1w
        out["load_unchecked_g1"] = load(0, pk)
        api._key_blobs[0] = pk
        api._keys_loaded[0] = "<test>"
        out["report_unchecked_g1"] = z.check_key(0, pk, tables=True)
        os.environ["ZKP_HIP_G16_TABLE_FLIP"] = "vk:%d" % vkw
        out["load_unchecked_vk"] = load(0, pk)
        out["report_unchecked_vk"] = z.check_key(0, pk, tables=True)
        del os.environ["ZKP_HIP_G16_TABLE_FLIP"], os.environ["ZKP_HIP_G16_TABLE_CHECK"]
        api.install_proving_key(0, pk)
        out["report_clean_after"] = z.check_key(0)
        out["counters"] = z.key_check_counters()
    else:
        raise SystemExit("unknown case %r" % case)
    print(json.dumps(out))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2:])
