"""The two key formats of zkp_hip_groth16_load_key (libzkp_amd/csrc/g16_keyblob.h), on the CPU: a blob that ends behind gamma_abc_g1 is
a verifying key, one with bytes left is a proving key; the shape rules of a verifying key; the parsed points against oracle/py/bn254.py's
reading of the same bytes.  Blobs are cut from the golden proving keys."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle.py import bn254 as bn
from util import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {0: "equality_mimc_pk.bin", 1: "membership_mimc_pk.bin"}
N_IC = {0: 2, 1: 2 + 2 * 64}          # the constant one, the commitment | and 64 set values + 64 is-real flags
MALFORMED, PROVING, VERIFYING, REFUSED = -1, 0, 1, 2


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_keyblob") / "libemul_g16_keyblob.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "emul_g16_keyblob.cpp")])
    L = ctypes.CDLL(so)
    L.emul_keyblob_vk_bytes.restype = ctypes.c_uint64
    L.emul_keyblob_vk_bytes.argtypes = [ctypes.c_uint64]
    return L


def pk_blob(kind):
    with open(os.path.join(ROOT, "tests", "golden", KINDS[kind]), "rb") as f:
        return f.read()


def vk_len(kind):
    return 64 + 384 + 8 + 64 * N_IC[kind]


def classify(lib, kind, blob):
    n_ic, rest, why = ctypes.c_uint32(), ctypes.c_uint64(), ctypes.create_string_buffer(200)
    r = lib.emul_keyblob_classify(kind, blob, ctypes.c_uint64(len(blob)), ctypes.byref(n_ic), ctypes.byref(rest), why, 200)
    return r, n_ic.value, rest.value, why.value.decode()


def test_sizes_come_from_the_circuits(lib):
    for kind in KINDS:
        assert lib.emul_keyblob_n_inst(kind) == N_IC[kind]
        assert lib.emul_keyblob_vk_bytes(N_IC[kind]) == vk_len(kind)
        assert int.from_bytes(pk_blob(kind)[448:456], "little") == N_IC[kind]


@pytest.mark.parametrize("kind", KINDS)
def test_whole_file_is_a_proving_key(lib, kind):
    blob = pk_blob(kind)
    r, n_ic, rest, _ = classify(lib, kind, blob)
    assert (r, n_ic, rest) == (PROVING, N_IC[kind], len(blob) - vk_len(kind))


@pytest.mark.parametrize("kind", KINDS)
def test_prefix_is_a_verifying_key(lib, kind):
    r, n_ic, rest, why = classify(lib, kind, pk_blob(kind)[:vk_len(kind)])
    assert (r, n_ic, rest, why) == (VERIFYING, N_IC[kind], 0, "")


@pytest.mark.parametrize("kind", KINDS)
def test_one_byte_fewer_and_one_byte_more(lib, kind):
    blob, n = pk_blob(kind), vk_len(kind)
    assert classify(lib, kind, blob[:n - 1])[0] == MALFORMED          # truncated inside the last gamma_abc_g1 point
    r, n_ic, rest, _ = classify(lib, kind, blob[:n + 1])              # bytes remain: offered to the proving-key reader, which refuses it
    assert (r, n_ic, rest) == (PROVING, N_IC[kind], 1)
    for cut in (0, 63, 64, 448, 455, 456):                            # and every earlier boundary of the prefix
        assert classify(lib, kind, blob[:cut])[0] == MALFORMED, cut


def test_wrong_circuit(lib):
    r, n_ic, _, why = classify(lib, 1, pk_blob(0)[:vk_len(0)])
    assert (r, n_ic) == (REFUSED, 2) and "verifying key" in why and "circuit" in why
    r, n_ic, _, why = classify(lib, 0, pk_blob(1)[:vk_len(1)])
    assert (r, n_ic) == (REFUSED, 130) and "verifying key" in why


@pytest.mark.parametrize("kind", KINDS)
def test_points_at_infinity_are_refused(lib, kind):
    good = pk_blob(kind)[:vk_len(kind)]
    ends = {"alpha": 64, "beta": 192, "gamma": 320, "delta": 448, "abc0": 520, "abc_last": vk_len(kind)}
    for name, end in ends.items():
        blob = bytearray(good)
        blob[end - 1] = (blob[end - 1] & 0x3F) | 0x40
        r, _, _, why = classify(lib, kind, bytes(blob))
        assert r == REFUSED and "verifying key" in why and "infinity" in why, (name, r, why)
        blob[end - 1] |= 0xC0                                          # both flag bits: no valid encoding at all
        assert classify(lib, kind, bytes(blob))[0] == MALFORMED, name


@pytest.mark.parametrize("kind", KINDS)
def test_a_point_off_the_curve_or_not_canonical(lib, kind):
    good = pk_blob(kind)[:vk_len(kind)]
    blob = bytearray(good)
    blob[456 + 3] ^= 1                                                 # x of gamma_abc_g1[0]
    assert classify(lib, kind, bytes(blob))[0] == MALFORMED
    blob = bytearray(good)
    blob[0:32] = (bn.P).to_bytes(32, "little")                         # alpha.x = p
    assert classify(lib, kind, bytes(blob))[0] == MALFORMED


@pytest.mark.parametrize("kind", KINDS)
def test_points_match_the_oracles_reading(lib, kind):
    blob = pk_blob(kind)[:vk_len(kind)]
    n = N_IC[kind]
    words = np.zeros(16 + 96 + 16 * n, dtype=np.uint32)
    inf = np.zeros(4 + n, dtype=np.uint8)
    for src in (blob, pk_blob(kind)):                                  # the same prefix read from either format
        assert lib.emul_keyblob_points(src, ctypes.c_uint64(len(src)), P(words), len(words), P(inf)) == 4 + n
        assert not inf.any()
        raw = words.tobytes()
        val = lambda off: int.from_bytes(raw[off:off + 32], "little")  # noqa: E731
        ok, alpha = bn.de_g1(blob[0:64])
        assert ok and (val(0), val(32)) == alpha
        for k in range(3):
            ok, pt = bn.de_g2(blob[64 + 128 * k:192 + 128 * k])
            o = 64 + 128 * k
            assert ok and ((val(o), val(o + 32)), (val(o + 64), val(o + 96))) == pt
        for i in range(n):
            ok, pt = bn.de_g1(blob[456 + 64 * i:520 + 64 * i])
            o = 448 + 64 * i
            assert ok and (val(o), val(o + 32)) == pt, i
    # a point at infinity is reported as such and the others are still read
    bad = bytearray(blob)
    bad[319] = (bad[319] & 0x3F) | 0x40
    assert lib.emul_keyblob_points(bytes(bad), ctypes.c_uint64(len(bad)), P(words), len(words), P(inf)) == 4 + n
    assert list(np.nonzero(inf)[0]) == [2] and bn.de_g2(bytes(bad[192:320])) == (True, None)
