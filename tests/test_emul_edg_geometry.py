"""The Bulletproofs generator tables at every radix 2^10 .. 2^16 (libzkp_amd/csrc/edg.h: EdgGeom), on the CPU: window counts, the
signed recoding the prover and verifier store, the table builder and its self-check, and one MSM launch walked through its step list."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from util import P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 2**252 + 27742317777372353535851937790883648493
WBITS = range(10, 17)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emul_edg") / "libemul_edg_geometry.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, os.path.join(ROOT, "tests", "emul", "emul_edg_geometry.cpp")])
    return ctypes.CDLL(so)


def geom(lib, w):
    out = np.zeros(5, dtype=np.uint32)
    lib.emul_edg_geom(w, P(out))
    return dict(zip(("wbits", "nwin", "nwin_u64", "nent", "nseg"), (int(x) for x in out)))


def digits(lib, w, k):
    raw = np.frombuffer(int(k).to_bytes(32, "little"), dtype=np.uint32).copy()
    out = np.zeros(13, dtype=np.uint32)
    lib.emul_edg_digits(w, P(raw), P(out))
    return [int(d) for d in out.view(np.int16)]


@pytest.mark.parametrize("w", WBITS)
def test_geometry_is_the_smallest_that_covers(lib, w):
    g = geom(lib, w)
    assert g["wbits"] == w and g["nent"] == 2 ** (w - 1) and g["nseg"] * 64 == g["nent"]
    assert g["nwin"] * w >= 254 and (g["nwin"] - 1) * w < 254          # a scalar below l < 2^253 plus the carry of the recoding
    assert g["nwin_u64"] * w >= 65 and (g["nwin_u64"] - 1) * w < 65
    assert g["nwin"] <= 26                                            # the 13-word digit rows hold them
    assert 130 * g["nwin"] * g["nent"] * 128 == {16: 8724152320, 15: 4634705920, 14: 2589982720, 13: 1363148800,
                                                 12: 749731840, 11: 408944640, 10: 221511680}[w]


@pytest.mark.parametrize("w", WBITS)
def test_recoding_reassembles(lib, w):
    g = geom(lib, w)
    rng = np.random.default_rng(100 + w)
    scalars = [0, 1, L - 1, 2**253 - 1] + [int.from_bytes(rng.bytes(32), "little") % L for _ in range(200)]
    values = [0, 1, 2**64 - 1] + [int.from_bytes(rng.bytes(8), "little") for _ in range(50)]
    half = 2 ** (w - 1)
    for k, nd in [(k, g["nwin"]) for k in scalars] + [(v, g["nwin_u64"]) for v in values]:
        d = digits(lib, w, k)
        assert sum(x << (w * i) for i, x in enumerate(d[:nd])) == k, (w, k)
        assert not any(d[nd:]), (w, k)                                 # nothing beyond the windows the layouts walk
        if w < 16:
            assert all(-(half - 1) <= x <= half for x in d), (w, k)
        else:                                                          # sc_recode_signed65536, unchanged: [-32768, 32767]
            assert all(-half <= x < half for x in d), (w, k)


@pytest.mark.parametrize("w", WBITS)
def test_builder_and_self_check(lib, w):
    g = geom(lib, w)
    for gen, win in ((0, 0), (67, g["nwin"] // 2), (129, g["nwin"] - 1)):
        assert lib.emul_edg_window_geom(w, gen, win, 10, 3 + win) == 0, (w, gen, win)


@pytest.mark.parametrize("w", WBITS)
def test_msm_chunks_through_step_lists(lib, w):
    assert lib.emul_edg_msm_phase1(w, 8, 2, 40 + w) == 0
