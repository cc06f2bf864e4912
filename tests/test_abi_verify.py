"""The C ABI of the mixed verifier: include/libzkp_hip_verify.h compiles as C, the built library exports its symbols, and the Python
binding, the Rust binding and the C++ caller name exactly those.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_verify.h")


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkp_hip_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "libzkp_hip_verify.h"\nint main(void){return ZKP_HIP_COUNTER_VERIFY_MIXED == 6 ? ZKP_HIP_OK : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])


def test_library_exports_both_symbols():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    syms = declared_symbols()
    assert syms == ["zkp_hip_verify_envelopes", "zkp_hip_verify_envelopes_device"] == sorted(_native.EXPORTS_VERIFY)
    assert not set(syms) & set(_native.EXPORTS) and _native.COUNTER_VERIFY_MIXED == 6
    lib = ctypes.CDLL(_native.LIB_PATH)
    for s in syms:
        assert getattr(lib, s) is not None
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert set(syms) <= set(re.findall(r" T (zkp_hip_\w+)", nm))


def test_rust_binding_declares_exactly_the_headers_symbols():
    rs = open(os.path.join(ROOT, "rust", "hip_ffi_verify.rs")).read()
    assert sorted(set(re.findall(r"pub fn (zkp_hip_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()
    assert "pub const ZKP_HIP_COUNTER_VERIFY_MIXED: c_int = 6;" in rs
    backend = open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()
    assert "ffi_verify::zkp_hip_verify_envelopes(" in backend and "pub fn verify_proofs_parallel(" in backend and "pub fn verify_composite_inner_proofs(" in backend


def test_absurd_sizes_are_argument_errors_before_anything_is_read():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    for f in (L.zkp_hip_verify_envelopes, L.zkp_hip_verify_envelopes_device):
        f.argtypes = [ctypes.c_uint64] + [ctypes.c_void_p] * 4
        assert f((1 << 22) + 1, None, None, None, None) == -3 and b"batch too large" in L.zkp_hip_last_error()
        assert f(1 << 40, None, None, None, None) == -3
        assert f(0, None, None, None, None) == 0
        assert f(1, None, None, None, None) == -3 and b"null pointer" in L.zkp_hip_last_error()


# the six per-scheme host-buffer verify calls: name, number of pointer arguments (n first, stride after the first pointer)
PER_SCHEME_VERIFY = [("range", 5), ("threshold", 4), ("consistency", 3), ("equality", 3), ("membership", 3), ("improvement", 4)]


@pytest.mark.parametrize("name,nptr", PER_SCHEME_VERIFY)
def test_per_scheme_verify_refusals_and_their_order(name, nptr):
    """Every refusal below is made before a device is looked for.  The order is part of the contract: a null pointer is reported before
    the batch size (the mixed call above tests the size first), the stride last."""
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    f = getattr(L, "zkp_hip_verify_%s_batch" % name)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * (nptr - 1)
    bufs = [ctypes.create_string_buffer(64) for _ in range(nptr)]
    valid = [ctypes.addressof(b) for b in bufs]

    def call(n, ptrs, stride=64):
        return f(n, ptrs[0], stride, *ptrs[1:])

    assert call(0, [None] * nptr) == 0
    for k in range(nptr):
        assert call(1, valid[:k] + [None] + valid[k + 1:]) == -3 and b"null pointer" in L.zkp_hip_last_error(), k
    assert call((1 << 22) + 1, [None] * nptr) == -3 and b"null pointer" in L.zkp_hip_last_error()
    assert call((1 << 22) + 1, valid) == -3 and b"batch too large" in L.zkp_hip_last_error()
    assert call((1 << 22) + 1, valid, 0) == -3 and b"batch too large" in L.zkp_hip_last_error()
    assert call(1, valid, 0) == -3 and b"bad stride" in L.zkp_hip_last_error()


def test_cpp_caller_builds_and_fails_loudly_without_gpu():
    """tests/abi/abi_call_verify.cpp calls both entry points through the headers alone.  Here: it compiles and links against the built
    library, names every declared symbol, and -- on a box without a GPU -- reports the missing device instead of computing anything on
    the CPU.  The GPU tier runs it for real (tests/test_gpu_abi_verify.py)."""
    import __graft_entry__ as ge
    exe = ge.build_abi_verify_caller()
    src = open(os.path.join(ROOT, "tests", "abi", "abi_call_verify.cpp")).read()
    assert sorted(set(re.findall(r"CALLED\((zkp_hip_[a-z_0-9]+)\)", src))) == declared_symbols()
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present: the real run is in the gpu tier")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden")], capture_output=True, text=True)
    assert r.returncode != 0 and "no HIP device available" in r.stderr
