"""The C ABI of the Bulletproofs localisation counters: include/libzkp_hip_bp_localise.h compiles as C, the built library exports its one
symbol, and the Python and Rust bindings name exactly it.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_bp_localise.h")
SYMBOL = "zkp_hip_bp_localise_counters"


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkp_hip_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "libzkp_hip_bp_localise.h"\nint main(void){double ms; uint64_t a, b, c; return zkp_hip_bp_localise_counters(&ms, &a, &b, &c, 0) == ZKP_HIP_OK ? 0 : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])


def test_library_exports_the_symbol_and_no_other_list_names_it():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    assert declared_symbols() == [SYMBOL] == list(_native.EXPORTS_BP_LOCALISE)
    assert SYMBOL not in _native.EXPORTS and SYMBOL not in _native.EXPORTS_VERIFY
    assert getattr(ctypes.CDLL(_native.LIB_PATH), SYMBOL) is not None
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert SYMBOL in set(re.findall(r" T (zkp_hip_\w+)", nm))
    import libzkp_amd
    assert "bp_verify_counters" in libzkp_amd.__all__


def test_rust_binding_declares_exactly_the_headers_symbol():
    rs = open(os.path.join(ROOT, "rust", "hip_ffi_bp_localise.rs")).read()
    assert sorted(set(re.findall(r"pub fn (zkp_hip_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()


def test_the_call_works_with_null_pointers_before_any_init():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    f = getattr(L, SYMBOL)
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_uint64)] * 3 + [ctypes.c_int]
    assert f(None, None, None, None, 0) == 0 and f(None, None, None, None, 1) == 0
    ms, a, b, c = ctypes.c_double(7), ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert f(ctypes.byref(ms), ctypes.byref(a), None, ctypes.byref(c), 0) == 0
    assert (ms.value, a.value, b.value, c.value) == (0.0, 0, 7, 0)
