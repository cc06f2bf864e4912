"""The C ABI of the composite-proof list call: include/libzkp_hip_composites.h compiles as C, the built library exports its two symbols, and
the Python and Rust bindings name exactly them.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_composites.h")
SYMBOLS = ["zkp_hip_composites_counters", "zkp_hip_verify_composites"]


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkp_hip_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "libzkp_hip_composites.h"\n'
                 'int main(void){double ms; uint64_t a, b, c; uint8_t st[1]; const uint64_t off[2] = {0, 0}; uint32_t f = ZKP_HIP_COMPOSITES_INTEGRITY_ONLY;\n'
                 'return zkp_hip_verify_composites(0, 0, off, f, st) == ZKP_HIP_OK && zkp_hip_composites_counters(&ms, &a, &b, &c, 0) == ZKP_HIP_OK ? 0 : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])


def test_library_exports_the_symbols_and_no_other_list_names_them():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    assert declared_symbols() == SYMBOLS == sorted(_native.EXPORTS_COMPOSITES)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = set(re.findall(r" T (zkp_hip_\w+)", nm))
    L = ctypes.CDLL(_native.LIB_PATH)
    for s in SYMBOLS:
        assert s not in _native.EXPORTS and s not in _native.EXPORTS_VERIFY and s not in _native.EXPORTS_BP_LOCALISE
        assert getattr(L, s) is not None and s in exported
    # every exported symbol belongs to exactly one header's list
    assert exported == set(_native.EXPORTS) | set(_native.EXPORTS_VERIFY) | set(_native.EXPORTS_BP_LOCALISE) | set(_native.EXPORTS_COMPOSITES)
    import libzkp_amd
    assert "verify_composite_proofs" in libzkp_amd.__all__ and "verify_composites_counters" in libzkp_amd.__all__
    assert re.search(r"#define ZKP_HIP_COMPOSITES_INTEGRITY_ONLY (\d+)u", open(HEADER).read()).group(1) == str(_native.COMPOSITES_INTEGRITY_ONLY) == "1"


def test_rust_binding_declares_exactly_the_headers_symbols():
    rs = open(os.path.join(ROOT, "rust", "hip_ffi_composites.rs")).read()
    assert sorted(set(re.findall(r"pub fn (zkp_hip_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()
    assert "pub const ZKP_HIP_COMPOSITES_INTEGRITY_ONLY: u32 = 1;" in rs


def test_the_counters_call_works_with_null_pointers_before_any_init_and_n_0_returns_0():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    f = L.zkp_hip_composites_counters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_uint64)] * 3 + [ctypes.c_int]
    assert f(None, None, None, None, 0) == 0 and f(None, None, None, None, 1) == 0
    ms, a, b, c = ctypes.c_double(7), ctypes.c_uint64(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert f(ctypes.byref(ms), ctypes.byref(a), None, ctypes.byref(c), 0) == 0
    assert (ms.value, a.value, b.value, c.value) == (0.0, 0, 7, 0)
    v = L.zkp_hip_verify_composites
    v.restype = ctypes.c_int
    v.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    assert v(0, None, None, 0, None) == 0 and v(0, None, None, 1, None) == 0          # touches nothing: no pointer is read, no device is opened
    assert f(None, ctypes.byref(a), None, None, 0) == 0 and a.value == 0
    # refused before any device work: more containers than a call takes
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    assert v((1 << 22) + 1, None, None, 0, None) == -3 and b"split" in L.zkp_hip_last_error()
