"""The C ABI of the sealing calls: include/libzkp_hip_seal.h compiles as C, the built library exports its three symbols, none of them is a
zkp_* name, the Python and Rust bindings name exactly them, and the status constants agree across the three.  No compute calls (no GPU
needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_seal.h")
SYMBOLS = ["libzkp_seal_batch", "libzkp_seal_composites", "libzkp_seal_counters"]
STATUSES = {"FAILED_OP": 0, "SEALED": 1, "REFUSED": 2, "UNREADABLE": 3}


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(libzkp_seal_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "libzkp_hip_seal.h"\n'
                 'int main(void){double ms; uint64_t a, b, c, d; uint8_t st[1], out[1]; uint64_t off[2] = {0, 0}; const uint64_t first[2] = {0, 0}; zkp_hip_batch* batch = 0;\n'
                 'return libzkp_seal_composites(0, 0, off, 0, first, 0, 0, out, 1, off, st) == ZKP_HIP_OK && libzkp_seal_batch(batch, 0, first, 0, 0, out, 1, off, st) == ZKP_HIP_OK\n'
                 '       && libzkp_seal_counters(&ms, &a, &b, &c, &d, 0) == ZKP_HIP_OK\n'
                 '       && LIBZKP_SEAL_FAILED_OP + LIBZKP_SEAL_SEALED + LIBZKP_SEAL_REFUSED + LIBZKP_SEAL_UNREADABLE == 6u ? 0 : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])


def test_library_exports_the_symbols_and_no_other_list_names_them():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    assert declared_symbols() == SYMBOLS == sorted(_native.EXPORTS_SEAL)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = set(re.findall(r" T (libzkp_\w+)", nm))
    assert exported == set(SYMBOLS)                                       # exactly the header's three under this prefix
    L = ctypes.CDLL(_native.LIB_PATH)
    others = set(_native.EXPORTS) | set(_native.EXPORTS_VERIFY) | set(_native.EXPORTS_BP_LOCALISE) | set(_native.EXPORTS_COMPOSITES) | set(_native.EXPORTS_STATEMENTS)
    for s in SYMBOLS:
        assert not s.startswith("zkp_") and s not in others
        assert getattr(L, s) is not None
    # the zkp_* names of the library stay the closed set they were
    assert set(re.findall(r" T (zkp_\w+)", nm)) == others
    import libzkp_amd
    for name in ("create_composite_proofs", "process_ops_sealed", "seal_counters"):
        assert name in libzkp_amd.__all__ and callable(getattr(libzkp_amd, name))


def test_status_constants_agree_across_header_python_and_rust():
    from libzkp_amd import _native
    hdr, rs = open(HEADER).read(), open(os.path.join(ROOT, "rust", "hip_ffi_seal.rs")).read()
    assert sorted(set(re.findall(r"pub fn (libzkp_seal_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()
    assert not re.findall(r"pub fn (zkp_\w+)", rs)
    for name, value in STATUSES.items():
        assert re.search(r"#define LIBZKP_SEAL_%s (\d+)u" % name, hdr).group(1) == str(value)
        assert getattr(_native, "SEAL_" + name) == value
        assert "pub const LIBZKP_SEAL_%s: u8 = %d;" % (name, value) in rs
    assert "not upstream's" in hdr and "one 4 MiB container is the worst case" in hdr and "not spread over the registered" in hdr


def test_n_0_touches_nothing_and_argument_errors_come_before_any_device():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    f = L.libzkp_seal_counters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_uint64)] * 4 + [ctypes.c_int]
    assert f(None, None, None, None, None, 0) == 0 and f(None, None, None, None, None, 1) == 0
    ms, a, b = ctypes.c_double(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert f(ctypes.byref(ms), ctypes.byref(a), None, None, ctypes.byref(b), 0) == 0 and (ms.value, a.value, b.value) == (0.0, 0, 0)
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    s = L.libzkp_seal_composites
    s.restype = ctypes.c_int
    s.argtypes = [u64, vp, vp, u64, vp, vp, vp, vp, u64, vp, vp]
    assert s(0, None, None, 0, None, None, None, None, 0, None, None) == 0          # no pointer is read, no device is opened
    assert s((1 << 22) + 1, None, None, 0, None, None, None, None, 0, None, None) == -3 and b"split" in L.zkp_hip_last_error()
    assert s(1, None, None, (1 << 22) + 1, None, None, None, None, 0, None, None) == -3 and b"split" in L.zkp_hip_last_error()
    assert s(1, None, None, 0, None, None, None, None, 0, None, None) == -3 and b"null pointer" in L.zkp_hip_last_error()
    first = (u64 * 3)(0, 2, 1)
    off, st = (u64 * 3)(), (ctypes.c_uint8 * 2)()
    assert s(2, None, None, 2, first, None, None, None, 0, off, st) == -3 and b"first[]" in L.zkp_hip_last_error()          # runs backwards
    first = (u64 * 3)(0, 1, 3)
    assert s(2, None, None, 2, first, None, None, None, 0, off, st) == -3 and b"first[]" in L.zkp_hip_last_error()          # leaves the list
    t = L.libzkp_seal_batch
    t.restype = ctypes.c_int
    t.argtypes = [vp, u64, vp, vp, vp, vp, u64, vp, vp]
    assert t(None, 0, None, None, None, None, 0, None, None) == 0
    assert t(None, 1, None, None, None, None, 0, None, None) == -3 and b"null batch" in L.zkp_hip_last_error()
    assert f(None, ctypes.byref(a), None, None, None, 0) == 0 and a.value == 0
