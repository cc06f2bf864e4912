"""The C ABI of the statement verifier: include/libzkp_hip_statements.h compiles as C, the built library exports its three symbols, none of
them is a zkp_hip_* name, and the Python and Rust bindings name exactly them.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_statements.h")
SYMBOLS = ["zkp_stmt_counters", "zkp_stmt_verify", "zkp_stmt_verify_device"]


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkp_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c(tmp_path):
    c = tmp_path / "t.c"
    c.write_text('#include "libzkp_hip_statements.h"\n'
                 'int main(void){double ms; uint64_t a, b, c, d; uint8_t ok[1], why[1]; const uint64_t off[2] = {0, 0}; zkp_hip_op op; op.kind = ZKP_HIP_OP_RANGE;\n'
                 'return zkp_stmt_verify(0, &op, 0, 0, 0, off, ok, why) == ZKP_HIP_OK && zkp_stmt_verify_device(0, &op, 0, 0, 0, off, ok, 0) == ZKP_HIP_OK\n'
                 '       && zkp_stmt_counters(&ms, &a, &b, &c, &d, 0) == ZKP_HIP_OK && ZKP_STMT_ACCEPTED + ZKP_STMT_ENVELOPE + ZKP_STMT_STATEMENT + ZKP_STMT_PROOF == 6 ? 0 : 1;}\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(c), "-o", str(tmp_path / "t.o")])


def test_library_exports_the_symbols_and_no_other_list_names_them():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    assert declared_symbols() == SYMBOLS == sorted(_native.EXPORTS_STATEMENTS)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    exported = set(re.findall(r" T (zkp_\w+)", nm))
    L = ctypes.CDLL(_native.LIB_PATH)
    others = set(_native.EXPORTS) | set(_native.EXPORTS_VERIFY) | set(_native.EXPORTS_BP_LOCALISE) | set(_native.EXPORTS_COMPOSITES)
    for s in SYMBOLS:
        assert not s.startswith("zkp_hip_") and s not in others
        assert getattr(L, s) is not None and s in exported
    # every exported symbol belongs to exactly one header's list
    assert exported == others | set(_native.EXPORTS_STATEMENTS)
    import libzkp_amd
    assert "verify_ops" in libzkp_amd.__all__ and "verify_statements_counters" in libzkp_amd.__all__
    enum = re.search(r"enum \{ ZKP_STMT_ACCEPTED = (\d),.*?ZKP_STMT_ENVELOPE = (\d),.*?ZKP_STMT_STATEMENT = (\d),.*?ZKP_STMT_PROOF = (\d) \}", open(HEADER).read(), flags=re.S)
    assert tuple(int(x) for x in enum.groups()) == (_native.STMT_ACCEPTED, _native.STMT_ENVELOPE, _native.STMT_STATEMENT, _native.STMT_PROOF) == (0, 1, 2, 3)


def test_rust_binding_declares_exactly_the_headers_symbols():
    rs = open(os.path.join(ROOT, "rust", "hip_ffi_statements.rs")).read()
    assert sorted(set(re.findall(r"pub fn (zkp_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()
    for name, value in (("ACCEPTED", 0), ("ENVELOPE", 1), ("STATEMENT", 2), ("PROOF", 3)):
        assert "pub const ZKP_STMT_%s: u8 = %d;" % (name, value) in rs
    backend = open(os.path.join(ROOT, "rust", "hip_backend.rs")).read()
    assert "ffi_statements::zkp_stmt_verify(" in backend and "pub fn verify_batch_operations(ops: &[BatchOperation], proofs: &[Vec<u8>]) -> Vec<bool>" in backend


def test_n_0_touches_nothing_and_an_absurd_size_is_an_argument_error_without_a_device():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    f = L.zkp_stmt_counters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_uint64)] * 4 + [ctypes.c_int]
    assert f(None, None, None, None, None, 0) == 0 and f(None, None, None, None, None, 1) == 0
    ms, a, b = ctypes.c_double(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert f(ctypes.byref(ms), ctypes.byref(a), None, None, ctypes.byref(b), 0) == 0 and (ms.value, a.value, b.value) == (0.0, 0, 0)
    for v in (L.zkp_stmt_verify, L.zkp_stmt_verify_device):
        v.restype = ctypes.c_int
        v.argtypes = [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4
        assert v(0, None, None, 0, None, None, None, None) == 0          # no pointer is read, no device is opened
        assert v((1 << 22) + 1, None, None, 0, None, None, None, None) == -3 and b"batch too large" in L.zkp_hip_last_error()
        assert v(1 << 40, None, None, 0, None, None, None, None) == -3
    assert f(None, ctypes.byref(a), None, None, None, 0) == 0 and a.value == 0
