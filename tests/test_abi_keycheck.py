"""The C ABI of the Groth16 key check: include/libzkp_hip_keycheck.h compiles as C, the built library exports its two symbols, neither is a
zkp_* or libzkp_* name (those sets stay closed), the Python and Rust bindings name exactly them, and the constants and the report's layout
agree across the three.  No compute calls (no GPU needed)."""
import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "libzkp_hip_keycheck.h")
SYMBOLS = ["zkpkeycheck_counters", "zkpkeycheck_key"]
STAGES = {"POINTS": 1, "TWINS": 2, "TABLES": 4}
VERDICTS = {"SOUND": 0, "FAILED_FORMAT": 1, "FAILED_SUBGROUP": 2, "FAILED_TWINS": 3, "FAILED_TABLES": 4}


def declared_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(zkpkeycheck_[a-z_0-9]+)\s*\(", src)))


def test_header_is_plain_c_and_the_report_has_the_bindings_layout(tmp_path):
    from libzkp_amd import _native
    c = tmp_path / "t.c"
    fields = [f for f, _ in _native.KeyCheckReport._fields_]
    c.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "libzkp_hip_keycheck.h"\n'
                 'int main(int argc, char** argv){ zkp_keycheck_report r; double ms; uint64_t a, b, c; const uint8_t key[1] = {0};\n'
                 ' if (argc > 5) return zkpkeycheck_key(0, key, 1, ZKP_KEYCHECK_POINTS | ZKP_KEYCHECK_TWINS | ZKP_KEYCHECK_TABLES, &r) == ZKP_HIP_OK\n'
                 '        && zkpkeycheck_counters(&ms, &a, &b, &c, 0) == ZKP_HIP_OK && r.verdict == ZKP_KEYCHECK_SOUND ? 0 : 1;\n'
                 ' (void)argv; printf("%u", (unsigned)sizeof r);\n' +
                 "".join(' printf(" %%u", (unsigned)offsetof(zkp_keycheck_report, %s));\n' % f for f in fields) +
                 ' return 0; }\n')
    inc = ["-I", os.path.join(ROOT, "include")]
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic"] + inc + ["-c", str(c), "-o", str(tmp_path / "t.o")])
    # a C caller links against the library with the header alone, and the struct it sees is the one ctypes lays out
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    exe = str(tmp_path / "t")
    libdir = os.path.dirname(_native.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99"] + inc + [str(c), "-o", exe, "-L" + libdir, "-lzkp_hip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    got = [int(x) for x in subprocess.check_output([exe], text=True).split()]
    assert got[0] == ctypes.sizeof(_native.KeyCheckReport)
    assert got[1:] == [getattr(_native.KeyCheckReport, f).offset for f in fields]


def test_library_exports_the_symbols_and_no_other_list_names_them():
    from libzkp_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        import __graft_entry__ as ge
        ge.build_hip()
    assert declared_symbols() == SYMBOLS == sorted(_native.EXPORTS_KEYCHECK)
    nm = subprocess.check_output(["nm", "-D", "--defined-only", _native.LIB_PATH], text=True)
    assert set(re.findall(r" T (zkpkeycheck\w+)", nm)) == set(SYMBOLS)
    L = ctypes.CDLL(_native.LIB_PATH)
    others = (set(_native.EXPORTS) | set(_native.EXPORTS_VERIFY) | set(_native.EXPORTS_BP_LOCALISE) | set(_native.EXPORTS_COMPOSITES) | set(_native.EXPORTS_STATEMENTS)
              | set(_native.EXPORTS_SEAL))
    for s in SYMBOLS:
        assert not s.startswith("zkp_") and not s.startswith("libzkp_") and s not in others
        assert getattr(L, s) is not None
    # every exported function of the library belongs to exactly one header's list
    assert set(re.findall(r" T ((?:lib)?zkp\w+)", nm)) == others | set(SYMBOLS)
    import libzkp_amd
    for name in ("check_key", "key_check_counters"):
        assert name in libzkp_amd.__all__ and callable(getattr(libzkp_amd, name))


def test_constants_agree_across_header_python_and_rust():
    from libzkp_amd import _native
    hdr, rs = open(HEADER).read(), open(os.path.join(ROOT, "rust", "hip_ffi_keycheck.rs")).read()
    assert sorted(set(re.findall(r"pub fn (zkpkeycheck_[a-z_0-9]+)\s*\(", rs))) == declared_symbols()
    assert not re.findall(r"pub fn (zkp_\w+)", rs)
    for name, value in list(STAGES.items()) + list(VERDICTS.items()):
        assert re.search(r"#define ZKP_KEYCHECK_%s\s+(\d+)u" % name, hdr).group(1) == str(value)
        assert getattr(_native, "KEYCHECK_" + name) == value
        assert "pub const ZKP_KEYCHECK_%s: u32 = %d;" % (name, value) in rs
    # the Rust struct names the report's fields in the header's order
    rust_fields = re.findall(r"pub (\w+): ", rs[rs.index("pub struct ZkpKeycheckReport"):rs.index('extern "C" {')])
    assert rust_fields == [f for f, _ in _native.KeyCheckReport._fields_]
    body = hdr[hdr.index("typedef struct zkp_keycheck_report"):hdr.index("} zkp_keycheck_report;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    c_fields = [n.strip().split("[")[0] for decl in re.findall(r"(?:u?int\d+_t|double|char)\s+([^;]+);", body) for n in decl.split(",")]
    assert c_fields == rust_fields


def test_argument_errors_come_before_any_device():
    from libzkp_amd import _native
    L = ctypes.CDLL(_native.LIB_PATH)
    L.zkp_hip_last_error.restype = ctypes.c_char_p
    f = L.zkpkeycheck_counters
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_double)] + [ctypes.POINTER(ctypes.c_uint64)] * 3 + [ctypes.c_int]
    assert f(None, None, None, None, 0) == 0 and f(None, None, None, None, 1) == 0
    ms, a, b = ctypes.c_double(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert f(ctypes.byref(ms), ctypes.byref(a), None, ctypes.byref(b), 0) == 0 and (ms.value, a.value, b.value) == (0.0, 0, 0)
    k = L.zkpkeycheck_key
    k.restype = ctypes.c_int
    k.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p]
    rep = _native.KeyCheckReport()
    assert k(2, b"x", 1, 1, ctypes.byref(rep)) == -3 and b"unknown circuit kind" in L.zkp_hip_last_error()
    assert k(0, None, 1, 1, ctypes.byref(rep)) == -3 and b"null pointer" in L.zkp_hip_last_error()
    assert k(0, b"x", 1, 1, None) == -3 and b"null pointer" in L.zkp_hip_last_error()
    assert k(0, b"x", 1, 8, ctypes.byref(rep)) == -3 and b"ZKP_KEYCHECK_" in L.zkp_hip_last_error()
