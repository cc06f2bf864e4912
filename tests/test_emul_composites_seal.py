"""The sealing call's host plan and both step functions on the host (no GPU), compiled from the header the kernels use (composite_seal.h),
the lanes as a loop: statuses, out_off and bytes of libzkp_seal_composites' emulation (tests/emul/emul_composites_seal.cpp: emul_seal).

Reference bytes never come from the code under test: per container they come from comp_build.comp (hashlib, keys as raw bytes) and, where
str keys can say it, from composite._serialize_composite / create_composite_proof / create_proof_with_metadata.  All comparisons are byte
equality.  Input blobs are allocations of exactly their size; the output is prefilled with 0xA5."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from comp_build import comp, entry, four_mib, proof, residue_family, straddle_family, u32
from libzkp_amd import composite

U64 = ctypes.c_uint64
SEALED, REFUSED, UNREADABLE, FAILED_OP = 1, 2, 3, 0


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_composites_seal.so"))
    L.emul_seal.restype = ctypes.c_int
    L.emul_seal.argtypes = [U64, ctypes.c_void_p, ctypes.c_void_p, U64] + [ctypes.c_void_p] * 5 + [U64, ctypes.c_void_p, ctypes.c_void_p]
    return L


def exact(data):
    return (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")


def offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths, dtype=np.uint64))).astype(np.uint64)


def seal(lib, lists, metas=None, stray=0, lead=0, cap=None, codes=None):
    """lists: per container its envelopes; metas: per container its metadata run in wire form.  `stray` bytes of another envelope lie in
    front of the first one.  Returns (rc, statuses, out_off, the whole output buffer: lead | cap | 8 guard bytes)."""
    envs = [bytes(stray)] + [p for lst in lists for p in lst]
    env_blob, env_off = exact(b"".join(envs)), offsets([len(e) for e in envs])
    first = (offsets([len(lst) for lst in lists]) + np.uint64(1)).astype(np.uint64)
    n = len(lists)
    meta_blob = meta_off = None
    if metas is not None:
        meta_blob, meta_off = exact(b"".join(metas)), offsets([len(m) for m in metas])
    P = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    code = None if codes is None else np.array([1] + list(codes), dtype=np.uint8)
    status, out_off = np.full(n, 9, dtype=np.uint8), np.full(n + 1, 9, dtype=np.uint64)
    if cap is None:                                   # ask for the size first, with no room
        rc = lib.emul_seal(n, env_blob, P(env_off), len(envs), P(code), P(first), meta_blob, P(meta_off), None, 0, P(out_off), P(status))
        cap = int(out_off[n])
        assert rc == (-3 if cap else rc) and rc in (-3, 0, 1)
    out = np.full(lead + cap + 8, 0xA5, dtype=np.uint8)
    rc = lib.emul_seal(n, env_blob, P(env_off), len(envs), P(code), P(first), meta_blob, P(meta_off), ctypes.c_void_p(out.ctypes.data + lead), cap, P(out_off), P(status))
    return rc, status.tolist(), [int(x) for x in out_off], out


def sealed_bytes(out, out_off, lead=0):
    return [out[lead + out_off[i]:lead + out_off[i + 1]].tobytes() for i in range(len(out_off) - 1)]


def guards_intact(out, out_off, lead=0):
    return (out[:lead + out_off[0]] == 0xA5).all() and (out[lead + out_off[-1]:] == 0xA5).all()


def wire(meta):
    return b"".join(entry(k, v) for k, v in meta)


def check(lib, cases, **kw):
    """cases: name -> (envelopes, metadata pairs with raw-bytes keys or a wire-form run, expected status).  A sealed container must equal
    comp_build.comp's bytes; any other takes zero bytes."""
    names = list(cases)
    metas = [m if isinstance(m, bytes) else wire(m) for _, m, _ in cases.values()]
    rc, status, off, out = seal(lib, [c[0] for c in cases.values()], metas, **kw)
    got = sealed_bytes(out, off, kw.get("lead", 0))
    for k, st, b in zip(names, status, got):
        envs, meta, want = cases[k]
        assert st == want, k
        assert b == (comp(envs, meta) if want == SEALED else b""), k
    assert rc == (0 if all(s == SEALED for s in status) else 1) and guards_intact(out, off, kw.get("lead", 0))
    return dict(zip(names, got))


G = proof(47, salt=3)


def test_one_container_per_refusal_on_both_sides_of_each_limit(lib):
    p1000, p1001 = [proof(10 + k % 4, salt=k) for k in range(1000)], [proof(10, salt=k) for k in range(1001)]
    m1000 = [(b"key%04d" % (999 - k), bytes(k % 5)) for k in range(1000)]
    big = bytes([2, 9]) + u32(900 * 1024 + 1) + u32(0) + bytes(900 * 1024 + 1)
    big_at = bytes([2, 9]) + u32(900 * 1024) + u32(0) + bytes(900 * 1024)
    cases = {
        "good": ([G, proof(10)], [(b"issuer", b"acme"), (b"epoch", u32(77)), (b"note", b"")], SEALED),
        "empty_list": ([], [], REFUSED),
        "empty_list_with_metadata": ([], [(b"k", b"v")], REFUSED),
        "envelope_of_9_bytes": ([G, bytes(9)], [], REFUSED),
        "envelope_of_10_bytes": ([proof(10)], [], SEALED),
        "length_mismatch": ([bytes([2, 9]) + u32(5) + u32(0) + bytes(6)], [], REFUSED),
        "payload_900_kib_plus_1": ([big], [], REFUSED),
        "payload_900_kib": ([big_at], [], SEALED),
        "commitment_257": ([bytes([2, 9]) + u32(5) + u32(257) + bytes(262), G], [], REFUSED),
        "commitment_256": ([bytes([2, 9]) + u32(5) + u32(256) + bytes(261)], [], SEALED),
        "above_1_mib": ([bytes([2, 9]) + u32((1 << 20) - 9) + u32(0) + bytes((1 << 20) - 9)], [], REFUSED),
        "refused_beats_unreadable": ([bytes(9)], [(b"k" * 1025, b"")], REFUSED),
        "proofs_1000": (p1000, [], SEALED),
        "proofs_1001": (p1001, [], UNREADABLE),
        "metadata_1000": ([G], m1000, SEALED),
        "metadata_1001": ([G], m1000 + [(b"one more", b"")], UNREADABLE),
        "key_1024": ([G], [(b"k" * 1024, b"v")], SEALED),
        "key_1025": ([G], [(b"k" * 1025, b"v")], UNREADABLE),
        "value_65536": ([G], [(b"k", bytes(range(256)) * 256)], SEALED),
        "value_65537": ([G], [(b"k", bytes(65537))], UNREADABLE),
        "repeated_key": ([G], [(b"k", b"first"), (b"j", b"x"), (b"k", b"last")], UNREADABLE),
        "truncated_run": ([G], wire([(b"kk", bytes(50))])[:-1], UNREADABLE),
        "truncated_value_length": ([G], u32(2) + b"kk" + b"\x01\0\0", UNREADABLE),
        "truncated_key": ([G], u32(40) + b"k" * 39, UNREADABLE),
        "bytes_left_over": ([G], wire([(b"kk", b"v")]) + b"\0", UNREADABLE),
        "version_3_inside": ([proof(40, version=3)], [], SEALED),      # the format layer does not read the version
    }
    got = check(lib, cases, stray=3, lead=1)
    # the same bytes from the Python that exists today, where str keys can say it
    assert got["good"] == composite._serialize_composite([G, proof(10)], {"issuer": b"acme", "epoch": u32(77), "note": b""})
    assert got["envelope_of_10_bytes"] == composite.create_composite_proof([proof(10)])
    assert got["key_1024"] == composite.create_proof_with_metadata(G, {"k" * 1024: b"v"})
    for k in ("good", "proofs_1000", "metadata_1000", "value_65536", "payload_900_kib"):
        composite.parse_composite(got[k])


def test_exactly_4_mib_is_sealed_and_one_byte_more_is_not(lib):
    (at, proofs, m_at), (over, _, m_over) = four_mib()
    got = check(lib, {"at": (proofs, m_at, SEALED), "over": (proofs, m_over, UNREADABLE)}, stray=1, lead=3)
    assert got["at"] == at and len(at) == 4 << 20 and len(over) == (4 << 20) + 1


@pytest.mark.parametrize("key,ok", [
    (b"\xc0\x80", False), (b"\xed\xa0\x80", False), (b"\xf4\x90\x80\x80", False), (b"caf\xc3", False), (b"a\xe2\x82", False), (b"\xf0\x9f\x98", False),
    (b"\x80", False), (b"\xc1\xbf", False), (b"\xe0\x9f\xbf", False), (b"\xf0\x8f\xbf\xbf", False), (b"\xf5\x80\x80\x80", False), (b"\xff", False),
    (b"caf\xc3\xa9", True), (b"\xe2\x82\xac", True), (b"\xf0\x9f\x98\x80", True), (b"\xf4\x8f\xbf\xbf", True), (b"\xed\x9f\xbf", True), (b"\xee\x80\x80", True), (b"", True),
])
def test_metadata_keys_are_judged_as_string_from_utf8_judges_them(lib, key, ok):
    m = [(b"a", b"1"), (key, b"value"), (b"z", b"2")]
    got = check(lib, {"key": ([G], m, SEALED if ok else UNREADABLE)})
    if ok:
        assert got["key"] == composite.create_proof_with_metadata(G, {"a": b"1", key.decode("utf-8"): b"value", "z": b"2"})


def test_every_order_of_three_keys_with_a_prefix_among_them(lib):
    base = [(b"ab", b"2"), (b"a", b"11"), (b"b", b"")]
    cases = {"".join(k.decode() + "," for k, _ in perm): ([G, proof(11)], list(perm), SEALED) for perm in itertools.permutations(base)}
    got = check(lib, cases, stray=2, lead=2)
    assert len(got) == 6 and len({b[-32:] for b in got.values()}) == 1 and len(set(got.values())) == 6          # one digest, six encodings
    for name, perm in zip(cases, itertools.permutations(base)):
        assert got[name] == composite._serialize_composite([G, proof(11)], {k.decode(): v for k, v in perm})
    check(lib, {"multibyte": ([G], [(b"\xf0\x9f\x98\x80", b"4"), (b"\xef\xbf\xbf", b"3"), (b"\xc3\xa9", b"2"), (b"z", b"1"), (b"", b"0"), (b"ab\x00", b"5")], SEALED)})


def test_hashed_lengths_of_every_residue_mod_64(lib):
    fam = list(residue_family())
    cases = {"value_%d" % i: (proofs, m, SEALED) for i, (_, proofs, m) in enumerate(fam)}
    assert {(20 + 10 + 8 + 1 + len(m[0][1])) % 64 for _, _, m in fam} == set(range(64))
    got = check(lib, cases, stray=5, lead=1)
    assert [got["value_%d" % i] for i in range(len(fam))] == [c for c, _, _ in fam]
    # the same lengths from the proofs alone, without a metadata array
    lists = [[proof(n)] for n in range(10, 141)]
    rc, status, off, out = seal(lib, lists, None, stray=1, lead=2)
    assert rc == 0 and status == [SEALED] * 131 and guards_intact(out, off, 2)
    assert sealed_bytes(out, off, 2) == [composite.create_composite_proof(lst) for lst in lists]


def test_pieces_begin_at_every_source_and_destination_alignment(lib):
    """straddle_family's proofs of 10..13 bytes: consecutive pieces lie 14..17 bytes apart, behind 0..7 stray source bytes and 0..3 bytes
    past a dword of the destination"""
    fam = [(c, proofs, m) for c, proofs, m in straddle_family() if proofs is not None]
    assert len(fam) == 8 * 64
    for stray, lead in itertools.product(range(8), range(4)):
        part = fam[64 * stray:64 * stray + 64] if lead else fam
        rc, status, off, out = seal(lib, [p for _, p, _ in part], [wire(m) for _, _, m in part], stray=stray, lead=lead)
        assert rc == 0 and status == [SEALED] * len(part) and guards_intact(out, off, lead)
        assert sealed_bytes(out, off, lead) == [c for c, _, _ in part]
    # pieces longer than a wave's pass of dwords, with ends at every phase
    for stray in range(4):
        proofs = [proof(n, salt=stray) for n in (63, 64, 65, 130 + stray, 255, 256, 257, 298, 1478, 3527)]
        m = [(b"long", bytes(range(200)) + bytes(stray)), (b"", b"")]
        check(lib, {"a": (proofs, m, SEALED), "b": (proofs[::-1], m[::-1], SEALED)}, stray=stray, lead=stray)


def test_a_buffer_that_is_too_small_is_left_alone_and_the_size_needed_comes_back(lib):
    lists, metas = [[G], [], [proof(13), proof(10)]], [wire([(b"k", b"v")]), b"", b""]
    rc, status, off, out = seal(lib, lists, metas, lead=4)
    need = off[-1]
    assert rc == 1 and status == [SEALED, REFUSED, SEALED] and need == len(comp([G], [(b"k", b"v")])) + len(comp(lists[2])) and off[1] == off[2]
    rc, status2, off2, out2 = seal(lib, lists, metas, lead=4, cap=need - 1)
    assert rc == -3 and off2 == off and status2 == status and (out2 == 0xA5).all()
    rc, _, off3, out3 = seal(lib, lists, metas, lead=4, cap=need + 5)
    assert rc == 1 and off3 == off and out3[4:4 + need].tobytes() == out[4:4 + need].tobytes() and guards_intact(out3, off3, 4)
    # nothing sealed: nothing written, no room needed
    rc, status, off, out = seal(lib, [[], [bytes(9)]], None, lead=2, cap=0)
    assert rc == 1 and status == [REFUSED, REFUSED] and off == [0, 0, 0] and (out == 0xA5).all()


def test_the_batch_forms_codes_a_failed_op_fails_its_container_alone(lib):
    a, b, c = proof(30), proof(31), proof(32)
    rc, status, off, out = seal(lib, [[a], [b, bytes(0)], [c], []], [b"", b"", wire([(b"k", b"")]), b""], codes=[1, 1, 2, 1])
    assert rc == 1 and status == [SEALED, FAILED_OP, SEALED, REFUSED] and guards_intact(out, off)
    assert sealed_bytes(out, off) == [comp([a]), b"", comp([c], [(b"k", b"")]), b""]
    assert lib.emul_seal_piece_bytes() == 32


def test_the_program_with_its_own_main_runs_clean_under_the_sanitizers():
    import __graft_entry__ as ge
    exe = ge.build_emul_composites_seal_program()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "emul_composites_seal ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
