"""The composite-proof list call's host walk and digest lane on the host (no GPU), compiled from the header the kernels use
(composite_steps.h): comp_walk's verdict and step_comp_digest's digest against composite.parse_composite and hashlib for one container per
Err branch of CompositeProof::from_bytes, String::from_utf8's corner cases, the size and count limits on both sides, every order of
metadata keys, hashed lengths of every residue mod 64, and inner proofs of 10..13 bytes at every source alignment.  Every verdict and every
digest is compared.  The blobs are allocations of exactly their size."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from comp_build import comp, digest_of, entry, four_mib, proof, residue_family, straddle_family, u32
from libzkp_amd import composite

U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    return ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_composites.so"))


def reference_ok(c):
    try:
        composite.parse_composite(c)
        return True
    except composite.ProofFormatError:
        return False


def run(lib, containers, off=None):
    """statuses and digests of a list of containers, from a blob allocated at exactly its size"""
    data = b"".join(containers)
    blob = (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0")
    if off is None:
        off = np.concatenate(([0], np.cumsum([len(c) for c in containers]))).astype(np.uint64)
    n = len(off) - 1
    status, digests = np.full(n, 9, dtype=np.uint8), np.zeros((n, 32), dtype=np.uint8)
    lib.emul_comp_statuses(U64(n), blob, off.ctypes.data_as(ctypes.c_void_p), status.ctypes.data_as(ctypes.c_void_p), digests.ctypes.data_as(ctypes.c_void_p))
    return status.tolist(), [bytes(d) for d in digests]


def check(lib, cases):
    """cases: name -> (container, digest the lane must compute, or None where the walk must refuse the framing).  The verdict of every
    container is parse_composite's."""
    names = list(cases)
    status, digests = run(lib, [cases[k][0] for k in names])
    for k, st, dg in zip(names, status, digests):
        c, want = cases[k]
        assert st == (1 if reference_ok(c) else 2), k
        assert dg == (bytes(32) if want is None else want), k
    return dict(zip(names, status))


P3 = [proof(10), proof(47, salt=3), proof(298, scheme=2, salt=5)]
M3 = [(b"issuer", b"acme"), (b"epoch", u32(77)), (b"note", b"")]


def test_one_container_per_err_branch_of_from_bytes(lib):
    good = comp(P3, M3)
    d = digest_of(P3, M3)
    big = proof(10 + 900 * 1024 + 1)
    cases = {
        "good": (good, d),
        "empty_container": (comp(), digest_of([], [])),
        "short_11": (good[:11], None),
        "magic": (b"COMQ" + good[4:], None),
        "proofs_1001": (comp(P3, M3, nproofs=1001), None),
        "metadata_1001": (comp(P3, M3, nmeta=1001), None),
        "truncated_proof_length": (comp(P3[:1], nproofs=2, digest=b"\x0a\0"), None),
        "truncated_proof_data": (b"COMP" + u32(1) + u32(0) + u32(400) + proof(47) + bytes(32), None),
        "truncated_metadata_header": (comp(P3, M3[:1], nmeta=2, digest=b"ab"), None),
        "truncated_metadata_key": (comp(P3, digest=b"", nmeta=1) + u32(40) + b"k" * 39, None),
        "truncated_value_length": (comp(P3, digest=b"", nmeta=1) + u32(2) + b"kk" + b"\x01\0\0", None),
        "truncated_value": (comp(P3, digest=b"", nmeta=1) + u32(2) + b"kk" + u32(50) + bytes(49), None),
        "proof_of_9_bytes": (b"COMP" + u32(1) + u32(0) + u32(9) + bytes(9) + bytes(32), None),
        "proof_above_1_mib": (b"COMP" + u32(1) + u32(0) + u32((1 << 20) + 1) + bytes([2, 9]) + u32((1 << 20) - 9) + u32(0) + bytes((1 << 20) - 9) + bytes(32), None),
        "payload_above_900_kib": (comp([big]), None),
        "commitment_257": (comp([bytes([2, 9]) + u32(5) + u32(257) + bytes(262)]), None),
        "proof_length_mismatch": (comp([bytes([2, 9]) + u32(5) + u32(0) + bytes(6)]), None),
        "key_1025": (comp(P3, [(b"k" * 1025, b"v")]), None),
        "key_1024": (comp(P3, [(b"k" * 1024, b"v")]), digest_of(P3, [(b"k" * 1024, b"v")])),
        "value_65537": (comp(P3, [(b"k", bytes(65537))]), None),
        "value_65536": (comp(P3, [(b"k", bytes(range(256)) * 256)]), digest_of(P3, [(b"k", bytes(range(256)) * 256)])),
        "digest_missing": (good[:-32], None),
        "digest_cut": (good[:-1], None),
        "trailing_byte": (good + b"\0", None),
        "digest_mismatch": (good[:-1] + bytes([good[-1] ^ 1]), d),
        "hashed_byte_flipped": (good[:40] + bytes([good[40] ^ 0x10]) + good[41:], digest_of([P3[0], P3[1][:10] + bytes([P3[1][10] ^ 0x10]) + P3[1][11:], P3[2]], M3)),
        "version_3_inside": (comp([proof(40, version=3)]), digest_of([proof(40, version=3)], [])),      # the format layer does not read the version
    }
    assert len(cases["payload_above_900_kib"][0]) < (4 << 20)
    st = check(lib, cases)
    accepted = {"good", "empty_container", "key_1024", "value_65536", "version_3_inside"}
    assert {k for k, v in st.items() if v == 1} == accepted and set(st.values()) == {1, 2}


def test_offsets_that_run_backwards_or_leave_the_blob(lib):
    good = comp(P3, M3)
    n = len(good)
    # [0, n) good | [n, 5) backwards | [5, n) inside, but no container starts there
    assert run(lib, [good], off=np.array([0, n, 5, n], dtype=np.uint64))[0] == [1, 2, 2]
    # the blob is [5, n): [n, 0) runs backwards, [0, n) starts before the blob
    assert run(lib, [good], off=np.array([5, n, 0, n], dtype=np.uint64))[0] == [2, 2, 2]
    # ... and [0, n) | [n, n + 7) would end behind it
    assert run(lib, [good], off=np.array([0, n, n + 7, n], dtype=np.uint64))[0] == [1, 2, 2]
    assert run(lib, [good, good])[0] == [1, 1]


@pytest.mark.parametrize("key,ok", [
    (b"\xc0\x80", False), (b"\xed\xa0\x80", False), (b"\xf4\x90\x80\x80", False), (b"caf\xc3", False), (b"a\xe2\x82", False), (b"\xf0\x9f\x98", False),
    (b"\x80", False), (b"\xc1\xbf", False), (b"\xe0\x9f\xbf", False), (b"\xf0\x8f\xbf\xbf", False), (b"\xf5\x80\x80\x80", False), (b"\xff", False),
    (b"caf\xc3\xa9", True), (b"\xe2\x82\xac", True), (b"\xf0\x9f\x98\x80", True), (b"\xf4\x8f\xbf\xbf", True), (b"\xed\x9f\xbf", True), (b"\xee\x80\x80", True), (b"", True),
])
def test_metadata_keys_are_judged_as_string_from_utf8_judges_them(lib, key, ok):
    c = comp(P3[:1], [(b"a", b"1"), (key, b"value"), (b"z", b"2")])
    assert reference_ok(c) is ok
    check(lib, {"key": (c, digest_of(P3[:1], [(b"a", b"1"), (key, b"value"), (b"z", b"2")]) if ok else None)})
    assert lib.emul_comp_utf8_ok(key, len(key)) == (1 if ok else 0)


def test_exactly_4_mib_is_accepted_and_one_byte_more_is_refused(lib):
    (at, proofs, m_at), (over, _, _) = four_mib()
    assert (len(at), len(over)) == (4 << 20, (4 << 20) + 1)
    st = check(lib, {"at": (at, digest_of(proofs, m_at)), "over": (over, None)})
    assert st == {"at": 1, "over": 2}


def test_proof_and_metadata_counts_of_1000_and_1001(lib):
    p1000, p1001 = [proof(10 + k % 4, salt=k) for k in range(1000)], [proof(10, salt=k) for k in range(1001)]
    m1000 = [(b"key%04d" % (999 - k), bytes(k % 5)) for k in range(1000)]
    m1001 = m1000 + [(b"one more", b"")]
    st = check(lib, {"p1000": (comp(p1000), digest_of(p1000, [])), "p1001": (comp(p1001), None),
                     "m1000": (comp([], m1000), digest_of([], m1000)), "m1001": (comp([], m1001), None)})
    assert st == {"p1000": 1, "p1001": 2, "m1000": 1, "m1001": 2}


def test_metadata_order_duplicates_and_prefix_keys(lib):
    metas = {
        "unsorted": [(b"zeta", b"1"), (b"alpha", b"22"), (b"mid", b"333"), (b"Alpha", b"4")],
        "duplicate_last_wins": [(b"k", b"first"), (b"j", b"x"), (b"k", b"second, longer"), (b"a", b""), (b"k", b"3")],
        "prefixes": [(b"abc", b"3"), (b"ab", b"2"), (b"", b"0"), (b"a", b"1"), (b"abcd", b"4"), (b"ab\x00", b"5")],
        "multibyte": [(b"\xf0\x9f\x98\x80", b"4"), (b"\xef\xbf\xbf", b"3"), (b"\xc3\xa9", b"2"), (b"z", b"1"), (b"\xe2\x82\xac", b"x")],
        "all_the_same": [(b"same", bytes([k])) for k in range(7)],
    }
    cases = {name: (comp(P3[:2], m), digest_of(P3[:2], m)) for name, m in metas.items()}
    assert set(check(lib, cases).values()) == {1}
    # the digest is not the one of the serialized order, nor of the first value
    assert digest_of(P3[:2], metas["unsorted"]) != hashlib.sha256(b"COMPOSITE_PROOF:" + u32(2) + b"".join(P3[:2]) + b"".join(entry(k, v) for k, v in metas["unsorted"])).digest()
    wrong = comp(P3[:2], metas["duplicate_last_wins"], digest=digest_of(P3[:2], metas["duplicate_last_wins"][:2] + metas["duplicate_last_wins"][3:4]))
    check(lib, {"first_value_hashed": (wrong, digest_of(P3[:2], metas["duplicate_last_wins"]))})
    # the walk's own output: entries after de-duplication, their offsets in hash order
    c = comp(P3[:2], metas["duplicate_last_wins"])
    out, order = (ctypes.c_uint64 * 6)(), (ctypes.c_uint32 * 1000)()
    blob = (ctypes.c_uint8 * len(c)).from_buffer_copy(c)
    assert lib.emul_comp_walk(blob, U64(0), U64(len(c)), U64(0), U64(len(c)), out, order) == 1
    start = 12 + sum(4 + len(p) for p in P3[:2])
    at, offs = start, []
    for k, v in metas["duplicate_last_wins"]:
        offs.append(at); at += 8 + len(k) + len(v)
    assert list(out) == [1, 2, 3, at, 20 + 57 + (8 + 1 + 0) + (8 + 1 + 1) + (8 + 1 + 1), 57]
    assert list(order[:3]) == [offs[3], offs[1], offs[4]]                     # a, j, the last k


def test_hashed_lengths_of_every_residue_mod_64(lib):
    cases, residues = {}, set()
    for c, proofs, m in residue_family():
        cases["value_%d" % len(m[0][1])] = (c, digest_of(proofs, m))
        residues.add((20 + 10 + 8 + 1 + len(m[0][1])) % 64)
    assert residues == set(range(64)) and {55, 56, 63, 0, 1} <= residues
    assert set(check(lib, cases).values()) == {1}
    # the same lengths from the proofs alone (no metadata: the stream ends inside a proof)
    cases = {"proof_%d" % n: (comp([proof(n)]), digest_of([proof(n)], [])) for n in range(10, 141)}
    assert set(check(lib, cases).values()) == {1}


def test_short_inner_proofs_at_every_source_alignment(lib):
    """words of the stream straddle the segments' boundaries: proofs of 10..13 bytes lie 14..17 bytes apart, behind 0..7 stray bytes"""
    containers, want = [], []
    for c, proofs, m in straddle_family():
        containers.append(c); want.append(None if proofs is None else digest_of(proofs, m))
    status, digests = run(lib, containers)
    for c, st, dg, w in zip(containers, status, digests, want):
        assert st == (1 if reference_ok(c) else 2) == (2 if w is None else 1)
        assert dg == (w or bytes(32))
    # segments longer than a block (fetched a block at a time) at every alignment, with segment ends at every phase of a block
    long_ones, want_long = [], []
    for before in range(8):
        proofs = [proof(n, salt=before) for n in (63, 64, 65, 130 + before, 200, 298, 1478)]
        m = [(b"long", bytes(range(200)) + bytes(before))]
        long_ones += [bytes(before + 1), comp(proofs, m)]; want_long += [None, digest_of(proofs, m)]
    status, digests = run(lib, long_ones)
    assert status == [2, 1] * 8 and digests == [w or bytes(32) for w in want_long]
    # the last container ends at the blob's last byte; cut there by one byte, it is refused and nothing behind the blob is read
    status, _ = run(lib, containers[:-1] + [containers[-1][:-1]])
    assert status[-1] == 2 and status[:-1] == [1 if w else 2 for w in want[:-1]]


def test_pack_and_fold_steps(lib):
    proofs = [proof(n, salt=n) for n in (10, 11, 12, 13, 64, 65, 298, 1478)]
    for before in range(4):
        data = bytes(before) + comp(proofs)
        blob = (ctypes.c_uint8 * len(data)).from_buffer_copy(data)
        src, at = [], before + 12
        for p in proofs:
            src.append(at + 4); at += 4 + len(p)
        src = np.array(src, dtype=np.uint64)
        poff = np.concatenate(([0], np.cumsum([len(p) for p in proofs]))).astype(np.uint64)
        packed = np.full(int(poff[-1]) + 8, 0xA5, dtype=np.uint8)
        lib.emul_comp_pack(packed.ctypes.data_as(ctypes.c_void_p), poff.ctypes.data_as(ctypes.c_void_p), blob, U64(len(data)), src.ctypes.data_as(ctypes.c_void_p), U64(len(proofs)))
        assert packed[:-8].tobytes() == b"".join(proofs) and (packed[-8:] == 0xA5).all()
    status = np.array([1, 2, 1, 1, 1], dtype=np.uint8)
    ok = np.array([1, 1, 1, 0, 1, 1, 2], dtype=np.uint8)
    env0 = np.array([0, 2, 2, 2, 5, 7], dtype=np.uint64)
    lib.emul_comp_fold(status.ctypes.data_as(ctypes.c_void_p), ok.ctypes.data_as(ctypes.c_void_p), env0.ctypes.data_as(ctypes.c_void_p), U64(5))
    assert status.tolist() == [1, 2, 1, 0, 0]
    assert lib.emul_comp_lane_bytes() == 40
