"""The mixed verifier's glue steps on the host (no GPU): libzkp_amd/csrc/venv_steps.h compiled from the header the kernels use
(tests/emul/emul_verify_mixed.cpp) -- the classification of an envelope against a Python restatement built on composite.parse_proof, the
blob -> row copy at every alignment, the row plan, and the verdicts' way back to the caller's order."""
import ctypes
import os

import numpy as np
import pytest

from libzkp_amd import composite

U64, U32, VP = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p
REC = np.dtype([("scheme", "<u4"), ("len", "<u4"), ("p0", "<u8"), ("p1", "<u8"), ("jobs", "<u4"), ("reserved", "<u4")])
NO_ROW = 0xFFFFFFFF
CAPS = {1: 4096, 2: 4096, 3: 4096, 4: 4096, 5: 8192, 6: 1 << 20}


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build_emul()
    L = ctypes.CDLL(os.path.join(ge.EMUL_DIR, "_build", "libemul_verify_mixed.so"))
    L.emul_ve_classify.argtypes = [U64, VP, VP, VP, VP]
    L.emul_ve_classify.restype = None
    L.emul_ve_consistency_jobs.argtypes = [VP, U64]
    L.emul_ve_weight.argtypes = [VP, VP, U64, U64]
    L.emul_ve_scheme_weight.argtypes = [U32, VP, U64]
    L.emul_ve_scheme_weight.restype = U32
    L.emul_ve_plan.argtypes = [U64, VP, VP, VP]
    L.emul_ve_plan_uniform.argtypes = [U64, U32, U32]
    L.emul_ve_copy.argtypes = [VP, VP, U32, VP, VP, U32]
    L.emul_ve_copy.restype = None
    L.emul_ve_pipeline.argtypes = [U64, VP, VP, VP, VP, VP, VP, VP, VP, VP]
    for f in (L.emul_ve_consistency_jobs, L.emul_ve_weight, L.emul_ve_plan, L.emul_ve_plan_uniform, L.emul_ve_pipeline, L.emul_ve_record_bytes):
        f.restype = U32
    assert L.emul_ve_record_bytes() == 32 == REC.itemsize
    return L


def P(a):
    return a.ctypes.data_as(VP)


# ---- the restatement: verify_single_proof up to the cryptographic check (performance.rs:270-293, proof_helpers.rs:156-247)
def ref_jobs(env):
    if len(env) < 14:
        return 0
    k = int.from_bytes(env[10:14], "little")
    return k - 1 if 1 <= k < (1 << 20) and 10 + 4 + 32 * k + (4 + 672 + 32) * (k - 1) + 32 <= len(env) else 0


def ref_classify(env, expect):
    """(scheme or 0, p0, p1, jobs)"""
    try:
        version, scheme, payload, commitment = composite.parse_proof(env)
    except composite.ProofFormatError:
        return (0, 0, 0, 0)
    if version != composite.PROOF_VERSION or expect not in (None, 0, scheme):
        return (0, 0, 0, 0)
    u64 = lambda b: int.from_bytes(b, "little")  # noqa: E731
    if scheme == 1 and len(payload) >= 20 and len(commitment) == 32 and u64(payload[:8]) <= u64(payload[8:16]):
        return (1, u64(payload[:8]), u64(payload[8:16]), 0)
    if scheme == 2 and len(commitment) == 32:
        return (2, 0, 0, 0)
    if scheme == 3 and len(payload) >= 12 and len(commitment) == 32:
        return (3, u64(payload[:8]), 0, 0)
    if scheme == 4 and len(commitment) == 32 and len(payload) >= 4 and 1 <= u64(payload[:4]) <= 64 and len(payload) > 4 + 8 * u64(payload[:4]):
        return (4, 0, 0, 0)
    if scheme == 5 and len(commitment) == 32 and len(payload) >= 16:
        return (5, u64(payload[:8]), 0, 0)
    if scheme == 6:
        return (6, 0, 0, ref_jobs(env))
    return (0, 0, 0, 0)


def classify(L, envs, expect=None, off=None, blob=None):
    blob = np.frombuffer(b"".join(envs) + b"\0", dtype=np.uint8) if blob is None else blob
    if off is None:
        off = np.concatenate(([0], np.cumsum([len(e) for e in envs]))).astype(np.uint64)
    n = len(off) - 1
    ex = None if expect is None else np.asarray(expect, dtype=np.uint8)
    rec = np.zeros(n, dtype=REC)
    L.emul_ve_classify(n, P(blob), P(off), None if ex is None else P(ex), P(rec))
    return rec


def make_env(rng, scheme, version=2, plen=None, clen=32, delta=0, payload=None):
    """an envelope whose header says (plen, clen) and whose length is 10 + plen + clen + delta"""
    if payload is None:
        payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
    plen = len(payload) if plen is None else plen
    body = payload + rng.integers(0, 256, clen, dtype=np.uint8).tobytes()
    body = body[:len(body) + delta] if delta <= 0 else body + bytes(delta)
    return bytes([version, scheme]) + plen.to_bytes(4, "little") + clen.to_bytes(4, "little") + body


def random_env(rng):
    scheme = int(rng.integers(0, 8))
    version = 2 if rng.random() < 0.9 else int(rng.choice([0, 1, 3]))
    clen = int(rng.choice([32] * 6 + [0, 31, 33, 256, 257]))
    delta = int(rng.choice([0] * 8 + [-1, 1]))
    if scheme == 1:
        lo, hi = (int(x) for x in rng.integers(0, 2**64, 2, dtype=np.uint64))
        if rng.random() < 0.7 and lo > hi:
            lo, hi = hi, lo
        payload = lo.to_bytes(8, "little") + hi.to_bytes(8, "little") + rng.integers(0, 256, int(rng.choice([0, 3, 4, 40])), dtype=np.uint8).tobytes()
    elif scheme == 4:
        count = int(rng.choice([0, 1, 5, 64, 65]))
        payload = count.to_bytes(4, "little") + rng.integers(0, 256, 8 * count + int(rng.choice([0, 1, 256])), dtype=np.uint8).tobytes()
        if rng.random() < 0.1:
            payload = payload[:int(rng.integers(0, 5))]
    elif scheme == 6:
        k = int(rng.choice([0, 1, 2, 5]))
        need = 4 + 32 * k + (4 + 672 + 32) * max(k - 1, 0)
        payload = k.to_bytes(4, "little") + rng.integers(0, 256, max(need - 4 + int(rng.choice([0, 0, -1])), 0), dtype=np.uint8).tobytes()
        if rng.random() < 0.1:
            payload = payload[:3]
    else:
        payload = rng.integers(0, 256, int(rng.choice([0, 7, 8, 11, 12, 15, 16, 19, 20, 256])), dtype=np.uint8).tobytes()
    return make_env(rng, scheme, version, None, clen, delta, payload)


def assert_records(rec, envs, expect):
    for i, e in enumerate(envs):
        want = ref_classify(e, None if expect is None else int(expect[i]))
        got = (int(rec["scheme"][i]), int(rec["p0"][i]), int(rec["p1"][i]), int(rec["jobs"][i]))
        assert got == want, (i, e[:14].hex(), len(e), None if expect is None else int(expect[i]), got, want)
        assert int(rec["len"][i]) == len(e)


def test_random_headers_against_the_restatement(lib):
    rng = np.random.default_rng(2611)
    total, seen = 0, set()
    for batch in range(12):
        envs = [random_env(rng) for _ in range(200)]
        expect = None if batch % 3 == 0 else rng.integers(0, 8, len(envs), dtype=np.uint8)
        rec = classify(lib, envs, expect)
        assert_records(rec, envs, expect)
        total += len(envs)
        seen |= {int(s) for s in rec["scheme"]}
    assert total >= 2000 and seen == {0, 1, 2, 3, 4, 5, 6}          # every scheme was accepted somewhere, and something was rejected


def test_every_scheme_byte_against_every_expected_value(lib):
    rng = np.random.default_rng(5)
    envs, expect = [], []
    for scheme in range(8):
        for ex in list(range(8)) + [9, 255]:
            payload = {1: (3).to_bytes(8, "little") + (9).to_bytes(8, "little") + bytes(8), 4: (2).to_bytes(4, "little") + bytes(16 + 256)}.get(scheme, bytes(64))
            envs.append(make_env(rng, scheme, payload=payload)); expect.append(ex)
    rec = classify(lib, envs, expect)
    assert_records(rec, envs, expect)
    for i, (e, ex) in enumerate(zip(envs, expect)):
        assert (rec["scheme"][i] != 0) == (1 <= e[1] <= 6 and ex in (0, e[1]))
    assert_records(classify(lib, envs, None), envs, None)


def test_length_fields_at_and_one_past_every_limit(lib):
    rng = np.random.default_rng(6)
    big = 900 * 1024
    envs = [
        make_env(rng, 6, plen=0, clen=0),                         # 10 bytes: the shortest Proof::from_bytes accepts
        make_env(rng, 6, plen=0, clen=0)[:9],                     # 9: too short for a header
        b"",
        make_env(rng, 6, plen=big, clen=32), make_env(rng, 6, plen=big + 1, clen=32),
        make_env(rng, 6, plen=64, clen=256), make_env(rng, 6, plen=64, clen=257),
        make_env(rng, 6, plen=big, clen=256),                     # the longest consistent envelope
        make_env(rng, 6, plen=64, clen=32, delta=1), make_env(rng, 6, plen=64, clen=32, delta=-1),
        make_env(rng, 6, plen=(1 << 20) - 42, clen=32), make_env(rng, 6, plen=(1 << 20) - 41, clen=32),      # 2^20 and 2^20 + 1 bytes in all
        make_env(rng, 1, plen=20, clen=32, payload=bytes(20)), make_env(rng, 1, payload=bytes(19)), make_env(rng, 1, payload=bytes(20), clen=31),
        make_env(rng, 1, payload=(2).to_bytes(8, "little") + (1).to_bytes(8, "little") + bytes(4)),              # min > max
        make_env(rng, 1, payload=(2).to_bytes(8, "little") + (2).to_bytes(8, "little") + bytes(4)),
        make_env(rng, 3, payload=bytes(12)), make_env(rng, 3, payload=bytes(11)), make_env(rng, 3, payload=bytes(12), clen=33),
        make_env(rng, 5, payload=bytes(16)), make_env(rng, 5, payload=bytes(15)), make_env(rng, 5, payload=bytes(16), clen=0),
        make_env(rng, 2, payload=bytes(256)), make_env(rng, 2, payload=bytes(256), clen=31), make_env(rng, 2, payload=b""),
    ]
    for count in (0, 1, 64, 65):
        for extra in (0, 1):
            envs.append(make_env(rng, 4, payload=count.to_bytes(4, "little") + bytes(8 * count + extra)))
    envs += [make_env(rng, 4, payload=bytes(3)), make_env(rng, 4, payload=(1).to_bytes(4, "little") + bytes(9), clen=31)]
    assert len(envs[10]) == 1 << 20 and len(envs[11]) == (1 << 20) + 1
    rec = classify(lib, envs)
    assert_records(rec, envs, None)
    live = [int(s) for s in rec["scheme"]]
    assert live[:12] == [6, 0, 0, 6, 0, 6, 0, 6, 0, 0, 0, 0]
    assert live[12:26] == [1, 0, 0, 0, 1, 3, 0, 0, 5, 0, 0, 2, 0, 2]
    assert live[26:] == [0, 0, 0, 4, 0, 4, 0, 0, 0, 0]             # membership: count 0 | 1 | 64 | 65, nothing / something behind the set


def test_offsets_that_run_backwards_or_leave_the_blob(lib):
    rng = np.random.default_rng(7)
    a, b, c = make_env(rng, 2, payload=bytes(256)), make_env(rng, 3, payload=bytes(100)), make_env(rng, 5, payload=bytes(40))
    blob = np.frombuffer(a + b + c, dtype=np.uint8)
    A, B, C = len(a), len(a) + len(b), len(blob)
    for off in ([0, A, B, C], [0, B, A, C], [0, A, A, C], [0, A, C + 1, C], [0, C + 5, B, C], [A, 0, B, C], [0, A, B, B], [C, B, A, 0], [0, 0, 0, 0]):
        o = np.array(off, dtype=np.uint64)
        rec = classify(lib, None, off=o, blob=blob)
        for i in range(3):
            lo, hi = off[i], off[i + 1]
            inside = lo <= hi and off[0] <= lo and hi <= off[3]
            want = ref_classify(bytes(blob[lo:hi]), None) if inside else (0, 0, 0, 0)
            assert (int(rec["scheme"][i]), int(rec["p0"][i]), int(rec["p1"][i]), int(rec["jobs"][i])) == want, (off, i)
            assert int(rec["len"][i]) == (hi - lo if inside else 0)
            if inside:
                assert lib.emul_ve_weight(P(blob), P(o), 3, i) == (1 if hi - lo < 2 or blob[lo + 1] not in (1, 6) else 2 if blob[lo + 1] == 1 else max(ref_jobs(bytes(blob[lo:hi])), 0))
            else:
                assert lib.emul_ve_weight(P(blob), P(o), 3, i) == 1
    assert [int(s) for s in classify(lib, None, off=np.array([0, A, B, C], dtype=np.uint64), blob=blob)["scheme"]] == [2, 3, 5]


def test_the_consistency_job_rule_is_the_one_the_verifier_reads(lib):
    for k in (0, 1, 2, 5, (1 << 20) - 1, 1 << 20):
        need = 10 + 4 + 32 * k + (4 + 672 + 32) * max(k - 1, 0) + 32
        for length in (13, 14, need - 1, need, need + 7):
            if length < 0 or length > 4096:
                continue
            env = np.zeros(max(length, 16), dtype=np.uint8)
            env[10:14] = np.frombuffer(k.to_bytes(4, "little"), dtype=np.uint8)
            assert lib.emul_ve_consistency_jobs(P(env), length) == ref_jobs(env[:length].tobytes()), (k, length)
    env = np.zeros(16, dtype=np.uint8)
    env[10:14] = np.frombuffer(((1 << 20) - 1).to_bytes(4, "little"), dtype=np.uint8)
    assert lib.emul_ve_consistency_jobs(P(env), 1 << 30) == (1 << 20) - 2 and lib.emul_ve_consistency_jobs(P(env), 1 << 20) == 0


def test_the_weight_rule_is_one_for_a_packed_list_and_for_a_containers_envelopes(lib):
    """ve_weight (envelope i of a packed list: the mixed verifier's and the statements call's fan-out) and ve_scheme_weight (scheme byte,
    envelope, length: a container's inner envelopes) give the same weight: 2 for a range envelope, k - 1 for a consistency envelope that
    holds what its k announces and 0 for one that does not, 1 for everything else, scheme bytes that name no scheme included"""
    rng = np.random.default_rng(21)

    def consistency(k, short=0):
        need = 4 + 32 * k + (4 + 672 + 32) * max(k - 1, 0)
        return make_env(rng, 6, payload=k.to_bytes(4, "little") + bytes(need - 4 - short))

    envs = [make_env(rng, s, payload=bytes(40)) for s in (0, 1, 2, 3, 4, 5, 7, 255)]
    envs += [consistency(1), consistency(2), consistency(5), consistency(5, short=1), consistency(0), make_env(rng, 6, payload=b"")]
    want = [1, 2, 1, 1, 1, 1, 1, 1, 0, 1, 4, 0, 0, 0]
    blob = np.frombuffer(b"".join(envs) + b"\0", dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(e) for e in envs]))).astype(np.uint64)
    for i, (e, w) in enumerate(zip(envs, want)):
        one = np.frombuffer(e + b"\0", dtype=np.uint8)
        assert w == (2 if e[1] == 1 else ref_jobs(e) if e[1] == 6 else 1)
        assert lib.emul_ve_weight(P(blob), P(off), len(envs), i) == w == lib.emul_ve_scheme_weight(e[1], P(one), len(e)), i
    # what only the packed form can meet: an envelope too short to hold a scheme byte weighs 1, whatever lies behind it
    two = np.frombuffer(bytes([2]) + envs[1], dtype=np.uint8)
    assert lib.emul_ve_weight(P(two), P(np.array([0, 1, len(two)], dtype=np.uint64)), 2, 0) == 1
    assert lib.emul_ve_weight(P(two), P(np.array([0, 1, len(two)], dtype=np.uint64)), 2, 1) == 2


# ---- the copy
GUARD = 64


@pytest.mark.parametrize("dst_align", (0, 1, 2, 3))
def test_copy_is_byte_exact_at_every_alignment(lib, dst_align):
    rng = np.random.default_rng(11 + dst_align)
    for length in list(range(71)) + [298, 762, 814, 1478, 3527]:
        for src_align in range(16):
            for before in (0, 3):                                  # the envelope first in the blob, or behind three bytes of another
                store = np.full(GUARD + 16 + before + length + GUARD + 16, 0xC3, dtype=np.uint8)
                s0 = GUARD + (src_align - (store.ctypes.data + GUARD + before)) % 16          # blob start: envelope at address = src_align (mod 16)
                store[s0:s0 + before + length] = rng.integers(0, 256, before + length, dtype=np.uint8)
                src = store[s0 + before:s0 + before + length].copy()
                snapshot = store.copy()
                out = np.full(GUARD + 4 + length + GUARD, 0x3C, dtype=np.uint8)
                d0 = GUARD + (dst_align - (out.ctypes.data + GUARD)) % 4
                base = store.ctypes.data + s0
                lib.emul_ve_copy(out.ctypes.data + d0, base + before, length, base, base + before + length, 64)
                assert (out[d0:d0 + length] == src).all(), (length, src_align, before)
                assert (out[:d0] == 0x3C).all() and (out[d0 + length:] == 0x3C).all(), (length, src_align, before)          # nothing written around the row
                assert (store == snapshot).all()                                                                         # the blob and what surrounds it are untouched


def test_copy_with_fewer_lanes_than_dwords(lib):
    rng = np.random.default_rng(12)
    src = rng.integers(0, 256, 3527 + 5, dtype=np.uint8)
    for lanes in (1, 7, 64):
        out = np.full(3527 + 8, 0x3C, dtype=np.uint8)
        lib.emul_ve_copy(out.ctypes.data + 1, src.ctypes.data + 5, 3527, src.ctypes.data, src.ctypes.data + len(src), lanes)
        assert (out[1:3528] == src[5:]).all() and out[0] == 0x3C and (out[3528:] == 0x3C).all()


# ---- the plan
def plan(L, rec):
    n = len(rec)
    op_row = np.full(n, 12345, dtype=np.uint32)
    out = np.zeros(31, dtype=np.uint64)
    rc = L.emul_ve_plan(n, P(rec), P(op_row), P(out))
    o = [int(x) for x in out]
    return rc, op_row, {"rows": o[0:7], "row0": o[7:14], "stride": o[14:21], "base": o[21:28], "total_rows": o[28], "live": o[29], "bytes": o[30]}


def test_row_plan_order_alignment_and_stride_caps(lib):
    rng = np.random.default_rng(13)
    n = 1000
    rec = np.zeros(n, dtype=REC)
    rec["scheme"] = rng.integers(0, 7, n)
    rec["len"] = rng.integers(10, 3000, n)
    rc, op_row, p = plan(lib, rec)
    assert rc == 0
    next_row, next_byte = 0, 0
    for k in range(1, 7):
        idx = np.nonzero(rec["scheme"] == k)[0]
        assert p["rows"][k] == len(idx) > 0
        assert p["row0"][k] % 64 == 0 and p["base"][k] % 256 == 0
        assert p["row0"][k] >= next_row and p["base"][k] >= next_byte                                  # the schemes' rows do not overlap
        assert p["stride"][k] == max(16, int(rec["len"][idx].max()))
        assert (op_row[idx] == p["row0"][k] + np.arange(len(idx))).all()                                # envelope order within a scheme
        next_row, next_byte = p["row0"][k] + len(idx), p["base"][k] + p["stride"][k] * len(idx)
    assert (op_row[rec["scheme"] == 0] == NO_ROW).all()
    assert p["total_rows"] >= next_row and p["total_rows"] % 64 == 0 and p["bytes"] >= next_byte and p["live"] == int((rec["scheme"] != 0).sum())
    # the caps: a longer envelope keeps its row and its recorded length (its verifier rejects it); a short list gets the 16-byte floor
    for k in range(1, 7):
        for longest, want in ((CAPS[k] - 1, CAPS[k] - 1), (CAPS[k], CAPS[k]), (CAPS[k] + 1, CAPS[k]), (10, 16)):
            r = np.zeros(3, dtype=REC)
            r["scheme"] = (k, 0, k); r["len"] = (12, 999999, longest)
            rc, op_row, p = plan(lib, r)
            assert rc == 0 and p["stride"][k] == want and list(op_row) == [0, NO_ROW, 1] and p["rows"][k] == 2 and p["bytes"] == (2 * want + 255) // 256 * 256
    rc, op_row, p = plan(lib, np.zeros(5, dtype=REC))
    assert rc == 0 and p["live"] == 0 and p["total_rows"] == 0 and p["bytes"] == 0 and (op_row == NO_ROW).all()


def test_row_plan_refuses_more_than_4_gib_per_scheme(lib):
    assert lib.emul_ve_plan_uniform(1 << 20, 1, 4096) == 0              # exactly 4 GiB
    assert lib.emul_ve_plan_uniform((1 << 20) + 1, 1, 4096) == 1        # the scheme that does not fit
    assert lib.emul_ve_plan_uniform((1 << 20) + 1, 3, 9000) == 3        # (capped stride)
    assert lib.emul_ve_plan_uniform(1 << 19, 5, 8192) == 0 and lib.emul_ve_plan_uniform((1 << 19) + 1, 5, 8192) == 5
    assert lib.emul_ve_plan_uniform(4097, 6, 1 << 20) == 6 and lib.emul_ve_plan_uniform(4096, 6, 1 << 20) == 0
    assert lib.emul_ve_plan_uniform(1 << 22, 2, 298) == 0              # the largest call of equality envelopes fits


# ---- classification -> plan -> rows -> verdicts back
def test_pipeline_rows_parameters_and_scatter(lib):
    rng = np.random.default_rng(14)
    envs = []
    for i in range(60):
        envs.append(random_env(rng))
    envs += [make_env(rng, 1, payload=(5).to_bytes(8, "little") + (9).to_bytes(8, "little") + bytes(5000)),          # beyond the 4096 cap
             make_env(rng, 2, payload=bytes(256)), make_env(rng, 5, payload=(77).to_bytes(8, "little") + bytes(100))]
    n = len(envs)
    blob = np.frombuffer(b"".join(envs) + b"\0", dtype=np.uint8)
    off = np.concatenate(([0], np.cumsum([len(e) for e in envs]))).astype(np.uint64)
    rec = classify(lib, envs)
    rc, op_row, p = plan(lib, rec)
    assert rc == 0 and p["stride"][1] == 4096
    accept = rng.integers(0, 2, n, dtype=np.uint8)
    rows = np.full(p["bytes"] + GUARD, 0xEE, dtype=np.uint8)
    R = p["total_rows"]
    row_len, row_p0, row_p1 = np.full(R, 0xABCD, dtype=np.uint32), np.zeros(R, dtype=np.uint64), np.zeros(R, dtype=np.uint64)
    ok = np.full(n, 7, dtype=np.uint8)
    assert lib.emul_ve_pipeline(n, P(blob), P(off), None, P(accept), P(rows), P(row_len), P(row_p0), P(row_p1), P(ok)) == 0
    assert (rows[p["bytes"]:] == 0xEE).all()
    written = np.zeros(p["bytes"], dtype=bool)
    for i, e in enumerate(envs):
        s = int(rec["scheme"][i])
        assert ok[i] == (accept[i] if s else 0)
        if not s:
            continue
        g = int(op_row[i]); at = p["base"][s] + p["stride"][s] * (g - p["row0"][s]); take = min(len(e), p["stride"][s])
        assert rows[at:at + take].tobytes() == e[:take]
        written[at:at + take] = True
        assert row_len[g] == len(e) and row_p0[g] == rec["p0"][i] and row_p1[g] == rec["p1"][i]
    assert (rows[:p["bytes"]][~written] == 0xEE).all()          # nothing behind an envelope or between the schemes' rows is touched
