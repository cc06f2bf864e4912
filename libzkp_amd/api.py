"""Host-side mirror of the reference's operator interface for the hot path.

Same names, argument meaning and error behaviour as the reference:
  prove_range                 /root/reference/src/proof/range_proof.rs:10-27   (validation.rs:5-18 messages)
  create_proof_batch .. process_batch, get_batch_status, clear_batch
                              /root/reference/src/advanced/batch.rs:35-175,262-283
  benchmark_proof_generation  /root/reference/src/advanced/mod.rs:83-172,204-215
Error mapping follows /root/reference/src/utils/error_handling.rs:39-50: InvalidInput -> ValueError(msg);
everything else -> RuntimeError("<Display prefix>: msg").
"""
import ctypes
import secrets
import threading
import time

import numpy as np

from . import _native, perf, batch_store

U64_MAX = 2**64 - 1


class ZkpBackendError(RuntimeError):
    pass


def _check_u64(name, x):
    if not isinstance(x, (int, np.integer)) or isinstance(x, bool) or x < 0 or x > U64_MAX:
        raise OverflowError("%s out of range for u64" % name)
    return int(x)


def _u64_array(name, xs):
    """u64 column of a batch.  Unsigned numpy arrays are taken as they are; anything else is checked element by element."""
    if isinstance(xs, np.ndarray) and xs.dtype.kind == "u" and xs.ndim == 1:
        return np.ascontiguousarray(xs, dtype=np.uint64)
    return np.array([_check_u64(name, x) for x in xs], dtype=np.uint64)


def _rows(blobs, cap=4096):
    """Byte strings of a batch as rows of one buffer (stride = the longest, at most `cap`: longer ones are rejected by the
    library through their recorded length).  Equal lengths -- the usual case -- are packed without a Python loop."""
    n = len(blobs)
    lens = np.fromiter((len(b) for b in blobs), dtype=np.uint32, count=n)
    stride = int(min(cap, max(16, int(lens.max()))))
    if int(lens.min()) == int(lens.max()) == stride:
        return np.frombuffer(b"".join(blobs), dtype=np.uint8).reshape(n, stride).copy(), lens, stride
    buf = np.zeros((n, stride), dtype=np.uint8)
    for i, b in enumerate(blobs):
        buf[i, : min(len(b), stride)] = np.frombuffer(b[:stride], dtype=np.uint8)
    return buf, lens, stride


def validate_range_params(value, mn, mx):
    """validation.rs:5-18."""
    if mn > mx:
        raise ValueError("min cannot be greater than max")
    if value < mn or value > mx:
        raise ValueError("value %d is not in range [%d, %d]" % (value, mn, mx))


def _P(a):
    return a.ctypes.data_as(ctypes.c_void_p)


BIT_WIDTHS = (8, 16, 32, 64)          # RangeProof::prove_single's valid bit sizes


def max_u64_for_bit_width(n_bits):
    """bulletproofs.rs:94-100"""
    return 2**64 - 1 if n_bits >= 64 else (1 << n_bits) - 1


def _check_bits(n_bits, what):
    if n_bits not in BIT_WIDTHS:         # upstream: ProofError::InvalidBitsize -> "... proof generation failed"
        raise ZkpBackendError("Backend error: %s proof generation failed (n_bits must be 8, 16, 32 or 64)" % what)
    return int(n_bits)


def prove_range_batch(values, mins, maxs, seeds=None, device=None, n_bits=64):
    """Batched prove_range / prove_range_with_bits: returns a list of proof bytes (one envelope per op; 1478 bytes for
    n_bits = 64, 128 fewer per halving of the width).

    Raises ValueError (reference message) if any op is invalid -- like process_batch, one failure fails the call.
    `seeds` (n x 32 bytes) pins the randomness tape; None draws fresh OS randomness like the reference.
    """
    n = len(values)
    n_bits = _check_bits(n_bits, "min range")
    v, mn, mx = _u64_array("value", values), _u64_array("min", mins), _u64_array("max", maxs)
    if not (len(mn) == n and len(mx) == n):
        raise ValueError("values, mins, maxs must have equal length")
    cap = np.uint64(max_u64_for_bit_width(n_bits))
    bad = (mn > mx) | (v < mn) | (v > mx)
    if bad.any():
        i = int(np.argmax(bad))
        validate_range_params(int(v[i]), int(mn[i]), int(mx[i]))                  # raises the reference's message
    if n and (((v - mn) > cap) | ((mx - v) > cap)).any():                          # bulletproofs.rs:121-129
        raise ZkpBackendError("Backend error: range width exceeds %d-bit capacity; use n_bits=64" % n_bits)
    if n == 0:
        return []
    L = _native.lib()
    if device is not None:
        _native.check(L.zkp_hip_init(int(device)), "zkp_hip_init")
    sp = None
    if seeds is not None:
        s = np.frombuffer(bytes(seeds), dtype=np.uint8) if not isinstance(seeds, np.ndarray) else seeds.astype(np.uint8).ravel()
        if s.size != 32 * n:
            raise ValueError("seeds must hold 32 bytes per op")
        s = np.ascontiguousarray(s)
        sp = _P(s)
    out = np.zeros((n, _native.RANGE_PROOF_BYTES), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_prove_range_batch(n, _P(v), _P(mn), _P(mx), n_bits, sp, _P(out), _native.RANGE_PROOF_BYTES, _P(lens), _P(st))
    if rc < 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    if rc > 0:
        bad = int(np.nonzero(st)[0][0])
        raise ZkpBackendError("Backend error: range proof generation failed for op %d (status %d)" % (bad, int(st[bad])))
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def _seed_ptr(seeds, n):
    if seeds is None:
        return None, None
    s = np.frombuffer(bytes(seeds), dtype=np.uint8) if not isinstance(seeds, np.ndarray) else seeds.astype(np.uint8).ravel()
    if s.size != 32 * n:
        raise ValueError("seeds must hold 32 bytes per op")
    s = np.ascontiguousarray(s)
    return s, _P(s)


def _raise_backend(rc, st, what):
    if rc < 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    if rc > 0:
        bad = int(np.nonzero(st)[0][0])
        raise ZkpBackendError("Backend error: %s failed for op %d (status %d)" % (what, bad, int(st[bad])))


def validate_threshold_params(values, threshold):
    """validation.rs:30-47."""
    if len(values) == 0:
        raise ValueError("values cannot be empty")
    total = sum(values)
    if total > U64_MAX:
        raise ValueError("integer overflow in sum calculation")
    if total < threshold:
        raise ValueError("sum %d is less than threshold %d" % (total, threshold))
    return total


def validate_consistency_params(data):
    """validation.rs:75-88."""
    if len(data) == 0:
        raise ValueError("data cannot be empty")
    if any(a > b for a, b in zip(data, data[1:])):
        raise ValueError("data is not monotonic non-decreasing")


def prove_threshold_batch(value_lists, thresholds, seeds=None, n_bits=64):
    """Batched prove_threshold / prove_threshold_with_bits (threshold_proof.rs:12-32): one envelope per op (762 bytes for
    n_bits = 64, 64 fewer per halving of the width)."""
    n = len(value_lists)
    n_bits = _check_bits(n_bits, "threshold range")
    lists = [[_check_u64("value", x) for x in vl] for vl in value_lists]
    thr = [_check_u64("threshold", t) for t in thresholds]
    for vl, t in zip(lists, thr):
        validate_threshold_params(vl, t)
        if sum(vl) - t > max_u64_for_bit_width(n_bits):                           # bulletproofs.rs:330-336
            raise ZkpBackendError("Backend error: sum - threshold exceeds %d-bit capacity; use n_bits=64" % n_bits)
    if n == 0:
        return []
    flat = np.array([x for vl in lists for x in vl], dtype=np.uint64)
    counts = np.array([len(vl) for vl in lists], dtype=np.uint32)
    th = np.array(thr, dtype=np.uint64)
    keep, sp = _seed_ptr(seeds, n)
    stride = 762
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = _native.lib().zkp_hip_prove_threshold_batch(n, _P(flat), _P(counts), _P(th), n_bits, sp, _P(out), stride, _P(lens), _P(st))
    _raise_backend(rc, st, "threshold proof generation")
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def prove_consistency_batch(data_lists, seeds=None):
    """Batched prove_consistency (consistency_proof.rs:12-22)."""
    n = len(data_lists)
    lists = [[_check_u64("value", x) for x in dl] for dl in data_lists]
    for dl in lists:
        validate_consistency_params(dl)
    if n == 0:
        return []
    L = _native.lib()
    flat = np.array([x for dl in lists for x in dl], dtype=np.uint64)
    counts = np.array([len(dl) for dl in lists], dtype=np.uint32)
    stride = max(int(L.zkp_hip_consistency_proof_bytes(int(c))) for c in counts)
    keep, sp = _seed_ptr(seeds, n)
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_prove_consistency_batch(n, _P(flat), _P(counts), sp, _P(out), stride, _P(lens), _P(st))
    _raise_backend(rc, st, "consistency proof generation")
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def prove_threshold(values, threshold):
    return prove_threshold_batch([list(values)], [threshold])[0]


def prove_threshold_with_bits(values, threshold, n_bits):
    """threshold_proof.rs:17-32: sum(values) - threshold must fit in n_bits (8, 16, 32 or 64)."""
    return prove_threshold_batch([list(values)], [threshold], n_bits=n_bits)[0]


def prove_consistency(data):
    return prove_consistency_batch([list(data)])[0]


# ---------------------------------------------------------------- Groth16 (equality / membership), snark.rs
MAX_SET_SIZE = 64
_key_dir_override = None
_keys_loaded = {}
_reinstall = {}            # kind -> key bytes to load again on first use after shutdown()
_key_blobs = {}            # kind -> key bytes of the loaded key (multi-GPU: rank 0's proving key is broadcast, sharding.py)
_verifier_only = set()     # kinds whose loaded key is a verifying key alone (`{prefix}_vk.bin`): they verify, they cannot prove
_KEY_PREFIX = {0: "equality_mimc", 1: "membership_mimc"}          # snark.rs:306,327
_snark_lock = threading.Lock()


def set_snark_key_dir(path):
    """snark.rs:141-170 (ConfigError -> TypeError, error_handling.rs:43-45).  Must precede the first SNARK proof."""
    global _key_dir_override
    if not path:
        raise TypeError("SNARK key directory cannot be empty")
    with _snark_lock:
        if _keys_loaded:
            raise TypeError("SNARK setup is already initialized; set LIBZKP_SNARK_KEY_DIR before first proof")
        if _key_dir_override is not None and _key_dir_override != path:
            raise TypeError("SNARK key directory already set to %s; new value %s rejected" % (_key_dir_override, path))
        _key_dir_override = path
    return True


def is_snark_setup_initialized():
    return bool(_keys_loaded)


def _vk_prefix_len(blob):
    """Bytes of the VerifyingKey that leads an ark-serialize uncompressed ProvingKey<Bn254> (and is the whole of a `_vk.bin`):
    alpha_g1 | beta_g2, gamma_g2, delta_g2 | u64 n | gamma_abc_g1[n]."""
    return 64 + 3 * 128 + 8 + 64 * int.from_bytes(blob[448:456], "little")


def _ensure_key(kind, verifier=False):
    """load_or_generate_setup (snark.rs:122-139): loads `{dir}/{prefix}_pk.bin` (ark-serialize uncompressed
    ProvingKey<Bn254>, the reference's own key-file format) or runs a fresh setup on the GPU and persists it.
    verifier=True (the verify_* paths): a key directory that holds `{prefix}_vk.bin` but no `{prefix}_pk.bin` is a verifier's
    deployment -- that verifying key is loaded alone (snark.rs:377-401 verifies with the VerifyingKey only) instead of running a
    fresh setup under which no foreign envelope could verify.  A prove call with such a directory, before or after, needs the proving
    key file: it raises instead of generating a second setup over the directory's `_vk.bin`."""
    import os
    with _snark_lock:
        if kind in _keys_loaded and (verifier or kind not in _verifier_only):
            return
        d = _key_dir_override or os.environ.get("LIBZKP_SNARK_KEY_DIR")
        L = _native.lib()
        path = os.path.join(d, _KEY_PREFIX[kind] + "_pk.bin") if d else None
        vk_path = os.path.join(d, _KEY_PREFIX[kind] + "_vk.bin") if d else None
        # a prove call where this process holds (or held before shutdown()) a verifying key alone: the proving key file, never a second setup
        upgrade = not verifier and kind in _verifier_only and (kind in _keys_loaded or kind in _reinstall)
        if upgrade and not (path and os.path.exists(path)):
            raise ZkpBackendError("Configuration error: only the verifying key of the %s circuit is loaded and there is no proving key (%s) to prove with"
                                  % (_KEY_PREFIX[kind], path or _KEY_PREFIX[kind] + "_pk.bin: no key directory set"))
        if kind in _reinstall and not upgrade:                      # after shutdown(): the process keeps ONE setup per circuit
            blob = _reinstall.pop(kind)
            if L.zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
                raise ZkpBackendError("Configuration error: %s" % _native.last_error())
            _key_blobs[kind] = blob
            path = "<reinstalled verifying key>" if kind in _verifier_only else path or "<reinstalled>"
        elif path and os.path.exists(path):
            blob = open(path, "rb").read()
            if L.zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
                raise ZkpBackendError("Configuration error: %s" % _native.last_error())
            _key_blobs[kind] = blob
            _verifier_only.discard(kind)
            _reinstall.pop(kind, None)
        elif verifier and vk_path and os.path.exists(vk_path):
            blob = open(vk_path, "rb").read()
            if L.zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
                raise ZkpBackendError("Configuration error: %s" % _native.last_error())
            _key_blobs[kind] = blob
            _verifier_only.add(kind)
            path = vk_path
        elif vk_path and os.path.exists(vk_path):
            # a prove call in a directory that holds the verifying key but not the proving key: a fresh setup here would overwrite that
            # `_vk.bin` with the key of another setup, under which nothing proved elsewhere verifies
            raise ZkpBackendError("Configuration error: %s holds the verifying key of the %s circuit but no proving key (%s) to prove with; "
                                  "a fresh setup would replace that verifying key" % (d, _KEY_PREFIX[kind], path))
        else:
            # load_or_generate_setup (snark.rs:122-139): fresh trusted setup (OS randomness), persisted if a key dir is set
            pk_len, vk_len = ctypes.c_uint64(), ctypes.c_uint64()
            cap_pk, cap_vk = 1 << 20, 1 << 16
            pk, vk = ctypes.create_string_buffer(cap_pk), ctypes.create_string_buffer(cap_vk)
            if L.zkp_hip_groth16_generate_key(kind, None, pk, cap_pk, ctypes.byref(pk_len), vk, cap_vk, ctypes.byref(vk_len)) != 0:
                raise ZkpBackendError("Proof generation failed: setup failed: %s" % _native.last_error())
            if d:
                try:
                    os.makedirs(d, exist_ok=True)
                    open(path, "wb").write(pk.raw[: pk_len.value])
                    open(os.path.join(d, _KEY_PREFIX[kind] + "_vk.bin"), "wb").write(vk.raw[: vk_len.value])
                except OSError:
                    pass                                              # the reference ignores persist errors too (snark.rs:131-133)
            _key_blobs[kind] = pk.raw[: pk_len.value]
            _verifier_only.discard(kind)
            path = path or "<generated in memory>"
        _keys_loaded[kind] = path


def shutdown():
    """Release every device resource of the library (tables, keys, workspaces, streams).  The next call initialises again;
    the Groth16 keys of this process are kept on the host and reinstalled on first use, so proofs made before still verify."""
    with _snark_lock:
        _native.lib().zkp_hip_shutdown()
        _reinstall.update({k: _key_blobs[k] for k in _keys_loaded if k in _key_blobs})
        _keys_loaded.clear()


def generator_table_info():
    """The Bulletproofs generator tables of the calling thread's shard (zkp_hip_groth16_key_info kind ZKP_HIP_TABLES_BP_GENERATORS):
    {"radix": "2^w", "table_bytes": n}, or {"radix": None, "table_bytes": 0} while ZKP_HIP_ED_TABLES=lazy has not built them yet.
    Initialises the shard (device 0) on first use, like the prove calls."""
    L = _native.lib()
    wbits, uneven, nbytes = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint64()
    if L.zkp_hip_groth16_key_info(_native.TABLES_BP_GENERATORS, ctypes.byref(wbits), ctypes.byref(uneven), ctypes.byref(nbytes)) != 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    return {"radix": "2^%d" % wbits.value if wbits.value else None, "table_bytes": int(nbytes.value)}


def export_proving_key(kind):
    """The loaded (or freshly generated) proving key of a circuit (0 equality, 1 membership) in ark-serialize form."""
    _ensure_key(kind)
    return _key_blobs[kind]


def export_verifying_key(kind):
    """The verifying key of a circuit in ark-serialize uncompressed form (the content of `{prefix}_vk.bin`): the installed verifying
    key, or the VerifyingKey that leads the loaded (or freshly generated) proving key."""
    _ensure_key(kind, verifier=True)
    blob = _key_blobs[kind]
    return blob[:_vk_prefix_len(blob)]


def install_proving_key(kind, blob):
    """Make `blob` THE proving key of this process (every rank of a multi-GPU job must prove under one setup)."""
    with _snark_lock:
        if _native.lib().zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
            raise ZkpBackendError("Configuration error: %s" % _native.last_error())
        _key_blobs[kind] = bytes(blob)
        _verifier_only.discard(kind)
        _keys_loaded[kind] = "<installed>"


def install_verifying_key(kind, blob):
    """Make `blob` (ark-serialize uncompressed VerifyingKey<Bn254>, a `{prefix}_vk.bin`) the key of this process for verification only:
    no circuit, no MSM tables -- what a verifier service holds.  Replaces a proving key loaded earlier (its tables are freed)."""
    blob = bytes(blob)
    if len(blob) < 456 or len(blob) != _vk_prefix_len(blob):
        raise ZkpBackendError("Configuration error: not a verifying key (a proving key is installed with install_proving_key)")
    with _snark_lock:
        if _native.lib().zkp_hip_groth16_load_key(kind, blob, len(blob)) != 0:
            raise ZkpBackendError("Configuration error: %s" % _native.last_error())
        _key_blobs[kind] = blob
        _verifier_only.add(kind)
        _keys_loaded[kind] = "<installed verifying key>"


_KEYCHECK_VERDICTS = ("sound", "format", "subgroup", "twins", "tables")
_KEYCHECK_TABLES = ("g1", "g2", "vk")


def check_key(kind, blob=None, twins=True, tables=None):
    """The Groth16 key check on the GPU (zkpkeycheck_key, include/libzkp_hip_keycheck.h) of `blob` as a key of circuit `kind` (0 equality,
    1 membership), either format.  blob=None: this process's key (loaded or generated first, as a verify call would).  Always: format,
    shape and the G2 points' subgroup membership, what the loader enforces.  twins=True: a proving key's b_g1_query / b_g2_query, beta and
    delta pairs share their discrete logarithms (a verifying key has none: the two verdicts are None).  tables: every entry of the window
    tables resident on this shard against the key's points; None means "yes when the blob is the loaded key".
    Returns the report as a dict; "verdict" is "sound" or the first stage that failed ("format", "subgroup", "twins", "tables")."""
    if blob is None:
        _ensure_key(kind, verifier=True)
        blob = _key_blobs[kind]
    blob = bytes(blob)
    if tables is None:
        tables = kind in _keys_loaded and _key_blobs.get(kind) == blob
    what = _native.KEYCHECK_POINTS | (_native.KEYCHECK_TWINS if twins else 0) | (_native.KEYCHECK_TABLES if tables else 0)
    rep = _native.KeyCheckReport()
    if _native.lib().zkpkeycheck_key(kind, blob, len(blob), what, ctypes.byref(rep)) != 0:
        raise ZkpBackendError("Key check failed: %s" % _native.last_error())
    tri = lambda v: None if v < 0 else bool(v)      # noqa: E731
    first = None if rep.table_first_which < 0 else {"table": _KEYCHECK_TABLES[rep.table_first_which], "slot": int(rep.table_first_slot),
                                                    "window": int(rep.table_first_window), "entry": int(rep.table_first_entry)}
    return {"format": ("proving_key", "verifying_key", None)[rep.format], "verdict": _KEYCHECK_VERDICTS[rep.verdict], "sound": rep.verdict == 0,
            "stages_run": [n for n, bit in (("points", 1), ("twins", 2), ("tables", 4)) if rep.stages_run & bit],
            "g2_checked": int(rep.g2_checked), "g2_outside": int(rep.g2_outside), "g2_first_outside": None if rep.g2_first_outside < 0 else int(rep.g2_first_outside),
            "twins_checked": int(rep.twins_checked), "twin_inf_mismatches": int(rep.twin_inf_mismatches),
            "twins_query_ok": tri(rep.twins_query_ok), "twins_beta_delta_ok": tri(rep.twins_beta_delta_ok),
            "table_entries": {"g1": int(rep.table_entries_g1), "g2": int(rep.table_entries_g2), "vk": int(rep.table_entries_vk)},
            "table_bad_pairs": int(rep.table_bad_pairs), "table_first_bad": first,
            "ms": {"points": float(rep.ms_points), "twins": float(rep.ms_twins), "tables": float(rep.ms_tables)},
            "message": rep.message.decode("utf-8", "replace")}


def _read_counters(symbol, lead, keys, reset):
    """One family of the library's host-side counters through its export `symbol`: the leading arguments `lead` (the id, for the families of
    zkp_hip_profile_read_kernel), then a double and one uint64 per key as outs, `reset` last.  {key: count, ..., "ms": host milliseconds}."""
    ms, counts = ctypes.c_double(), [ctypes.c_uint64() for _ in keys]
    _native.check(getattr(_native.lib(), symbol)(*lead, ctypes.byref(ms), *[ctypes.byref(c) for c in counts], 1 if reset else 0), symbol)
    out = {k: int(c.value) for k, c in zip(keys, counts)}
    out["ms"] = float(ms.value)
    return out


def key_check_counters(reset=True):
    """What the key loader's checks and check_key did, summed over the shards since the last reset (zkpkeycheck_counters,
    include/libzkp_hip_keycheck.h; always counted): {"loads_checked": key loads whose freshly built tables were self-checked,
    "entries_checked": table entries checked, "refused": keys refused at load or judged unsound by check_key, "ms": host time of the table
    checks}.  reset=True zeroes the counters."""
    return _read_counters("zkpkeycheck_counters", (), ("loads_checked", "entries_checked", "refused"), reset)


def snark_commit_value_batch(values):
    v = np.array([_check_u64("value", x) for x in values], dtype=np.uint64)
    if len(v) == 0:
        return []
    out = np.zeros((len(v), 32), dtype=np.uint8)
    rc = _native.lib().zkp_hip_snark_commit_value_batch(len(v), _P(v), _P(out))
    if rc != 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    return [out[i].tobytes() for i in range(len(v))]


def snark_commit_value(value):
    """python_api.rs:32 -> commitment.rs:14-16 (MiMC-5 over BN254 Fr, 32 bytes LE)."""
    return snark_commit_value_batch([value])[0]


def validate_membership_params(value, the_set):
    """validation.rs:50-63, 91-100."""
    if len(the_set) == 0:
        raise ValueError("set cannot be empty")
    if value not in the_set:
        raise ValueError("value %d is not in the provided set" % value)
    if len(the_set) > MAX_SET_SIZE:
        raise ValueError("set size %d exceeds maximum allowed size %d" % (len(the_set), MAX_SET_SIZE))


def prove_equality_batch(vals1, vals2, seeds=None):
    """Batched prove_equality (equality_proof.rs:10-32): one 298-byte envelope per op."""
    n = len(vals1)
    a = np.array([_check_u64("val1", x) for x in vals1], dtype=np.uint64)
    b = np.array([_check_u64("val2", x) for x in vals2], dtype=np.uint64)
    if len(b) != n:
        raise ValueError("vals1, vals2 must have equal length")
    if (a != b).any():
        raise ValueError("values are not equal")                     # validation.rs:21-27
    if n == 0:
        return []
    _ensure_key(0)
    keep, sp = _seed_ptr(seeds, n)
    out = np.zeros((n, 298), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = _native.lib().zkp_hip_prove_equality_batch(n, _P(a), _P(b), sp, _P(out), 298, _P(lens), _P(st))
    if rc != 0:
        raise ZkpBackendError("Proof generation failed: SNARK proof generation failed%s" % (": " + _native.last_error() if rc < 0 else ""))
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def prove_membership_batch(values, sets, seeds=None):
    """Batched prove_membership (set_membership.rs:12-38)."""
    n = len(values)
    vs = [_check_u64("value", x) for x in values]
    ss = [[_check_u64("set element", x) for x in s] for s in sets]
    for v, s in zip(vs, ss):
        validate_membership_params(v, s)
    if n == 0:
        return []
    _ensure_key(1)
    flat = np.array([x for s in ss for x in s], dtype=np.uint64)
    counts = np.array([len(s) for s in ss], dtype=np.uint32)
    va = np.array(vs, dtype=np.uint64)
    stride = 10 + 4 + 8 * int(counts.max()) + 256 + 32
    keep, sp = _seed_ptr(seeds, n)
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = _native.lib().zkp_hip_prove_membership_batch(n, _P(va), _P(flat), _P(counts), sp, _P(out), stride, _P(lens), _P(st))
    if rc != 0:
        raise ZkpBackendError("Proof generation failed: SNARK membership proof generation failed%s" % (": " + _native.last_error() if rc < 0 else ""))
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def prove_improvement_batch(olds, news):
    """Batched prove_improvement (improvement_proof.rs:10-35): Winterfell-style STARK envelopes (scheme 5); deterministic."""
    n = len(olds)
    o = np.array([_check_u64("old", x) for x in olds], dtype=np.uint64)
    w = np.array([_check_u64("new", x) for x in news], dtype=np.uint64)
    if len(w) != n:
        raise ValueError("olds, news must have equal length")
    if (w <= o).any():
        raise ValueError("new value must be greater than old value")        # validation.rs:63-71
    if n == 0:
        return []
    L = _native.lib()
    stride = int(L.zkp_hip_improvement_max_bytes())
    out = np.zeros((n, stride), dtype=np.uint8)
    lens = np.zeros(n, dtype=np.uint32)
    st = np.zeros(n, dtype=np.int32)
    rc = L.zkp_hip_prove_improvement_batch(n, _P(o), _P(w), _P(out), stride, _P(lens), _P(st))
    if rc != 0:
        raise ZkpBackendError("Proof generation failed: STARK proof generation failed%s" % (": " + _native.last_error() if rc < 0 else ""))
    return [out[i, : lens[i]].tobytes() for i in range(n)]


def prove_improvement(old, new):
    return prove_improvement_batch([old], [new])[0]


def prove_equality(val1, val2):
    return prove_equality_batch([val1], [val2])[0]


def prove_equality_advanced(val1, val2):
    """advanced/mod.rs:193-196: same semantics as prove_equality."""
    return prove_equality(val1, val2)


def prove_membership(value, set):  # noqa: A002
    return prove_membership_batch([value], [list(set)])[0]


def verify_range_batch(proofs, mins, maxs):
    """Batched verify_range (range_proof.rs:28-47): list of bools.  Never raises on malformed proofs (they are False)."""
    n = len(proofs)
    if len(mins) != n or len(maxs) != n:
        raise ValueError("proofs, mins, maxs must have equal length")
    if n == 0:
        return []
    mn, mx = _u64_array("min", mins), _u64_array("max", maxs)
    buf, lens, stride = _rows([bytes(p) for p in proofs])      # a range envelope is 1478 bytes: anything beyond 4096 is rejected outright
    ok = np.zeros(n, dtype=np.uint8)
    rc = _native.lib().zkp_hip_verify_range_batch(n, _P(buf), stride, _P(lens), _P(mn), _P(mx), _P(ok))
    _native.check(rc, "zkp_hip_verify_range_batch")
    return [x == 1 for x in ok]


def verify_threshold_batch(proofs, thresholds):
    """Batched verify_threshold (threshold_proof.rs:34-47): list of bools."""
    n = len(proofs)
    if len(thresholds) != n:
        raise ValueError("proofs, thresholds must have equal length")
    if n == 0:
        return []
    th = _u64_array("threshold", thresholds)
    buf, lens, stride = _rows([bytes(p) for p in proofs])
    ok = np.zeros(n, dtype=np.uint8)
    _native.check(_native.lib().zkp_hip_verify_threshold_batch(n, _P(buf), stride, _P(lens), _P(th), _P(ok)), "zkp_hip_verify_threshold_batch")
    return [x == 1 for x in ok]


def _verify_snark_envelopes(kind, blobs):
    """Groth16 pairing check of equality (kind 0) / membership (kind 1) envelopes under the loaded key; public inputs are the
    envelope's own commitment and embedded set."""
    n = len(blobs)
    if n == 0:
        return []
    _ensure_key(kind, verifier=True)
    buf, lens, stride = _rows(blobs, 4096)
    ok = np.zeros(n, dtype=np.uint8)
    fn = _native.lib().zkp_hip_verify_equality_batch if kind == 0 else _native.lib().zkp_hip_verify_membership_batch
    _native.check(fn(n, _P(buf), stride, _P(lens), _P(ok)), "zkp_hip_verify_%s_batch" % ("equality" if kind == 0 else "membership"))
    return ok.astype(bool).tolist()


def groth16_verify_counters(reset=True):
    """What verify_equality_batch / verify_membership_batch did after batch checks that did not stand, summed over the shards since the last
    reset (zkp_hip_profile_read_kernel id ZKP_HIP_COUNTER_G16_VERIFY; always counted): {"launches": segment checks run by localisation
    passes, "point_adds": envelopes given the per-envelope check after a failed batch check (the suspects, or the whole batch), "ms": host
    wall time from the failed checks' verdicts to the calls' returns}.  reset=True zeroes the counters."""
    return _read_counters("zkp_hip_profile_read_kernel", (_native.COUNTER_G16_VERIFY,), ("launches", "point_adds"), reset)


def bp_verify_counters(reset=True):
    """What verify_range_batch / verify_threshold_batch / verify_consistency_batch and everything built on them did after batch checks that
    did not stand, summed over the shards since the last reset (zkp_hip_bp_localise_counters, include/libzkp_hip_bp_localise.h; always
    counted): {"failed_checks": batch checks (calls or slices) that did not stand, "segment_checks": segments checked by localisation
    passes, "jobs_again": jobs given the per-job pass after a failed check (the suspects, or the whole batch), "ms": host wall time from the
    failed checks' verdicts to the calls' returns}.  reset=True zeroes the counters."""
    return _read_counters("zkp_hip_bp_localise_counters", (), ("failed_checks", "segment_checks", "jobs_again"), reset)


def batch_self_check_counters(reset=True):
    """What the self-check of flagged batches (process_ops / process_batch with self_check=True; ZKP_HIP_OP_SELF_CHECK) did, summed over the
    shards since the last reset (zkp_hip_profile_read_kernel id ZKP_HIP_COUNTER_BATCH_SELF_CHECK; always counted): {"launches": ops whose
    envelope went through its verifier, "point_adds": ops the self-check refused, "ms": host wall time from the end of proving to the end of
    verification}.  reset=True zeroes the counters."""
    return _read_counters("zkp_hip_profile_read_kernel", (_native.COUNTER_BATCH_SELF_CHECK,), ("launches", "point_adds"), reset)


def verify_fanout_counters(reset=True):
    """What the verify_*_batch calls that were spread over several registered shards did, summed over the shards since the last reset
    (zkp_hip_profile_read_kernel id ZKP_HIP_COUNTER_VERIFY_FANOUT; always counted): {"launches": slices run by fanned-out calls,
    "point_adds": envelopes in those slices, "ms": host wall time of the fanned-out calls}.  A call that stayed on one shard -- one shard
    registered, ZKP_HIP_VERIFY_SHARDS=0, a thread that selected a shard, less than two minimum slices of work -- counts nothing.
    reset=True zeroes the counters."""
    return _read_counters("zkp_hip_profile_read_kernel", (_native.COUNTER_VERIFY_FANOUT,), ("launches", "point_adds"), reset)


def verify_mixed_counters(reset=True):
    """What the mixed verifier (verify_envelopes, and through it verify_proofs_parallel / verify_composite_proof) did, summed over the shards
    since the last reset (zkp_hip_profile_read_kernel id ZKP_HIP_COUNTER_VERIFY_MIXED; always counted): {"launches": scheme passes run,
    "point_adds": envelopes that got a row (everything the classification did not reject), "ms": host wall time of the calls}.
    reset=True zeroes the counters."""
    return _read_counters("zkp_hip_profile_read_kernel", (_native.COUNTER_VERIFY_MIXED,), ("launches", "point_adds"), reset)


def verify_envelopes(envelopes, expect=None):
    """verify_single_proof (performance.rs:270-293) for a list of envelopes of any scheme in ONE library call (zkp_hip_verify_envelopes,
    include/libzkp_hip_verify.h): list of bools in the caller's order.  expect: None, or per envelope 0 ("any scheme") or the scheme id
    the envelope must carry.  Every parameter (bounds, threshold, old value, embedded set) is the envelope's own.  Never raises on
    malformed envelopes (they are False)."""
    blobs = [bytes(e) for e in envelopes]
    n = len(blobs)
    if expect is not None and len(expect) != n:
        raise ValueError("envelopes, expect must have equal length")
    if n == 0:
        return []
    for kind, scheme in ((0, 2), (1, 4)):              # a Groth16 key only for the circuits whose scheme byte occurs
        if any(len(b) > 1 and b[1] == scheme for b in blobs):
            _ensure_key(kind, verifier=True)
    blob = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.uint64, count=n), out=off[1:])
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    ex = None if expect is None else np.ascontiguousarray(np.asarray(expect, dtype=np.uint8))
    ok = np.zeros(n, dtype=np.uint8)
    _native.check(_native.lib().zkp_hip_verify_envelopes(n, _P(blob), _P(off), None if ex is None else _P(ex), _P(ok)), "zkp_hip_verify_envelopes")
    return (ok == 1).tolist()


def statement_ops(ops):
    """The zkp_hip_op array and the value lists zkp_stmt_verify reads (include/libzkp_hip_statements.h) for `ops`, the tuples process_ops
    takes plus ("equality_commitment", bytes32): (ctypes array, list of list values, set of op kinds that occur).  Only what a statement
    consists of is filled in: a range op's value, a threshold op's values and a consistency op's data are no part of theirs."""
    code = {"range": _native.OP_RANGE, "equality": _native.OP_EQUALITY, "equality_commitment": _native.OP_EQUALITY, "threshold": _native.OP_THRESHOLD,
            "membership": _native.OP_MEMBERSHIP, "improvement": _native.OP_IMPROVEMENT, "consistency": _native.OP_CONSISTENCY}
    arr = (_native.Op * max(len(ops), 1))()
    lists = []
    kinds = set()
    for i, o in enumerate(ops):
        k = o[0]
        e = arr[i]
        e.kind = code[k]
        kinds.add(e.kind)
        if k == "range":
            e.a, e.b, e.c = (_check_u64("range op", x) for x in o[1:4])
        elif k in ("equality", "improvement"):
            e.a, e.b = (_check_u64(k + " op", x) for x in o[1:3])
        elif k == "equality_commitment":
            c = bytes(o[1])
            if len(c) != 32:
                raise ValueError("an expected commitment has 32 bytes")
            e.count, e.list_off = 4, len(lists)
            lists.extend(int.from_bytes(c[8 * j: 8 * j + 8], "little") for j in range(4))
        elif k == "threshold":
            e.a = _check_u64("threshold", o[2])
        elif k == "membership":
            e.a, e.count, e.list_off = _check_u64("membership value", o[1]), len(o[2]), len(lists)
            lists.extend(_check_u64("set element", x) for x in o[2])
    return arr, lists, kinds


def verify_ops(ops, envelopes, reasons=False):
    """The reference's verify_range / verify_equality / verify_equality_with_commitment / verify_threshold / verify_membership /
    verify_improvement / verify_consistency for a mixed list in ONE library call (zkp_stmt_verify, include/libzkp_hip_statements.h): ops are
    the tuples process_ops takes, envelopes[i] the proof held against ops[i]; an equality op may also be ("equality_commitment", bytes32).
    Every statement is compared with its envelope on the GPU.  List of bools in the caller's order, or with reasons=True of (bool, why) with
    why one of _native.STMT_ACCEPTED / _ENVELOPE / _STATEMENT / _PROOF.  Never raises on malformed envelopes (they are False)."""
    blobs = [bytes(e) for e in envelopes]
    n = len(blobs)
    if len(ops) != n:
        raise ValueError("ops, envelopes must have equal length")
    if n == 0:
        return []
    arr, lists, kinds = statement_ops(ops)
    for kind, op in ((0, _native.OP_EQUALITY), (1, _native.OP_MEMBERSHIP)):          # a Groth16 key only for the circuits whose kind occurs
        if op in kinds:
            _ensure_key(kind, verifier=True)
    la = np.array(lists if lists else [0], dtype=np.uint64)
    blob = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.uint64, count=n), out=off[1:])
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    ok, why = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
    _native.check(_native.lib().zkp_stmt_verify(n, ctypes.byref(arr), _P(la), len(lists), _P(blob), _P(off), _P(ok), _P(why) if reasons else None), "zkp_stmt_verify")
    return [(bool(a == 1), int(w)) for a, w in zip(ok, why)] if reasons else (ok == 1).tolist()


def verify_statements_counters(reset=True):
    """What verify_ops did, summed over the shards since the last reset (zkp_stmt_counters, include/libzkp_hip_statements.h; always counted):
    {"envelopes": envelopes seen, "refused_envelope" / "refused_statement" / "refused_proof": envelopes refused by the envelope step, the
    statement step, their scheme's verifier, "ms": host wall time of the calls (of their slices)}.  reset=True zeroes the counters."""
    return _read_counters("zkp_stmt_counters", (), ("envelopes", "refused_envelope", "refused_statement", "refused_proof"), reset)


def verify_equality_with_commitment_batch(proofs, commitments):
    """Batched verify_equality_with_commitment (equality_proof.rs:34-60): the envelope must carry exactly that commitment."""
    blobs = [bytes(p) for p in proofs]
    cms = [bytes(c) for c in commitments]
    if len(cms) != len(blobs):
        raise ValueError("proofs, commitments must have equal length")
    crypto = _verify_snark_envelopes(0, blobs)
    return [ok and len(c) == 32 and len(b) == 298 and b[266:] == c for ok, b, c in zip(crypto, blobs, cms)]


def verify_equality_with_commitment(proof, commitment):
    return verify_equality_with_commitment_batch([proof], [commitment])[0]


def verify_equality(proof, val1, val2):
    """equality_proof.rs:52-59"""
    val1, val2 = _check_u64("val1", val1), _check_u64("val2", val2)
    if val1 != val2:
        return False
    return verify_equality_with_commitment(proof, snark_commit_value(val1))


def verify_membership_batch(proofs, sets):
    """Batched verify_membership (set_membership.rs:40-70): the embedded set must equal `set` as a multiset."""
    blobs = [bytes(p) for p in proofs]
    if len(sets) != len(blobs):
        raise ValueError("proofs, sets must have equal length")
    crypto = _verify_snark_envelopes(1, blobs)
    out = []
    for ok, b, st in zip(crypto, blobs, sets):
        good = ok and len(b) >= 14
        if good:
            n = int.from_bytes(b[10:14], "little")
            emb = [int.from_bytes(b[14 + 8 * i: 22 + 8 * i], "little") for i in range(n)] if len(b) == 10 + 4 + 8 * n + 256 + 32 else None
            good = emb is not None and sorted(emb) == sorted(_check_u64("set element", x) for x in st)
        out.append(bool(good))
    return out


def verify_membership(proof, set):  # noqa: A002
    return verify_membership_batch([proof], [list(set)])[0]


def verify_consistency_batch(proofs):
    """Batched verify_consistency (consistency_proof.rs:24-32): list of bools."""
    n = len(proofs)
    if n == 0:
        return []
    blobs = [bytes(p) for p in proofs]
    buf, lens, stride = _rows(blobs, 1 << 20)
    ok = np.zeros(n, dtype=np.uint8)
    _native.check(_native.lib().zkp_hip_verify_consistency_batch(n, _P(buf), stride, _P(lens), _P(ok)), "zkp_hip_verify_consistency_batch")
    return ok.astype(bool).tolist()


def verify_consistency(proof):
    return verify_consistency_batch([proof])[0]


def verify_improvement_batch(proofs, olds):
    """Batched verify_improvement (improvement_proof.rs:37-68): list of bools."""
    n = len(proofs)
    if len(olds) != n:
        raise ValueError("proofs, olds must have equal length")
    if n == 0:
        return []
    ov = np.array([_check_u64("old", x) for x in olds], dtype=np.uint64)
    blobs = [bytes(p) for p in proofs]
    buf, lens, stride = _rows(blobs, 8192)
    ok = np.zeros(n, dtype=np.uint8)
    _native.check(_native.lib().zkp_hip_verify_improvement_batch(n, _P(buf), stride, _P(lens), _P(ov), _P(ok)), "zkp_hip_verify_improvement_batch")
    return ok.astype(bool).tolist()


def verify_improvement(proof, old):
    return verify_improvement_batch([proof], [old])[0]


def verify_threshold(proof, threshold):
    return verify_threshold_batch([proof], [threshold])[0]


def verify_range(proof, min, max):  # noqa: A002
    return verify_range_batch([proof], [min], [max])[0]


def prove_range(value, min, max):  # noqa: A002  (reference argument names)
    value, mn, mx = _check_u64("value", value), _check_u64("min", min), _check_u64("max", max)
    validate_range_params(value, mn, mx)
    return prove_range_batch([value], [mn], [mx])[0]


def prove_range_with_bits(value, min, max, n_bits):  # noqa: A002
    """range_proof.rs:14-27: value - min and max - value must both fit in n_bits (8, 16, 32 or 64)."""
    value, mn, mx = _check_u64("value", value), _check_u64("min", min), _check_u64("max", max)
    validate_range_params(value, mn, mx)
    return prove_range_batch([value], [mn], [mx], n_bits=n_bits)[0]


# ---------------------------------------------------------------- batch registry (batch.rs:18-175)
_registry = {}
_registry_lock = threading.Lock()


def _allocate_batch_id():
    while True:
        bid = secrets.randbits(64)
        if bid != 0 and bid not in _registry:
            return bid


def create_proof_batch():
    """batch.rs:36-48; with a store directory configured every change is written through (batch_store.rs:157-162)."""
    with _registry_lock:
        bid = _allocate_batch_id()
        _registry[bid] = []
        batch_store.persist_batch_if_configured(bid, _registry[bid])
        return bid


def _with_batch(batch_id, op):
    with _registry_lock:
        if batch_id not in _registry:
            raise ValueError("Invalid batch ID: %d" % batch_id)
        _registry[batch_id].append(op)
        batch_store.persist_batch_if_configured(batch_id, _registry[batch_id])


def open_batch_from_store(batch_id):
    """batch.rs:192-210: cold start from the on-disk store."""
    d = batch_store._store_dir_required()
    with _registry_lock:
        if batch_id in _registry:
            raise ValueError("batch %d is already open in this process" % batch_id)
        _registry[batch_id] = batch_store.read_batch_file(d, batch_id)


def refresh_batch_from_store(batch_id):
    """batch.rs:214-232: pick up what another process wrote."""
    d = batch_store._store_dir_required()
    with _registry_lock:
        if batch_id not in _registry:
            raise ValueError("batch %d is not loaded in this process" % batch_id)
        _registry[batch_id] = batch_store.read_batch_file(d, batch_id)


def export_batch_to_file(batch_id, dest):
    """batch.rs:236-245"""
    with _registry_lock:
        if batch_id not in _registry:
            raise ValueError("Invalid batch ID: %d" % batch_id)
        batch_store.export_proof_batch_to_path(_registry[batch_id], dest)


def import_batch_from_file(src):
    """batch.rs:249-260: new batch id; persisted if a store is configured."""
    ops = batch_store.import_proof_batch_from_path(src)
    with _registry_lock:
        bid = _allocate_batch_id()
        _registry[bid] = ops
        batch_store.persist_batch_if_configured(bid, ops)
        return bid


def batch_add_range_proof(batch_id, value, min, max):  # noqa: A002
    value, mn, mx = _check_u64("value", value), _check_u64("min", min), _check_u64("max", max)
    validate_range_params(value, mn, mx)
    _with_batch(batch_id, ("range", value, mn, mx))


def batch_add_equality_proof(batch_id, val1, val2):
    val1, val2 = _check_u64("val1", val1), _check_u64("val2", val2)
    if val1 != val2:
        raise ValueError("values are not equal")
    _with_batch(batch_id, ("equality", val1, val2))


def batch_add_threshold_proof(batch_id, values, threshold):
    values = [_check_u64("value", x) for x in values]
    validate_threshold_params(values, _check_u64("threshold", threshold))
    _with_batch(batch_id, ("threshold", tuple(values), threshold))


def batch_add_membership_proof(batch_id, value, set):  # noqa: A002
    value = _check_u64("value", value)
    the_set = [_check_u64("set element", x) for x in set]
    if not the_set:                                                  # batch.rs:94-97 validates membership only
        raise ValueError("set cannot be empty")
    if value not in the_set:
        raise ValueError("value %d is not in the provided set" % value)
    _with_batch(batch_id, ("membership", value, tuple(the_set)))


def batch_add_improvement_proof(batch_id, old, new):
    old, new = _check_u64("old", old), _check_u64("new", new)
    if new <= old:
        raise ValueError("new value must be greater than old value")
    _with_batch(batch_id, ("improvement", old, new))


def batch_add_consistency_proof(batch_id, data):
    data = [_check_u64("value", x) for x in data]
    validate_consistency_params(data)
    _with_batch(batch_id, ("consistency", tuple(data)))


def process_batch(batch_id, seeds=None, self_check=False):
    """batch.rs:110-140: consumes the batch (even if proving fails), returns proofs in insertion order.  self_check=True: every proof is
    verified on the GPU against its own op before it is returned (process_ops); a refused op fails the batch like any failed op."""
    with _registry_lock:
        if batch_id not in _registry:
            raise ValueError("Invalid batch ID: %d" % batch_id)
        ops = _registry.pop(batch_id)
    batch_store.delete_batch_file_if_configured(batch_id)            # batch.rs:120-121
    for op in ops:
        if op[0] == "membership" and len(op[2]) > MAX_SET_SIZE:      # set_membership.rs:14 (validate_set_size at prove time)
            raise ValueError("set size %d exceeds maximum allowed size %d" % (len(op[2]), MAX_SET_SIZE))
    return process_ops(ops, seeds, self_check)


def process_ops(ops, seeds=None, self_check=False):
    """The whole mixed batch through ONE C-ABI call (zkp_hip_process_batch, the compiled replacement of
    advanced::process_batch); same result as prove_ops, without the per-variant Python marshalling.  self_check=True sets
    ZKP_HIP_OP_SELF_CHECK on every op: each scheme's verifier runs over the proofs where they lie in HBM, against the op's own parameters,
    before anything is returned; the proofs are the same bytes, and an op whose proof is refused fails the batch (status 2)."""
    n = len(ops)
    if n == 0:
        return []
    arr, la, cap, sp = _marshal_ops(ops, seeds, self_check)
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    st = np.zeros(n, dtype=np.int32)
    rc = _native.lib().zkp_hip_process_batch(n, ctypes.byref(arr), _P(la), sp, _P(out), cap, _P(off), _P(st))
    if rc < 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    if rc != 0:
        i = int(np.nonzero(st)[0][0])
        raise ZkpBackendError("Proof generation failed: operation %d (%s) failed with status %d" % (i, ops[i][0], int(st[i])))
    raw = out.tobytes()
    return [raw[int(off[i]): int(off[i + 1])] for i in range(n)]


def _marshal_ops(ops, seeds, self_check):
    """The op tuples of batch_add_* as the C ABI takes them: (zkp_hip_op array, value lists, an upper bound of the proofs' bytes, seeds
    pointer or None).  Loads the Groth16 keys the ops need."""
    n = len(ops)
    seeds = None if seeds is None else bytes(seeds)
    if seeds is not None and len(seeds) != 32 * n:
        raise ValueError("seeds must hold 32 bytes per op")
    code = {"range": _native.OP_RANGE, "equality": _native.OP_EQUALITY, "threshold": _native.OP_THRESHOLD,
            "membership": _native.OP_MEMBERSHIP, "improvement": _native.OP_IMPROVEMENT, "consistency": _native.OP_CONSISTENCY}
    arr = (_native.Op * n)()
    lists = []
    cap = 0
    for i, o in enumerate(ops):
        k = o[0]
        e = arr[i]
        e.kind = code[k] | (_native.OP_SELF_CHECK if self_check else 0)
        if k == "range":
            e.a, e.b, e.c = o[1], o[2], o[3]; cap += 1478
        elif k == "equality":
            e.a, e.b = o[1], o[2]; cap += 298
            _ensure_key(0)
        elif k == "improvement":
            e.a, e.b = o[1], o[2]; cap += 3527
        elif k == "threshold":
            e.a, e.count, e.list_off = o[2], len(o[1]), len(lists); lists.extend(o[1]); cap += 762
        elif k == "membership":
            e.a, e.count, e.list_off = o[1], len(o[2]), len(lists); lists.extend(o[2]); cap += 10 + 4 + 8 * len(o[2]) + 256 + 32
            _ensure_key(1)
        else:
            e.count, e.list_off = len(o[1]), len(lists); lists.extend(o[1])
            cap += 10 + 4 + 32 * len(o[1]) + (4 + 672 + 32) * max(len(o[1]) - 1, 0) + 32
    la = np.array(lists if lists else [0], dtype=np.uint64)
    return arr, la, cap, None if seeds is None else ctypes.c_char_p(seeds)


def process_ops_sealed(ops, counts, metadata=None, seeds=None, self_check=False):
    """process_ops followed by create_composite_proof / create_proof_with_metadata per group of ops, without the proofs leaving the GPU in
    between: the batch is staged and proved, libzkp_seal_batch (include/libzkp_hip_seal.h) frames and hashes container i from the proofs
    of the next counts[i] consecutive ops where they lie in HBM (a batch staged on several shards is fetched once first), and the batch
    is freed.  metadata: None, or one dict (str -> bytes) per container, written in dict order.  Returns the containers as a list of
    bytes, the same bytes the host functions give for process_ops' proofs under the same seeds."""
    from . import composite
    n, m = len(ops), len(counts)
    if sum(int(c) for c in counts) != n or any(int(c) < 0 for c in counts):
        raise ValueError("counts must be non-negative and sum to the number of ops")
    if metadata is not None and len(metadata) != m:
        raise ValueError("metadata must hold one dict per container")
    if m == 0:
        return []
    for i, c in enumerate(counts):
        if int(c) == 0:
            raise ValueError("proof list cannot be empty")            # create_composite_proof's error, before anything is proved
    L = _native.lib()
    if not hasattr(L, "libzkp_seal_batch"):
        raise _native.NativeError("this build of libzkp_hip.so has no libzkp_seal_batch")
    arr, la, cap, sp = _marshal_ops(ops, seeds, self_check)
    first = composite.seal_offsets([int(c) for c in counts])
    meta_blob = meta_off = None
    if metadata is not None:
        wires = [composite._metadata_wire(md) for md in metadata]
        meta_blob, meta_off = np.frombuffer(b"".join(wires) or b"\0", dtype=np.uint8), composite.seal_offsets([len(w) for w in wires])
    total_cap = cap + 4 * n + 44 * m + (int(meta_off[-1]) if meta_off is not None else 0)          # an upper bound: every container sealed
    out, out_off, status = np.empty(max(total_cap, 1), dtype=np.uint8), np.zeros(m + 1, dtype=np.uint64), np.zeros(m, dtype=np.uint8)
    ptr = lambda a: None if a is None else _P(a)  # noqa: E731
    batch = ctypes.c_void_p()
    rc = L.zkp_hip_batch_stage(n, ctypes.byref(arr), _P(la), sp, ctypes.byref(batch))
    if rc < 0:
        raise ZkpBackendError("Backend error: %s" % _native.last_error())
    try:
        rc = L.zkp_hip_batch_prove_async(batch)
        if rc == 0:
            rc = L.libzkp_seal_batch(batch, m, _P(first), ptr(meta_blob), ptr(meta_off), _P(out), total_cap, _P(out_off), _P(status))
        if rc < 0:
            raise ZkpBackendError("Backend error: %s" % _native.last_error())
    finally:
        L.zkp_hip_batch_free(batch)
    for i in np.flatnonzero(status != _native.SEAL_SEALED):
        i = int(i)
        if status[i] == _native.SEAL_FAILED_OP:
            raise ZkpBackendError("Proof generation failed: an operation of container %d (ops %d .. %d) failed" % (i, int(first[i]), int(first[i + 1]) - 1))
        raise ValueError("composite proof %d would not be read back: %s" % (i, composite._unreadable_reason(range(int(counts[i])), metadata[i] if metadata is not None else {})))
    raw = out[:int(out_off[-1])].tobytes()
    return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(m)]


def seal_counters(reset=True):
    """What create_composite_proofs and process_ops_sealed did, summed over the shards since the last reset (libzkp_seal_counters,
    include/libzkp_hip_seal.h; always counted): {"containers": containers seen, "sealed": containers written, "envelopes": their inner
    proofs, "bytes": their bytes, "ms": host wall time of the device half of the calls}.  reset=True zeroes the counters."""
    return _read_counters("libzkp_seal_counters", (), ("containers", "sealed", "envelopes", "bytes"), reset)


KINDS = ("range", "threshold", "consistency", "equality", "membership", "improvement")


def prove_kind(kind, sel, seeds=None):
    """One batched device call for ops of one variant (tuples as stored by batch_add_*)."""
    if kind == "range":
        return prove_range_batch([o[1] for o in sel], [o[2] for o in sel], [o[3] for o in sel], seeds=seeds)
    if kind == "threshold":
        return prove_threshold_batch([o[1] for o in sel], [o[2] for o in sel], seeds=seeds)
    if kind == "consistency":
        return prove_consistency_batch([o[1] for o in sel], seeds=seeds)
    if kind == "equality":
        return prove_equality_batch([o[1] for o in sel], [o[2] for o in sel], seeds=seeds)
    if kind == "membership":
        return prove_membership_batch([o[1] for o in sel], [list(o[2]) for o in sel], seeds=seeds)
    if kind == "improvement":
        return prove_improvement_batch([o[1] for o in sel], [o[2] for o in sel])
    raise ValueError("unsupported proof type: %s" % kind)


def prove_ops(ops, seeds=None, prover=prove_kind, select=None):
    """Bucket by variant (one batched device call each), then restore insertion order (batch.rs:123-131 is
    order-preserving).  `select(kind, idx)` may narrow each bucket to the indices this process should prove
    (multi-GPU sharding); unproved ops stay None."""
    seeds = None if seeds is None else bytes(seeds)
    if seeds is not None and len(seeds) != 32 * len(ops):
        raise ValueError("seeds must hold 32 bytes per op")
    out = [None] * len(ops)
    for kind in KINDS:
        idx = [i for i, o in enumerate(ops) if o[0] == kind]
        if select is not None:
            idx = select(kind, idx)
        if not idx:
            continue
        sd = None if seeds is None else b"".join(seeds[32 * i: 32 * i + 32] for i in idx)
        proofs = prover(kind, [ops[i] for i in idx], sd)
        for i, p in zip(idx, proofs):
            out[i] = p
    return out


def get_batch_status(batch_id):
    with _registry_lock:
        if batch_id not in _registry:
            raise ValueError("Invalid batch ID: %d" % batch_id)
        ops = list(_registry[batch_id])
    out = {"total_operations": len(ops)}
    for key, name in (("range_proofs", "range"), ("equality_proofs", "equality"), ("threshold_proofs", "threshold"),
                      ("membership_proofs", "membership"), ("improvement_proofs", "improvement"), ("consistency_proofs", "consistency")):
        out[key] = sum(1 for o in ops if o[0] == name)
    return out


def clear_batch(batch_id):
    with _registry_lock:
        _registry.pop(batch_id, None)
    batch_store.delete_batch_file_if_configured(batch_id)            # batch.rs:183-184


# ---------------------------------------------------------------- benchmark harness (advanced/mod.rs:83-172)
def benchmark_proof_generation_numeric(proof_type, iterations):
    runners = {"range": lambda: prove_range(50, 0, 100),                          # mod.rs:94-104 fixed inputs
               "threshold": lambda: prove_threshold([10, 20, 30, 40], 50),
               "consistency": lambda: prove_consistency([10, 20, 30, 40, 50]),
               "equality": lambda: prove_equality(42, 42),
               "membership": lambda: prove_membership(25, [10, 20, 25, 30, 40]),
               "improvement": lambda: prove_improvement(30, 50)}                     # mod.rs:100
    if proof_type not in runners:
        raise ValueError("unsupported proof type: %s" % proof_type)
    times = []
    for _ in range(iterations):
        t0 = time.perf_counter()
        runners[proof_type]()
        dt = time.perf_counter() - t0
        perf.METRICS.record_operation(proof_type + "_proof", dt)                  # mod.rs:113-123
        times.append(dt * 1e3)
    if not times:
        raise ValueError("no successful proof generations")
    total = sum(times)
    avg = total / len(times)
    var = sum((x - avg) ** 2 for x in times) / len(times)
    return {
        "iterations": float(iterations), "successful_iterations": float(len(times)), "success_rate": 100.0,
        "total_time_ms": total, "avg_time_ms": avg, "min_time_ms": min(times), "max_time_ms": max(times),
        "std_dev_ms": var ** 0.5, "proofs_per_second": len(times) / (total / 1e3), "throughput_ms_per_proof": total / len(times),
    }


# ---------------------------------------------------------------- cache / metrics entry points (advanced/mod.rs:25-80,175-191,218-221)
def clear_cache():
    perf.CACHE.clear()


def get_cache_stats():
    return {"size": perf.CACHE.size()}


def get_performance_metrics():
    return perf.performance_metrics()


def prove_range_cached(value, min, max):  # noqa: A002
    """advanced/mod.rs:175-191: a hit returns the cached proof bytes; a miss proves, records the timing and stores."""
    value, mn, mx = _check_u64("value", value), _check_u64("min", min), _check_u64("max", max)
    key = perf.generate_cache_key("range_proof", ("%d:%d:%d" % (value, mn, mx)).encode())
    hit = perf.CACHE.get(key)
    if hit is not None:
        return hit
    t0 = time.perf_counter()
    proof = prove_range(value, mn, mx)
    perf.METRICS.record_operation("range_proof", time.perf_counter() - t0)
    perf.CACHE.put(key, proof)
    return proof


def prove_threshold_optimized(values, threshold):
    """advanced/mod.rs:218-221: delegates to prove_threshold."""
    return prove_threshold(values, threshold)


def benchmark_proof_generation(proof_type, iterations):
    """mod.rs:204-215: the Python variant stringifies every value and adds proof_type."""
    res = {k: repr(float(v)) for k, v in benchmark_proof_generation_numeric(proof_type, iterations).items()}
    res["proof_type"] = proof_type
    return res
