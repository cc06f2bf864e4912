"""Byte formats around the proving path and the batched verification front ends (row N2):

  Proof envelope parsing            /root/reference/src/proof/mod.rs:38-83  (limits: utils/limits.rs)
  CompositeProof ("COMP" container) /root/reference/src/utils/composition.rs:31-331
  create_composite_proof, verify_composite_proof[_integrity_only], create_proof_with_metadata, extract_proof_metadata
                                    /root/reference/src/advanced/composite.rs:10-59
  validate_proof_chain, get_proof_info            /root/reference/src/advanced/mod.rs:224-247
  verify_proofs_parallel, verify_proof_cryptographic
                                    /root/reference/src/utils/performance.rs:251-293, utils/proof_helpers.rs:156-247

Pure host-side framing (SHA-256, length-prefixed fields) around proofs that the GPU produces and verifies; the
cryptographic checks go through libzkp_amd.api.verify_envelopes, the library's one call for a list of envelopes of any scheme
(Bulletproofs family, STARK, Groth16 pairing check).
Error mapping as in api.py: InvalidInput -> ValueError, InvalidProofFormat -> TypeError (error_handling.rs:39-50)."""
import hashlib

MAX_PROOF_TOTAL_BYTES = 1 << 20
MAX_PROOF_PAYLOAD_BYTES = 900 * 1024
MAX_COMMITMENT_BYTES = 256
MAX_COMPOSITE_PROOF_BYTES = 4 << 20
PROOF_VERSION = 2
SCHEME_BY_NAME = {"range": 1, "equality": 2, "threshold": 3, "membership": 4, "improvement": 5, "consistency": 6}


class ProofFormatError(TypeError):
    """ZkpError::InvalidProofFormat"""


def parse_proof(data):
    """Proof::from_bytes: (version, scheme, proof, commitment)"""
    data = bytes(data)
    if len(data) > MAX_PROOF_TOTAL_BYTES:
        raise ProofFormatError("Invalid proof format: proof too large: max %d bytes" % MAX_PROOF_TOTAL_BYTES)
    if len(data) < 10:
        raise ProofFormatError("Invalid proof format: proof too short for header")
    plen, clen = int.from_bytes(data[2:6], "little"), int.from_bytes(data[6:10], "little")
    if plen > MAX_PROOF_PAYLOAD_BYTES or clen > MAX_COMMITMENT_BYTES:
        raise ProofFormatError("Invalid proof format: proof or commitment payload exceeds limit")
    if len(data) != 10 + plen + clen:
        raise ProofFormatError("Invalid proof format: proof byte length mismatch")
    return data[0], data[1], data[10:10 + plen], data[10 + plen:]


def _composition_hash(proofs, metadata):
    h = hashlib.sha256(b"COMPOSITE_PROOF:" + len(proofs).to_bytes(4, "little"))
    for p in proofs:
        h.update(p)
    for k in sorted(metadata):
        kb = k.encode("utf-8")
        h.update(len(kb).to_bytes(4, "little") + kb + len(metadata[k]).to_bytes(4, "little") + metadata[k])
    return h.digest()


def _serialize_composite(proofs, metadata):
    out = b"COMP" + len(proofs).to_bytes(4, "little") + len(metadata).to_bytes(4, "little")
    for p in proofs:
        out += len(p).to_bytes(4, "little") + p
    for k, v in metadata.items():                      # the reference iterates a HashMap here: any order is a valid encoding
        kb = k.encode("utf-8")
        out += len(kb).to_bytes(4, "little") + kb + len(v).to_bytes(4, "little") + v
    return out + _composition_hash(proofs, metadata)


def parse_composite(data):
    """CompositeProof::from_bytes: (list of proof envelopes, metadata dict); raises ProofFormatError"""
    data = bytes(data)
    if len(data) > MAX_COMPOSITE_PROOF_BYTES:
        raise ProofFormatError("Invalid proof format: composite proof too large: max %d bytes" % MAX_COMPOSITE_PROOF_BYTES)
    if len(data) < 12:
        raise ProofFormatError("Invalid proof format: composite proof too short: expected at least 12 bytes, got %d" % len(data))
    if data[:4] != b"COMP":
        raise ProofFormatError("Invalid proof format: invalid composite proof header: expected 'COMP', got '%r'" % list(data[:4]))
    nproofs, nmeta = int.from_bytes(data[4:8], "little"), int.from_bytes(data[8:12], "little")
    if nproofs > 1000 or nmeta > 1000:
        raise ProofFormatError("Invalid proof format: composite proof has too many items: proofs=%d, metadata=%d" % (nproofs, nmeta))
    off, proofs, metadata = 12, [], {}
    for _ in range(nproofs):
        if off + 4 > len(data):
            raise ProofFormatError("Invalid proof format: truncated proof length")
        n = int.from_bytes(data[off:off + 4], "little"); off += 4
        if off + n > len(data):
            raise ProofFormatError("Invalid proof format: truncated proof data")
        parse_proof(data[off:off + n])
        proofs.append(data[off:off + n]); off += n
    for i in range(nmeta):
        if off + 4 > len(data):
            raise ProofFormatError("Invalid proof format: truncated metadata header at index %d: offset=%d, data_len=%d" % (i, off, len(data)))
        kl = int.from_bytes(data[off:off + 4], "little"); off += 4
        if kl > 1024:
            raise ProofFormatError("Invalid proof format: metadata key too large at index %d: key_len=%d" % (i, kl))
        if off + kl > len(data):
            raise ProofFormatError("Invalid proof format: truncated metadata key at index %d: offset=%d, key_len=%d, data_len=%d" % (i, off, kl, len(data)))
        try:
            key = data[off:off + kl].decode("utf-8")
        except UnicodeDecodeError:
            raise ProofFormatError("Invalid proof format: invalid metadata key at index %d: non-utf8 bytes" % i) from None
        off += kl
        if off + 4 > len(data):
            raise ProofFormatError("Invalid proof format: truncated metadata value length at index %d: offset=%d, data_len=%d" % (i, off, len(data)))
        vl = int.from_bytes(data[off:off + 4], "little"); off += 4
        if vl > 65536:
            raise ProofFormatError("Invalid proof format: metadata value too large at index %d: value_len=%d" % (i, vl))
        if off + vl > len(data):
            raise ProofFormatError("Invalid proof format: truncated metadata value at index %d: offset=%d, value_len=%d, data_len=%d" % (i, off, vl, len(data)))
        metadata[key] = data[off:off + vl]; off += vl
    if off + 32 > len(data):
        raise ProofFormatError("Invalid proof format: missing composition hash")
    if off + 32 != len(data):
        raise ProofFormatError("Invalid proof format: trailing bytes after composition hash: %d extra byte(s)" % (len(data) - off - 32))
    if data[off:off + 32] != _composition_hash(proofs, metadata):
        raise ProofFormatError("Invalid proof format: composition hash mismatch")
    return proofs, metadata


def create_composite_proof(proof_list):
    if not proof_list:
        raise ValueError("proof list cannot be empty")
    proofs = [bytes(p) for p in proof_list]
    for p in proofs:
        parse_proof(p)
    return _serialize_composite(proofs, {})


def create_proof_with_metadata(proof_data, metadata):
    proof = bytes(proof_data)
    parse_proof(proof)
    return _serialize_composite([proof], {str(k): bytes(v) for k, v in metadata.items()})


def _metadata_wire(metadata):
    """a metadata dict (str -> bytes) in wire form, in dict order: (u32 key_len | key | u32 value_len | value)*"""
    out = b""
    for k, v in metadata.items():
        kb, v = str(k).encode("utf-8"), bytes(v)
        out += len(kb).to_bytes(4, "little") + kb + len(v).to_bytes(4, "little") + v
    return out


def _unreadable_reason(proofs, metadata):
    """why the library does not seal what the reference would write: CompositeProof::from_bytes would refuse to read it back"""
    if len(proofs) > 1000 or len(metadata) > 1000:
        return "composite proof has too many items: proofs=%d, metadata=%d" % (len(proofs), len(metadata))
    for k, v in metadata.items():
        if len(str(k).encode("utf-8")) > 1024:
            return "metadata key too large: key_len=%d" % len(str(k).encode("utf-8"))
        if len(bytes(v)) > 65536:
            return "metadata value too large: value_len=%d" % len(bytes(v))
    return "composite proof too large: max %d bytes" % MAX_COMPOSITE_PROOF_BYTES


def seal_offsets(lengths):
    """n lengths -> the n + 1 offsets of a packed list (uint64)"""
    import numpy as np
    off = np.zeros(len(lengths) + 1, dtype=np.uint64)
    if len(lengths):
        np.cumsum(np.fromiter(lengths, dtype=np.uint64, count=len(lengths)), out=off[1:])
    return off


def create_composite_proofs(proof_lists, metadata=None, errors="raise"):
    """create_composite_proof / create_proof_with_metadata for a list of containers in ONE library call (libzkp_seal_composites,
    include/libzkp_hip_seal.h): container i holds the envelopes of proof_lists[i] and, when `metadata` is given, the entries of the dict
    metadata[i] (str -> bytes) in dict order; the containers are framed and their digests computed on the GPU.  Returns a list of bytes.
    errors="raise": for the first container that the reference's own creation refuses (an empty list, an envelope that Proof::from_bytes
    refuses) the host function runs on it and raises the reference's ValueError / ProofFormatError; a container that
    CompositeProof::from_bytes would not read back (too many items, a key or value beyond its limit, more than 4 MiB) raises ValueError.
    errors="none": those places hold None."""
    import ctypes
    import numpy as np
    from . import _native
    if errors not in ("raise", "none"):
        raise ValueError("errors must be 'raise' or 'none'")
    lists = [[bytes(p) for p in lst] for lst in proof_lists]
    n = len(lists)
    if metadata is not None and len(metadata) != n:
        raise ValueError("metadata must hold one dict per container")
    if n == 0:
        return []
    L = _native.lib()
    if not hasattr(L, "libzkp_seal_composites"):
        raise _native.NativeError("this build of libzkp_hip.so has no libzkp_seal_composites")
    envs = [p for lst in lists for p in lst]
    env_blob = np.frombuffer(b"".join(envs) or b"\0", dtype=np.uint8)
    env_off, first = seal_offsets([len(p) for p in envs]), seal_offsets([len(lst) for lst in lists])
    vp = ctypes.c_void_p
    meta_blob = meta_off = None
    if metadata is not None:
        wires = [_metadata_wire(m) for m in metadata]
        meta_blob, meta_off = np.frombuffer(b"".join(wires) or b"\0", dtype=np.uint8), seal_offsets([len(w) for w in wires])
    ptr = lambda a: None if a is None else a.ctypes.data_as(vp)  # noqa: E731
    out_off, status = np.zeros(n + 1, dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    cap = int(env_off[-1]) + 4 * len(envs) + (int(meta_off[-1]) if meta_off is not None else 0) + 44 * n          # an upper bound: every container sealed
    out = np.empty(max(cap, 1), dtype=np.uint8)
    _native.check(L.libzkp_seal_composites(n, ptr(env_blob), ptr(env_off), len(envs), ptr(first), ptr(meta_blob), ptr(meta_off), ptr(out), cap, ptr(out_off), ptr(status)),
                  "libzkp_seal_composites")
    if errors == "raise":
        for i in np.flatnonzero(status != _native.SEAL_SEALED):
            i = int(i)
            if status[i] == _native.SEAL_REFUSED:
                create_composite_proof(lists[i])
            raise ValueError("composite proof %d would not be read back: %s" % (i, _unreadable_reason(lists[i], metadata[i] if metadata is not None else {})))
    raw = out[:int(out_off[-1])].tobytes()
    return [raw[int(out_off[i]):int(out_off[i + 1])] if status[i] == _native.SEAL_SEALED else None for i in range(n)]


def extract_proof_metadata(composite_bytes):
    return parse_composite(composite_bytes)[1]


def verify_composite_proof_integrity_only(composite_bytes):
    parse_composite(composite_bytes)                   # from_bytes already rejects a wrong digest; verify_integrity is then true
    return True


def verify_proof_cryptographic_batch(envelopes):
    """verify_proof_cryptographic for a list of envelopes (proof_helpers.rs:156-247): one library call for all schemes
    (api.verify_envelopes: the parsing, the pre-checks and the sorting by scheme happen on the GPU)."""
    from . import api
    return api.verify_envelopes(envelopes)


def verify_composite_proof(composite_bytes):
    proofs, _ = parse_composite(composite_bytes)
    return all(verify_proof_cryptographic_batch(proofs))


def _groth16_circuits_in(blob):
    """Which Groth16 circuits (0: equality, 1: membership) the inner envelopes of a container name, from a walk over the proof length
    prefixes alone; a container the walk cannot follow names none (the library decides whether it is malformed)."""
    kinds = set()
    if len(blob) < 12 or blob[:4] != b"COMP":
        return kinds
    nproofs, off = int.from_bytes(blob[4:8], "little"), 12
    for _ in range(min(nproofs, 1000)):
        if off + 6 > len(blob):
            break
        if blob[off + 5] == 2:
            kinds.add(0)
        elif blob[off + 5] == 4:
            kinds.add(1)
        off += 4 + int.from_bytes(blob[off:off + 4], "little")
    return kinds


def verify_composite_proofs(composites, integrity_only=False, errors="false"):
    """verify_composite_proof (or, with integrity_only, verify_composite_proof_integrity_only) for a list of containers in ONE library call
    (zkp_hip_verify_composites, include/libzkp_hip_composites.h): the digests are computed on the GPU, all inner envelopes of all
    well-formed containers go through one pass of the mixed verifier, and the verdicts come back per container as a list of bools.
    errors="false": a malformed container is False.  errors="raise": the first malformed container is parsed again with parse_composite,
    which raises the reference's ProofFormatError for it."""
    import ctypes
    import numpy as np
    from . import _native, api
    if errors not in ("false", "raise"):
        raise ValueError("errors must be 'false' or 'raise'")
    blobs = [bytes(c) for c in composites]
    n = len(blobs)
    if n == 0:
        return []
    if not integrity_only:                                # a Groth16 key only for the circuits whose scheme byte occurs
        needed = set()
        for b in blobs:
            needed |= _groth16_circuits_in(b)
            if len(needed) == 2:
                break
        for kind in sorted(needed):
            api._ensure_key(kind, verifier=True)
    L = _native.lib()
    if not hasattr(L, "zkp_hip_verify_composites"):
        raise _native.NativeError("this build of libzkp_hip.so has no zkp_hip_verify_composites")
    blob = np.frombuffer(b"".join(blobs), dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    np.cumsum(np.fromiter((len(b) for b in blobs), dtype=np.uint64, count=n), out=off[1:])
    if blob.size == 0:
        blob = np.zeros(1, dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    vp = ctypes.c_void_p
    _native.check(L.zkp_hip_verify_composites(n, blob.ctypes.data_as(vp), off.ctypes.data_as(vp), _native.COMPOSITES_INTEGRITY_ONLY if integrity_only else 0,
                                              status.ctypes.data_as(vp)), "zkp_hip_verify_composites")
    if errors == "raise":
        malformed = np.flatnonzero(status == 2)
        if malformed.size:
            parse_composite(blobs[int(malformed[0])])
            raise ProofFormatError("Invalid proof format: composite proof %d is malformed" % int(malformed[0]))      # (not reached while the library and parse_composite agree)
    return (status == 1).tolist()


def verify_composites_counters(reset=True):
    """What verify_composite_proofs did, summed over the shards since the last reset (zkp_hip_composites_counters,
    include/libzkp_hip_composites.h; always counted): {"composites": containers seen, "malformed": containers that
    CompositeProof::from_bytes refuses, "envelopes": inner envelopes handed to the mixed verifier, "ms": host wall time of the calls}.
    reset=True zeroes the counters."""
    from . import api
    return api._read_counters("zkp_hip_composites_counters", (), ("composites", "malformed", "envelopes"), reset)


def verify_proofs_parallel(proofs):
    """[(proof bytes, type name)] -> [bool]: the type must match the envelope's scheme id (performance.rs:269-293)."""
    from . import api
    # an unknown type name matches no scheme id: 255 is not one, and any expected value other than 0 and the envelope's own rejects
    return api.verify_envelopes([bytes(data) for data, _ in proofs], [SCHEME_BY_NAME.get(name, 255) for _, name in proofs])


def validate_proof_chain(proof_chain):
    for b in proof_chain:
        try:
            parse_proof(b)
        except ProofFormatError:
            return False
    return True


def get_proof_info(proof_bytes):
    version, scheme, payload, commitment = parse_proof(proof_bytes)
    return {"version": version, "scheme": scheme, "proof_size": len(payload), "commitment_size": len(commitment)}
