"""TEST INFRASTRUCTURE: composite proofs ("COMP" containers) built byte by byte, with metadata keys given as raw bytes so that a test can
write what no str encodes, and their digest from first principles (hashlib).  Shared by tests/test_emul_composites.py and the child
processes of tests/test_gpu_composites.py."""
import hashlib
import itertools


def u32(x):
    return int(x).to_bytes(4, "little")


def proof(n, scheme=9, salt=0, version=2):
    """a format-valid envelope of n >= 10 bytes: no commitment, n - 10 payload bytes"""
    return bytes([version, scheme]) + u32(n - 10) + u32(0) + bytes((7 * k + salt + n) & 0xff for k in range(n - 10))


def entry(key, value):
    return u32(len(key)) + key + u32(len(value)) + value


def digest_of(proofs, meta):
    """the digest from first principles: the last value of a repeated key, keys ascending bytewise"""
    last = {}
    for k, v in meta:
        last[k] = v
    h = hashlib.sha256(b"COMPOSITE_PROOF:" + u32(len(proofs)))
    for p in proofs:
        h.update(p)
    for k in sorted(last):
        h.update(entry(k, last[k]))
    return h.digest()


def comp(proofs=(), meta=(), digest=None, nproofs=None, nmeta=None):
    body = b"COMP" + u32(len(proofs) if nproofs is None else nproofs) + u32(len(meta) if nmeta is None else nmeta)
    body += b"".join(u32(len(p)) + p for p in proofs) + b"".join(entry(k, v) for k, v in meta)
    return body + (digest_of(proofs, meta) if digest is None else digest)


def residue_family():
    """(container, proofs, metadata): hashed lengths 39 .. 169, every residue mod 64, steered by one value of 0 .. 130 bytes"""
    for vl in range(131):
        m = [(b"v", bytes((vl + k) & 0xff for k in range(vl)))]
        yield comp([proof(10)], m), [proof(10)], m


def straddle_family():
    """(container or stray bytes, proofs or None, metadata): seven inner proofs of 10 .. 13 bytes, every combination of the first three,
    behind 0 .. 7 stray bytes (a one-container "gap" that is malformed), so that the proofs lie at every source alignment"""
    for before in range(8):
        if before:
            yield bytes(before), None, None
        for lens in itertools.product((10, 11, 12, 13), repeat=3):
            proofs = [proof(n, salt=before + k) for k, n in enumerate(lens + (10, 13, 11, 12))]
            m = [(b"k" * (before % 3), b"v" * before)]
            yield comp(proofs, m), proofs, m


def four_mib():
    """a container of exactly 4 MiB and the same with one byte more: five proofs below the payload limit, metadata that fills the rest"""
    proofs = [proof(900000, salt=s) for s in range(4)] + [proof((4 << 20) - 12 - 5 * 4 - 32 - 4 * 900000 - 500, salt=4)]
    room = (4 << 20) - (12 + sum(4 + len(p) for p in proofs) + 32)
    at, over = [(b"k", bytes(room - 9))], [(b"k", bytes(room - 8))]
    return (comp(proofs, at), proofs, at), (comp(proofs, over), proofs, over)
