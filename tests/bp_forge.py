"""Forger of well-formed but invalid Bulletproofs envelopes (range: scheme 1, threshold: 3, consistency: 6), built on the
bigint oracle (oracle/py).  Test infrastructure only.

Given a valid envelope, `forgeries()` yields one named forgery for every field the verifier reads a group element or a
scalar from.  Every forgery still parses: the framing is untouched, every 32-byte point field decodes with RFC 9496 and every
scalar field is below l.  Each carries the stage at which the verifier's rules must refuse it:

  "equation"  the wrong value reaches a verification equation of RangeProof::verify_single, which then does not hold.  In the
              GPU verifier's whole-batch check these are the values that enter the random linear combination: the check
              itself has to refuse them.
  "rule"      a rule that comes before any equation refuses the envelope: a proof point that is the identity
              (verify_single), an embedded commitment that is not the one derived from the envelope commitment and the
              bounds (bulletproofs.rs:266-283, 590-600, 520-530), a digest that is not the commitments' SHA-256.  The GPU
              verifier applies these rules in its parse and decode steps, so such an envelope is rejected without entering
              the sum, which then stands for the others.

`excluded()` yields envelopes whose fields do not decode at all (a scalar >= l, a point encoding off the curve, a
non-canonical point encoding); `rejection_stage()` replays the Python oracle and says where it refused an envelope.

Offsets come from the envelope's own length fields, for every bit width (8, 16, 32, 64).
"""
import collections
import ctypes
import hashlib

import numpy as np

from oracle.py import bulletproofs as bp
from oracle.py import ristretto as R
from oracle.py.ristretto import L, P as FIELD_P

SCALAR_NAMES = ("t_x", "t_x_blinding", "e_blinding", "a", "b")
IDENTITY_ENC = bytes(32)
POINT_MUTATIONS = ("plus_B", "neg", "identity")
SCALAR_MUTATIONS = ("plus_1", "neg")

Field = collections.namedtuple("Field", "name off kind")            # kind: "point" | "scalar"; off: byte offset in the envelope
Forgery = collections.namedtuple("Forgery", "name env stage")
Layout = collections.namedtuple("Layout", "scheme body commit n_bits proofs proof_fields commitments extra")
# proofs: [(name, offset, length)]; proof_fields: Fields inside the inner proofs; commitments: point Fields outside them;
# extra: scheme-specific offsets


def _u32(b, o):
    return int.from_bytes(b[o:o + 4], "little")


def to_wire(env):
    """The framing oracle/py/bulletproofs.py reads (decode_proof_body_and_commit) from the envelope framing of the C ABI."""
    bl, cl = _u32(env, 2), _u32(env, 6)
    assert env[0] == 2 and len(env) == 10 + bl + cl
    return bp._wire(env[10:10 + bl], env[10 + bl:])


def _proof_fields(prefix, off, length):
    lg = (length // 32 - 9) // 2
    assert length == 32 * (9 + 2 * lg) and lg in (3, 4, 5, 6)
    f = [Field(prefix + n, off + 32 * i, "point") for i, n in enumerate(("A", "S", "T1", "T2"))]
    f += [Field(prefix + n, off + 128 + 32 * i, "scalar") for i, n in enumerate(SCALAR_NAMES[:3])]
    for j in range(lg):
        f.append(Field("%sL%d" % (prefix, j), off + 224 + 64 * j, "point"))
        f.append(Field("%sR%d" % (prefix, j), off + 256 + 64 * j, "point"))
    f += [Field(prefix + "a", off + 224 + 64 * lg, "scalar"), Field(prefix + "b", off + 256 + 64 * lg, "scalar")]
    return f


def layout(env):
    """Offsets of every field, read from the envelope's own header and length fields."""
    scheme, bl, cl = env[1], _u32(env, 2), _u32(env, 6)
    assert env[0] == 2 and cl == 32 and len(env) == 10 + bl + cl
    body, commit = 10, 10 + bl
    proofs, fields, comms, extra = [], [], [], {}
    if scheme == 1:
        n_bits, pos = _u32(env, body + 16), body + 20
        for name in ("rp_min", "rp_max"):
            ln = _u32(env, pos)
            proofs.append((name, pos + 4, ln)); pos += 4 + ln
        comms = [Field("c_min", pos, "point"), Field("c_max", pos + 32, "point"), Field("value_commitment", commit, "point")]
        assert pos + 64 == commit
    elif scheme == 3:
        n_bits, ln = _u32(env, body + 8), _u32(env, body + 12)
        proofs.append(("rp", body + 16, ln))
        comms = [Field("c_diff", body + 16 + ln, "point"), Field("sum_commitment", commit, "point")]
        assert body + 16 + ln + 32 == commit
    elif scheme == 6:
        n_bits, k = 64, _u32(env, body)
        pos = body + 4 + 32 * k
        comms = [Field("commit%d" % i, body + 4 + 32 * i, "point") for i in range(k)]
        for i in range(1, k):
            ln = _u32(env, pos)
            proofs.append(("rp%d" % i, pos + 4, ln)); pos += 4 + ln
        comms += [Field("c_diff%d" % i, pos + 32 * (i - 1), "point") for i in range(1, k)]
        assert pos + 32 * (k - 1) == commit
        extra = {"k": k, "digest": commit, "commits": body + 4, "diffs": pos}
    else:
        raise ValueError("not a Bulletproofs envelope")
    for name, off, ln in proofs:
        fields += _proof_fields(name + ".", off, ln)
    return Layout(scheme, body, commit, n_bits, proofs, fields, comms, extra)


def _put(env, off, data):
    assert len(data) == 32
    return env[:off] + data + env[off + 32:]


def _point(env, off):
    p = R.decode(env[off:off + 32])
    assert p is not None
    return p


def mutate_point(enc, how):
    p = R.decode(enc)
    assert p is not None
    if how == "plus_B":
        return (p + bp.B).encode()
    if how == "minus_B":
        return (p - bp.B).encode()
    if how == "neg":
        return (-p).encode()
    if how == "identity":
        return IDENTITY_ENC
    raise ValueError(how)


def mutate_scalar(enc, how):
    s = int.from_bytes(enc, "little")
    assert s < L
    return R.scalar_to_bytes(s + 1 if how == "plus_1" else -s)


def _redigest(env, lay):
    k, c0 = lay.extra["k"], lay.extra["commits"]
    return _put(env, lay.extra["digest"], hashlib.sha256(env[c0:c0 + 32 * k]).digest())


def _shift_commitments(env, lay):
    """The envelope commitment moved by B together with every embedded commitment derived from it, so that the framing's
    commitment relations still hold and the wrong commitment reaches the V slot of the verification equation."""
    c = {f.name: f.off for f in lay.commitments}
    put = lambda e, name, how: _put(e, c[name], mutate_point(e[c[name]:c[name] + 32], how))  # noqa: E731
    if lay.scheme == 1:
        return [("commitments_shifted_by_B", put(put(put(env, "value_commitment", "plus_B"), "c_min", "plus_B"), "c_max", "minus_B"))]
    if lay.scheme == 3:
        return [("commitments_shifted_by_B", put(put(env, "sum_commitment", "plus_B"), "c_diff", "plus_B"))]
    out = []
    k = lay.extra["k"]
    for i in range(k):                                                  # commit_i + B: difference i grows by B, difference i + 1 shrinks
        e = put(env, "commit%d" % i, "plus_B")
        if i >= 1:
            e = put(e, "c_diff%d" % i, "plus_B")
        if i + 1 < k:
            e = put(e, "c_diff%d" % (i + 1), "minus_B")
        if k > 1:
            out.append(("commit%d_shifted_by_B_with_differences_and_digest" % i, _redigest(e, lay)))
    return out


def field_forgeries(env):
    """The listed mutations of every point and scalar of the inner proofs and of every commitment: (Forgery, ...)."""
    lay = layout(env)
    out = []
    for f in lay.proof_fields:
        cur = env[f.off:f.off + 32]
        if f.kind == "point":
            for how in POINT_MUTATIONS:
                out.append(Forgery("%s:%s" % (f.name, how), _put(env, f.off, mutate_point(cur, how)), "rule" if how == "identity" else "equation"))
        else:
            for how in SCALAR_MUTATIONS:
                new = mutate_scalar(cur, how)
                if new != cur:                                          # -0 = 0: no forgery
                    out.append(Forgery("%s:%s" % (f.name, how), _put(env, f.off, new), "equation"))
    for f in lay.commitments:                                           # one commitment alone: the relation between them no longer holds
        for how in POINT_MUTATIONS:
            new = mutate_point(env[f.off:f.off + 32], how)
            if new != env[f.off:f.off + 32]:
                out.append(Forgery("%s:%s" % (f.name, how), _put(env, f.off, new), "rule"))
    return out


def transplant_forgeries(env, donor=None):
    """Whole proofs moved to where they do not belong, commitments moved consistently, and the digest of a consistency envelope.
    donor: another valid envelope of the same scheme, width and bounds (and k) for another value."""
    lay = layout(env)
    out = []
    if lay.scheme == 1:
        (_, o0, l0), (_, o1, l1) = lay.proofs
        assert l0 == l1
        out.append(Forgery("rp_min_and_rp_max_swapped", env[:o0] + env[o1:o1 + l1] + env[o0 + l0:o1] + env[o0:o0 + l0] + env[o1 + l1:], "equation"))
    if lay.scheme == 6 and len(lay.proofs) >= 2:
        (_, o0, l0), (_, o1, l1) = lay.proofs[:2]
        out.append(Forgery("rp1_and_rp2_swapped", env[:o0] + env[o1:o1 + l1] + env[o0 + l0:o1] + env[o0:o0 + l0] + env[o1 + l1:], "equation"))
    if donor is not None:
        dl = layout(donor)
        assert dl.scheme == lay.scheme and [p[1:] for p in dl.proofs] == [p[1:] for p in lay.proofs] and donor != env
        e = env
        for _, off, ln in lay.proofs:
            e = e[:off] + donor[off:off + ln] + e[off + ln:]
        out.append(Forgery("proofs_of_another_envelope", e, "equation"))
    for name, e in _shift_commitments(env, lay):
        out.append(Forgery(name, e, "equation"))
    if lay.scheme == 6:
        k = lay.extra["k"]
        d = lay.extra["digest"]
        out.append(Forgery("digest:plus_1", _put(env, d, ((int.from_bytes(env[d:d + 32], "little") + 1) % 2**256).to_bytes(32, "little")), "rule"))
        c0 = lay.commitments[0]                                         # a commitment moved and the digest recomputed: the difference commitments disagree
        if k > 1:
            out.append(Forgery("commit0:plus_B_with_digest", _redigest(_put(env, c0.off, mutate_point(env[c0.off:c0.off + 32], "plus_B")), lay), "rule"))
    return out


def forgeries(env, donor=None):
    return field_forgeries(env) + transplant_forgeries(env, donor)


def opposite_pairs(env):
    """Two copies of one envelope with the same point slot moved by +B in one and by -B in the other: under equal weights the two
    errors would cancel in a sum over the batch.  [(slot name, copy with +B, copy with -B)], both of stage "equation"."""
    lay = layout(env)
    first = lay.proofs[0][0] + "."
    last_r = max(f.name for f in lay.proof_fields if f.name.startswith(first + "R"))
    slots = [first + n for n in ("A", "S", "T1", "T2", "L0")] + [last_r]
    out = []
    for f in lay.proof_fields:
        if f.name in slots:
            cur = env[f.off:f.off + 32]
            out.append((f.name, _put(env, f.off, mutate_point(cur, "plus_B")), _put(env, f.off, mutate_point(cur, "minus_B"))))
    assert len(out) == len(slots)
    return out


def _undecodable(enc):
    """The next canonical, non-negative field element after `enc` that is not the encoding of a point."""
    s = int.from_bytes(enc, "little")
    while True:
        s = (s + 2) % FIELD_P
        if s % 2 == 0 and R.decode(s.to_bytes(32, "little")) is None:
            return s.to_bytes(32, "little")


def excluded(env):
    """Envelopes that parsing or decoding must remove: [(name, envelope)].  Every scalar field with s + l (not canonical), every point
    field (commitments included) with an encoding off the curve, with s + p and with bit 255 set (not canonical)."""
    lay = layout(env)
    out = []
    for f in lay.proof_fields + lay.commitments:
        cur = env[f.off:f.off + 32]
        s = int.from_bytes(cur, "little")
        if f.kind == "scalar":
            out.append((f.name + ":plus_l", _put(env, f.off, (s + L).to_bytes(32, "little"))))
        else:
            out.append((f.name + ":off_curve", _put(env, f.off, _undecodable(cur))))
            out.append((f.name + ":plus_p", _put(env, f.off, (s + FIELD_P).to_bytes(32, "little"))))
            out.append((f.name + ":bit_255", _put(env, f.off, (s | 1 << 255).to_bytes(32, "little"))))
    return out


def well_formed(env):
    """The framing parses, every point field decodes and every scalar field is canonical."""
    wire = to_wire(env)
    if bp._unwire(wire) is None:
        return False
    lay = layout(env)
    for f in lay.proof_fields + lay.commitments:
        cur = env[f.off:f.off + 32]
        if f.kind == "point" and R.decode(cur) is None:
            return False
        if f.kind == "scalar" and R.scalar_from_canonical_bytes(cur) is None:
            return False
    return True


def python_verify(env, *bounds):
    wire = to_wire(env)
    if env[1] == 1:
        return bp.verify_range_with_bounds_bits(wire, *bounds)
    if env[1] == 3:
        return bp.verify_threshold(wire, *bounds)
    return bp.verify_consistency(wire)


def rejection_stage(env, *bounds):
    """Where the Python oracle refuses the envelope: "accepted", "equation" (inside verify_single, after it evaluated a verification
    equation) or "rule" (anything before: framing, commitment relations, decoding, canonicity, identity points)."""
    calls = []                                                          # per verify_single call: [equations evaluated, verdict]
    real_single, real_msm = bp.verify_single, R.msm

    def single(*a, **kw):
        calls.append([0, None])
        calls[-1][1] = real_single(*a, **kw)
        return calls[-1][1]

    def msm(*a, **kw):
        if calls and calls[-1][1] is None:
            calls[-1][0] += 1
        return real_msm(*a, **kw)
    bp.verify_single, R.msm = single, msm
    try:
        ok = python_verify(env, *bounds)
    finally:
        bp.verify_single, R.msm = real_single, real_msm
    if ok:
        return "accepted"
    failed = [c for c in calls if c[1] is False]
    return "equation" if failed and failed[0][0] > 0 else "rule"


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def c_verify(oracle_c, env, *bounds):
    """The C oracle's verdict on one envelope (range: through its batch entry point)."""
    if env[1] == 1:                                                     # the batch entry point, one envelope
        buf = np.frombuffer(env, dtype=np.uint8).reshape(1, -1).copy()
        lens = np.array([len(env)], dtype=np.uint32)
        mn, mx = (np.array([b], dtype=np.uint64) for b in bounds)
        ok = np.zeros(1, dtype=np.uint8)
        allok = oracle_c.zkp_oracle_verify_range_batch(ctypes.c_uint64(1), _ptr(buf), ctypes.c_uint64(len(env)), _ptr(lens), _ptr(mn), _ptr(mx), _ptr(ok), 1)
        assert allok == int(ok[0])
        return bool(ok[0])
    if env[1] == 3:
        return bool(oracle_c.zkp_oracle_verify_threshold(env, ctypes.c_uint32(len(env)), ctypes.c_uint64(bounds[0])))
    return bool(oracle_c.zkp_oracle_verify_consistency(env, ctypes.c_uint32(len(env))))
