// Sealing a list of composite proofs in one call (include/libzkp_hip_seal.h): the issuer's half of composite_steps.h.  n containers are
// framed and hashed from a packed envelope list -- envelope e is env[env_off[e] .. env_off[e + 1]), container i takes the envelopes
// first[i] .. first[i + 1] and the metadata run meta[meta_off[i] .. meta_off[i + 1]), already in wire form.  The division of work:
//
//   plan      host              one pass over the envelopes' lengths and "Proof::from_bytes accepts it" codes, the `first` array and the
//                               metadata runs (seal_plan): a status per container, out_off, and per sealed container a record -- where it
//                               goes, what it holds, where its digest lies, how many bytes the digest covers, its metadata entries'
//                               offsets in hash order (relative to the container's first byte, as the digest lane reads the framed
//                               container).  Every size is known here, before any device work.
//   frame     wave = piece      every byte of every sealed container except the digest (step_seal_frame).  A piece is an inner proof with
//                               its 4-byte length prefix -- the first one of a container carries the 12-byte header too -- or a
//                               container's metadata run.  Bulk bytes go through step_venv_copy (aligned dword stores inside the piece,
//                               byte stores at its two edges), headers and prefixes as byte stores: every output byte has exactly one
//                               writing wave, and no wave stores a dword that holds a byte of another piece.
//   seal      lane = container  step_comp_digest over the container the frame step has just written; the eight state words go out
//                               big-endian at digest_at (step_seal_digest)
//
// The step functions and the plan are shared by the kernels (composite_seal_impl.inc: k_comp_frame, k_comp_seal) and the host build of
// tests/emul/emul_composites_seal.cpp.
#pragma once
#include "composite_steps.h"

namespace zkp {

constexpr uint8_t SEAL_FAILED_OP = 0, SEAL_SEALED = 1, SEAL_REFUSED = 2, SEAL_UNREADABLE = 3;          // the statuses of the call (LIBZKP_SEAL_*)
constexpr uint8_t SEAL_ENV_REFUSED = 0, SEAL_ENV_ACCEPTED = 1, SEAL_ENV_FAILED_OP = 2;                   // what the plan is told per envelope
constexpr uint64_t SEAL_MAX_ITEMS = 1ull << 22;                                                          // containers, and envelopes, of one call

// Envelope [lo, hi) of a blob whose readable bytes are [blob_lo, blob_hi): Proof::from_bytes' verdict from its length and ten header bytes
inline uint8_t seal_env_code(const uint8_t* blob, uint64_t lo, uint64_t hi, uint64_t blob_lo, uint64_t blob_hi) {
    if (hi < lo || lo < blob_lo || hi > blob_hi) return SEAL_ENV_REFUSED;
    return cp_proof_accepts(blob + lo, hi - lo) ? SEAL_ENV_ACCEPTED : SEAL_ENV_REFUSED;
}

// What the plan leaves per sealed container
struct SealRecord {
    uint64_t out_base;      // its first byte in the output (= out_off[src])
    uint64_t env0;          // its first envelope
    uint64_t meta_src;      // its metadata run's first byte in the metadata blob
    uint64_t order0;        // its metadata entries' offsets are order[order0 .. order0 + nmeta), in hash order, relative to out_base
    uint32_t src;           // its index in the call
    uint32_t nproofs, meta_len, nmeta;
    uint32_t digest_at;     // offset of the 32 digest bytes (= length - 32)
    uint32_t hashed;        // bytes the digest covers, the 20-byte prefix included
};
struct SealPlan {
    std::vector<uint8_t> status;          // [n]
    std::vector<uint64_t> out_off;        // [n + 1]: a container that is not sealed takes zero bytes
    std::vector<SealRecord> rec;          // sealed containers, in container order
    std::vector<uint32_t> order;
    uint64_t envelopes = 0;               // inner proofs of the sealed containers
};

// env_off: n_env + 1 offsets (an envelope's length is only read when its code is SEAL_ENV_ACCEPTED); first: n + 1 entries, not decreasing,
// within [0, n_env] (the caller has checked that); meta / meta_off: both null, or n + 1 offsets that do not decrease.
inline void seal_plan(uint64_t n, const uint64_t* env_off, const uint8_t* env_code, const uint64_t* first, const uint8_t* meta, const uint64_t* meta_off, SealPlan& P) {
    P.status.assign(n, SEAL_REFUSED); P.out_off.assign(n + 1, 0); P.rec.clear(); P.order.clear(); P.envelopes = 0;
    uint64_t total = 0;
    std::vector<CpMetaEntry> entries;
    for (uint64_t i = 0; i < n; i++) {
        P.out_off[i] = total;
        const uint64_t e0 = first[i], e1 = first[i + 1];
        bool failed = false, refused = e0 == e1;                    // an empty proof list: create_composite_proof returns Err (advanced/composite.rs:11-15)
        for (uint64_t e = e0; e < e1; e++) { failed = failed || env_code[e] == SEAL_ENV_FAILED_OP; refused = refused || env_code[e] == SEAL_ENV_REFUSED; }
        if (failed) { P.status[i] = SEAL_FAILED_OP; continue; }
        if (refused) { P.status[i] = SEAL_REFUSED; continue; }
        // from here on the reference writes the container; what CompositeProof::from_bytes would refuse to read back is not sealed
        P.status[i] = SEAL_UNREADABLE;
        const uint64_t nproofs = e1 - e0;
        if (nproofs > CP_MAX_ITEMS) continue;
        uint64_t proof_bytes = 0;
        for (uint64_t e = e0; e < e1; e++) proof_bytes += env_off[e + 1] - env_off[e];          // (<= 1000 x 1 MiB)
        const uint64_t mlen = meta_off ? meta_off[i + 1] - meta_off[i] : 0;
        const uint64_t meta_at = CP_MIN_BYTES + 4 * nproofs + proof_bytes, len = meta_at + mlen + CP_DIGEST_BYTES;
        if (mlen > CP_MAX_BYTES || len > CP_MAX_BYTES) continue;
        const uint8_t* m = mlen ? meta + meta_off[i] : nullptr;
        entries.clear();
        uint64_t at = 0; bool readable = true;
        while (readable && at < mlen) {                              // a run that is truncated or has bytes left over stops here
            CpMetaEntry E;
            readable = entries.size() < CP_MAX_ITEMS && cp_meta_entry(m, mlen, at, (uint32_t)entries.size(), E);
            if (readable) entries.push_back(E);
        }
        if (!readable) continue;
        cp_meta_sort(m, entries);
        for (size_t k = 0; readable && k + 1 < entries.size(); k++) readable = !cp_meta_same_key(m, entries[k], entries[k + 1]);      // a key that occurs twice
        if (!readable) continue;
        SealRecord R{total, e0, meta_off ? meta_off[i] : 0, (uint64_t)P.order.size(), (uint32_t)i, (uint32_t)nproofs, (uint32_t)mlen, (uint32_t)entries.size(),
                     (uint32_t)(meta_at + mlen), (uint32_t)(CP_PREFIX_BYTES + proof_bytes + mlen)};
        for (const CpMetaEntry& E : entries) P.order.push_back((uint32_t)(meta_at + E.at));
        P.rec.push_back(R); P.status[i] = SEAL_SEALED; P.envelopes += nproofs;
        total += len;
    }
    P.out_off[n] = total;
}

// One wave's work of the frame step (32 bytes)
constexpr uint32_t SEAL_PIECE_PROOF = 0, SEAL_PIECE_FIRST_PROOF = 1, SEAL_PIECE_META = 2;
struct SealPiece {
    uint64_t dst;           // the piece's first byte in the output
    uint64_t src;           // its source bytes: an offset into the envelope blob, or into the metadata blob
    uint32_t len;           // source bytes
    uint32_t kind;          // _PROOF: u32 len | bytes; _FIRST_PROOF: "COMP" | u32 nproofs | u32 nmeta | u32 len | bytes; _META: bytes
    uint32_t nproofs, nmeta;
};
static_assert(sizeof(SealPiece) == 32, "one 32-byte record per piece");
// The pieces of the sealed containers, and the digest lanes in the order k_comp_digest uses: hashed length, descending
inline void seal_pieces(const SealPlan& P, const uint64_t* env_off, std::vector<SealPiece>& pieces, std::vector<CompLane>& lanes) {
    pieces.clear(); lanes.clear();
    pieces.reserve(P.envelopes + P.rec.size()); lanes.reserve(P.rec.size());
    for (const SealRecord& R : P.rec) {
        uint64_t at = R.out_base;
        for (uint32_t k = 0; k < R.nproofs; k++) {
            const uint64_t e = R.env0 + k;
            const uint32_t len = (uint32_t)(env_off[e + 1] - env_off[e]);
            pieces.push_back(SealPiece{at, env_off[e], len, k == 0 ? SEAL_PIECE_FIRST_PROOF : SEAL_PIECE_PROOF, R.nproofs, R.nmeta});
            at += (k == 0 ? CP_MIN_BYTES : 0) + 4 + len;
        }
        if (R.meta_len) pieces.push_back(SealPiece{at, R.meta_src, R.meta_len, SEAL_PIECE_META, R.nproofs, R.nmeta});
        lanes.push_back(CompLane{R.out_base, R.order0, R.src, R.nproofs, R.nmeta, R.digest_at, R.hashed, 0});
    }
    std::stable_sort(lanes.begin(), lanes.end(), [](const CompLane& a, const CompLane& b) { return a.hashed > b.hashed; });
}

// Lane `lane` of `lanes` writes its share of piece S.  env / meta: the source blobs, readable over [env_lo, env_hi) / [meta_lo, meta_hi).
// Nothing outside the piece's source bytes is read unless it lies inside the readable range; nothing outside the piece is written.
ZKP_HD inline void step_seal_frame(uint8_t* out, const SealPiece& S, const uint8_t* env, const uint8_t* env_lo, const uint8_t* env_hi, const uint8_t* meta,
                                   const uint8_t* meta_lo, const uint8_t* meta_hi, uint32_t lane, uint32_t lanes) {
    uint8_t* dst = out + S.dst;
    if (S.kind == SEAL_PIECE_META) { step_venv_copy(dst, meta + S.src, S.len, meta_lo, meta_hi, lane, lanes); return; }
    const uint32_t head = S.kind == SEAL_PIECE_FIRST_PROOF ? 16u : 4u;
    for (uint32_t b = lane; b < head; b += lanes) {                 // header and length prefix: one byte per lane
        const uint32_t f = b + (16u - head);                         // the byte's place in "COMP" | nproofs | nmeta | len
        const uint32_t word = f < 4 ? 0x504d4f43u : f < 8 ? S.nproofs : f < 12 ? S.nmeta : S.len;
        dst[b] = (uint8_t)(word >> (8 * (f & 3u)));
    }
    step_venv_copy(dst + head, env + S.src, S.len, env_lo, env_hi, lane, lanes);
}

// The lane of one sealed container: its digest over the framed bytes, stored big-endian at digest_at.  [lo, hi): the output buffer.
ZKP_HD inline void step_seal_digest(uint8_t* out, const uint8_t* lo, const uint8_t* hi, const CompLane& L, const uint32_t* order) {
    uint32_t h[8];
    (void)step_comp_digest(out, lo, hi, L, order, h);               // (the comparison with the bytes that lie at digest_at means nothing here)
    uint8_t* d = out + L.base + L.digest_at;
    ZKP_UNROLL for (int k = 0; k < 8; k++) { d[4 * k] = (uint8_t)(h[k] >> 24); d[4 * k + 1] = (uint8_t)(h[k] >> 16); d[4 * k + 2] = (uint8_t)(h[k] >> 8); d[4 * k + 3] = (uint8_t)h[k]; }
}

}  // namespace zkp
