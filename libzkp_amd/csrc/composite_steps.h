// One verify call for a list of composite proofs (include/libzkp_hip_composites.h): "COMP" containers
// (/root/reference/src/utils/composition.rs:113-331) packed back to back -- container i is blob[off[i] .. off[i + 1]).  The division of work:
//
//   walk      host              one pass over a container's framing (comp_walk): every Err branch of CompositeProof::from_bytes except the
//                               digest comparison, from the length fields, the ten header bytes of each inner proof and the metadata keys;
//                               the metadata entries' offsets in hash order (bytewise-ascending keys, a repeated key counted once with its
//                               last value, as HashMap::insert leaves it).  Nanoseconds per item; the framing is not parsed on the device.
//   digest    lane = container  SHA-256 over "COMPOSITE_PROOF:" | u32 proof count | the inner proofs without their length prefixes | the
//                               metadata entries as they are serialized, in the host's order -- a virtual byte stream over scattered segments
//                               of the blob, compressed 64 bytes at a time (step_comp_digest; a block that lies inside one segment is
//                               fetched at once, anything else word by word), compared with the container's digest
//   pack      wave = envelope   the inner envelopes of the containers that stand -> the packed (blob, off) form of the mixed verifier
//                               (step_venv_copy), which then runs unchanged (venv_impl.inc: verify_envelopes_core)
//   fold      lane = container  a container's envelope verdicts ANDed into its status (step_comp_fold)
//
// The step functions are shared by the kernels (composite_impl.inc: k_comp_*) and the host build of tests/emul/emul_composites.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "sha256_dev.h"
#include "venv_steps.h"

namespace zkp {

constexpr uint64_t CP_MAX_BYTES = 4ull << 20, CP_MIN_BYTES = 12, CP_MAX_ITEMS = 1000, CP_MAX_KEY = 1024, CP_MAX_VALUE = 65536;      // composition.rs:31-40
constexpr uint32_t CP_DIGEST_BYTES = 32, CP_PREFIX_BYTES = 20;          // "COMPOSITE_PROOF:" and the u32 proof count: five words of the first block
constexpr uint8_t CP_ACCEPTED = 1, CP_REJECTED = 0, CP_MALFORMED = 2;   // the statuses of the call

// What the walk leaves per container.  Offsets are relative to the container's first byte.
struct CompWalk {
    uint8_t ok;             // 1: every rule of from_bytes but the digest comparison holds; 0: malformed (nothing else is meaningful)
    uint32_t nproofs;       // inner proofs; the first one's length prefix is at offset 12
    uint32_t nmeta;         // metadata entries that are hashed (after de-duplication)
    uint64_t order0;        // their offsets are order[order0 .. order0 + nmeta), in hash order
    uint32_t digest_at;     // offset of the 32 digest bytes (= length - 32)
    uint32_t hashed;        // bytes the digest covers, the 20-byte prefix included
    uint64_t proof_bytes;   // the inner proofs' bytes, without prefixes
};

// String::from_utf8's verdict on s[0 .. n) (core::str::validations: no overlong forms, no surrogates, nothing above U+10FFFF, no truncated sequence)
inline bool cp_utf8_ok(const uint8_t* s, uint32_t n) {
    auto cont = [&](uint32_t at, uint8_t lo, uint8_t hi) { return at < n && s[at] >= lo && s[at] <= hi; };
    for (uint32_t i = 0; i < n;) {
        const uint8_t b = s[i];
        if (b < 0x80) { i += 1; continue; }
        if (b >= 0xC2 && b <= 0xDF) { if (!cont(i + 1, 0x80, 0xBF)) return false; i += 2; continue; }
        if (b >= 0xE0 && b <= 0xEF) {
            const uint8_t lo = b == 0xE0 ? 0xA0 : 0x80, hi = b == 0xED ? 0x9F : 0xBF;
            if (!cont(i + 1, lo, hi) || !cont(i + 2, 0x80, 0xBF)) return false;
            i += 3; continue;
        }
        if (b >= 0xF0 && b <= 0xF4) {
            const uint8_t lo = b == 0xF0 ? 0x90 : 0x80, hi = b == 0xF4 ? 0x8F : 0xBF;
            if (!cont(i + 1, lo, hi) || !cont(i + 2, 0x80, 0xBF) || !cont(i + 3, 0x80, 0xBF)) return false;
            i += 4; continue;
        }
        return false;          // a continuation byte first, C0 / C1, F5..FF
    }
    return true;
}

// Proof::from_bytes' verdict on an inner proof of n bytes, from n and its ten header bytes at p (proof/mod.rs:38-85).  p is read only when
// n >= VE_HEADER.  One copy for the walk below and for the sealing plan (composite_seal.h).
inline bool cp_proof_accepts(const uint8_t* p, uint64_t n) {
    if (n > VE_MAX_TOTAL || n < VE_HEADER) return false;
    const uint64_t plen = ve_le(p + 2, 4), clen = ve_le(p + 6, 4);
    return !(plen > VE_MAX_PAYLOAD || clen > VE_MAX_COMMITMENT || n != VE_HEADER + plen + clen);
}
// One metadata entry of c[0 .. len) at offset `at`, as from_bytes judges it: the key's length and UTF-8, the value's length, and that
// every field lies inside len.  On true E describes it and `at` is behind it.  One copy for the walk and the sealing plan.
struct CpMetaEntry { uint32_t at, klen, index, bytes; };
inline bool cp_meta_entry(const uint8_t* c, uint64_t len, uint64_t& at, uint32_t index, CpMetaEntry& E) {
    if (at + 4 > len) return false;
    const uint64_t kl = ve_le(c + at, 4);
    if (kl > CP_MAX_KEY || at + 4 + kl > len) return false;
    if (!cp_utf8_ok(c + at + 4, (uint32_t)kl)) return false;
    if (at + 4 + kl + 4 > len) return false;
    const uint64_t vl = ve_le(c + at + 4 + kl, 4);
    if (vl > CP_MAX_VALUE || at + 8 + kl + vl > len) return false;
    E = CpMetaEntry{(uint32_t)at, (uint32_t)kl, index, (uint32_t)(8 + kl + vl)};
    at += 8 + kl + vl;
    return true;
}
// hash order: keys ascending bytewise (a key that is a prefix of another comes first); equal keys in the order they were written
inline void cp_meta_sort(const uint8_t* c, std::vector<CpMetaEntry>& entries) {
    std::sort(entries.begin(), entries.end(), [&](const CpMetaEntry& a, const CpMetaEntry& b) {
        const uint32_t m = a.klen < b.klen ? a.klen : b.klen;
        const int d = m ? memcmp(c + a.at + 4, c + b.at + 4, m) : 0;
        if (d) return d < 0;
        if (a.klen != b.klen) return a.klen < b.klen;
        return a.index < b.index;
    });
}
inline bool cp_meta_same_key(const uint8_t* c, const CpMetaEntry& a, const CpMetaEntry& b) { return a.klen == b.klen && memcmp(c + a.at + 4, c + b.at + 4, a.klen) == 0; }

// Container [lo, hi) of a blob whose readable bytes are [blob_lo, blob_hi) (offsets into `blob`).  Appends the hashed metadata entries'
// offsets to `order`.  Reads the length fields, the ten header bytes of every inner proof and the metadata keys, nothing else.
inline CompWalk comp_walk(const uint8_t* blob, uint64_t lo, uint64_t hi, uint64_t blob_lo, uint64_t blob_hi, std::vector<uint32_t>& order) {
    CompWalk W{0, 0, 0, (uint64_t)order.size(), 0, 0, 0};
    if (hi < lo || lo < blob_lo || hi > blob_hi) return W;          // offsets that run backwards or leave the blob
    const uint64_t len = hi - lo;
    if (len > CP_MAX_BYTES || len < CP_MIN_BYTES) return W;
    const uint8_t* c = blob + lo;
    if (memcmp(c, "COMP", 4) != 0) return W;
    const uint64_t nproofs = ve_le(c + 4, 4), nmeta = ve_le(c + 8, 4);
    if (nproofs > CP_MAX_ITEMS || nmeta > CP_MAX_ITEMS) return W;
    uint64_t at = 12, proof_bytes = 0;
    for (uint64_t k = 0; k < nproofs; k++) {
        if (at + 4 > len) return W;
        const uint64_t n = ve_le(c + at, 4); at += 4;
        if (at + n > len) return W;
        if (!cp_proof_accepts(c + at, n)) return W;                 // Proof::from_bytes (proof/mod.rs:38-85)
        at += n; proof_bytes += n;
    }
    std::vector<CpMetaEntry> entries; entries.reserve(nmeta);
    for (uint64_t k = 0; k < nmeta; k++) {
        CpMetaEntry e;
        if (!cp_meta_entry(c, len, at, (uint32_t)k, e)) return W;
        entries.push_back(e);
    }
    if (at + CP_DIGEST_BYTES != len) return W;                      // digest missing, or bytes behind it
    // hash order: keys ascending bytewise (a key that is a prefix of another comes first); of equal keys the last one stands
    cp_meta_sort(c, entries);
    uint64_t meta_bytes = 0; uint32_t kept = 0;
    for (size_t k = 0; k < entries.size(); k++) {
        const CpMetaEntry& e = entries[k];
        if (k + 1 < entries.size() && cp_meta_same_key(c, e, entries[k + 1])) continue;
        order.push_back(e.at); meta_bytes += e.bytes; kept++;
    }
    W.ok = 1; W.nproofs = (uint32_t)nproofs; W.nmeta = kept; W.digest_at = (uint32_t)at; W.proof_bytes = proof_bytes;
    W.hashed = (uint32_t)(CP_PREFIX_BYTES + proof_bytes + meta_bytes);          // (< 4 MiB + 20: every hashed byte lies in the container, once)
    return W;
}
// The inner envelopes of a container that comp_walk found well-formed (its first byte at blob[lo], W.nproofs of them), in order: f(at, len)
// for the envelope of `len` bytes at blob[at], behind its length prefix.  One copy for the fan-out weights and the pack lists (composite_impl.inc).
template <class F> inline void comp_each_envelope(const uint8_t* blob, uint64_t lo, uint32_t nproofs, F f) {
    uint64_t at = lo + 12;
    for (uint32_t k = 0; k < nproofs; k++) {
        const uint64_t len = ve_le(blob + at, 4);
        f(at + 4, len);
        at += 4 + len;
    }
}

// What a digest lane reads of its container (40 bytes)
struct CompLane {
    uint64_t base;          // the container's first byte, as an offset into the blob
    uint64_t order0;        // its hashed metadata entries: order[order0 .. order0 + nmeta)
    uint32_t src;           // the container's index in the call (where its verdict goes)
    uint32_t nproofs, nmeta, digest_at, hashed;
    uint32_t reserved;
};
static_assert(sizeof(CompLane) == 40, "one 40-byte record per digest lane");
inline CompLane comp_lane(const CompWalk& W, uint64_t base, uint64_t order0, uint32_t src) {
    return CompLane{base, order0, src, W.nproofs, W.nmeta, W.digest_at, W.hashed, 0};
}

ZKP_HD inline uint32_t cp_bswap(uint32_t w) { return (w << 24) | ((w & 0xff00u) << 8) | ((w >> 8) & 0xff00u) | (w >> 24); }

// The compression function on a rolling 16-word schedule, every index static after unrolling: state and schedule stay in registers.
// w[] is left holding the schedule's last sixteen words.
ZKP_HD inline void cp_sha256_compress(uint32_t h[8], uint32_t w[16]) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    ZKP_UNROLL for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const uint32_t w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const uint32_t s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3), s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
        }
        const uint32_t t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha256_k(i) + w[i & 15];
        const uint32_t t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g; g = f; f = e; e = d + t1; d = c; c = b; b = a; a = t1 + t2;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// The stream behind the 20-byte prefix: the inner proofs, walked by their own length prefixes (bounded by the host's walk), then the metadata
// entries in the host's order, then one 0x80 byte and zeros.  next() delivers four stream bytes as a big-endian word.
struct CompCursor {
    const uint8_t *lo, *hi;             // [lo, hi): the readable bytes of the blob
    const uint8_t* p;                   // the next byte of the current segment
    uint32_t seg_left;                  // bytes left in it
    const uint8_t* next_prefix;         // the next inner proof's length prefix
    uint32_t proofs_left, meta_left;
    const uint8_t* base;                // the container
    const uint32_t* order;              // the next metadata entry's offset
    uint32_t left;                      // data bytes left in the stream
    uint32_t padded;                    // the 0x80 byte has gone out

    ZKP_HD inline void open_segment() {
        if (proofs_left) {
            seg_left = (uint32_t)ve_le(next_prefix, 4);
            p = next_prefix + 4; next_prefix = p + seg_left; proofs_left--;
        } else if (meta_left) {
            p = base + *order++; meta_left--;
            const uint32_t kl = (uint32_t)ve_le(p, 4);
            seg_left = 8 + kl + (uint32_t)ve_le(p + 4 + kl, 4);
        } else left = 0;                 // (not reached: `left` is the segments' sum)
    }
    ZKP_HD inline uint32_t next() {
        if (seg_left >= 4) {             // (then left >= 4 too) the fast path: aligned dwords and a byte funnel
            const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
            const uint8_t* q = p - sh;
            uint32_t w; bool have = true;
            if (sh == 0) w = ve_load_u32(q);
            else if (q >= lo && q + 8 <= hi) { const uint32_t w0 = ve_load_u32(q), w1 = ve_load_u32(q + 4); w = (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh)); }
            else { w = 0; have = false; }          // at the blob's edge: by bytes, below
            if (have) { p += 4; seg_left -= 4; left -= 4; return cp_bswap(w); }
        }
        uint32_t w = 0;                  // a word that straddles a segment boundary, the blob's edge or the end of the stream
        for (uint32_t k = 0; k < 4; k++) {
            uint32_t byte = 0;
            while (left && !seg_left) open_segment();
            if (left) { byte = *p++; seg_left--; left--; }
            else if (!padded) { byte = 0x80; padded = 1; }
            w = (w << 8) | byte;
        }
        return w;
    }
    // A whole block from inside the current segment: seventeen aligned dwords in flight at once, then sixteen funnels -- one wait for
    // memory per block instead of one per word.  false (nothing consumed) when the block leaves the segment or the dwords the blob.
    ZKP_HD inline bool next_block(uint32_t w[16]) {
        const uint32_t sh = (uint32_t)((uintptr_t)p & 3u);
        const uint8_t* q = p - sh;
        if (seg_left < 64 || q < lo || q + 68 > hi) return false;
        uint32_t t[17];
        ZKP_UNROLL for (int i = 0; i < 17; i++) t[i] = ve_load_u32(q + 4 * i);
        ZKP_UNROLL for (int i = 0; i < 16; i++) w[i] = cp_bswap((uint32_t)((((uint64_t)t[i + 1] << 32) | t[i]) >> (8 * sh)));
        p += 64; seg_left -= 64; left -= 64;
        return true;
    }
};

// The lane of one container: its digest from the stream, compared with the 32 bytes at digest_at.  digest_out (may be null): the eight
// state words.  Reads only bytes of the container, and of [lo, hi) where an aligned dword reaches beyond a segment.
ZKP_HD inline bool step_comp_digest(const uint8_t* blob, const uint8_t* lo, const uint8_t* hi, const CompLane& L, const uint32_t* order, uint32_t* digest_out) {
    CompCursor C;
    C.lo = lo; C.hi = hi; C.base = blob + L.base;
    C.p = C.base; C.seg_left = 0; C.next_prefix = C.base + 12; C.proofs_left = L.nproofs; C.meta_left = L.nmeta;
    C.order = order + L.order0; C.left = L.hashed - CP_PREFIX_BYTES; C.padded = 0;
    uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
    const uint32_t blocks = (L.hashed + 9 + 63) / 64;
    uint32_t w[16];
    for (uint32_t b = 0; b < blocks; b++) {
        if (b == 0) {                    // "COMPOSITE_PROOF:" and the little-endian proof count
            w[0] = 0x434f4d50u; w[1] = 0x4f534954u; w[2] = 0x455f5052u; w[3] = 0x4f4f463au; w[4] = cp_bswap(L.nproofs);
            ZKP_UNROLL for (int i = 5; i < 16; i++) w[i] = C.next();
        } else if (!C.next_block(w)) {
            ZKP_UNROLL for (int i = 0; i < 16; i++) w[i] = C.next();
        }
        if (b + 1 == blocks) { w[14] = L.hashed >> 29; w[15] = L.hashed << 3; }      // (the stream has ended before byte 56 of the last block)
        cp_sha256_compress(h, w);
    }
    if (digest_out) for (int k = 0; k < 8; k++) digest_out[k] = h[k];
    const uint8_t* d = C.base + L.digest_at;
    uint32_t diff = 0;
    ZKP_UNROLL for (int k = 0; k < 8; k++) diff |= h[k] ^ (((uint32_t)d[4 * k] << 24) | ((uint32_t)d[4 * k + 1] << 16) | ((uint32_t)d[4 * k + 2] << 8) | d[4 * k + 3]);
    return diff == 0;
}

// Envelope e of the packed list: src[e] = its first byte in the blob, poff[e] .. poff[e + 1] = where it goes
ZKP_HD inline void step_comp_pack(uint8_t* packed, const uint64_t* poff, const uint8_t* blob, const uint64_t* src, const uint8_t* lo, const uint8_t* hi, uint64_t e, uint32_t lane, uint32_t lanes) {
    step_venv_copy(packed + poff[e], blob + src[e], (uint32_t)(poff[e + 1] - poff[e]), lo, hi, lane, lanes);
}
// Container c: accepted only while every one of its envelopes env0[c] .. env0[c + 1] is; a malformed container keeps its status
ZKP_HD inline uint8_t step_comp_fold(uint8_t status, const uint8_t* ok, const uint64_t* env0, uint64_t c) {
    if (status != CP_ACCEPTED) return status;
    for (uint64_t e = env0[c]; e < env0[c + 1]; e++) if (ok[e] != 1) return CP_REJECTED;
    return CP_ACCEPTED;
}

}  // namespace zkp
