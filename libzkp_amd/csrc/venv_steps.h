// One verify call for a mixed envelope list (include/libzkp_hip_verify.h): n envelopes of any scheme, packed back to back -- envelope i is
// blob[off[i] .. off[i + 1]), the form zkp_hip_process_batch writes -- are sorted into per-scheme rows on the device and go through the
// library's own verifier cores (bpv_impl.inc, g16_impl.inc, stark_impl.inc), one scheme after the other on the shard's stream.  What is here
// is the glue around those cores, per-lane step functions shared by the kernels (venv_impl.inc: k_venv_*) and the host build of
// tests/emul/emul_verify_mixed.cpp:
//
//   classify  lane = envelope   verify_single_proof's checks up to the cryptographic one (performance.rs:270-293: Proof::from_bytes, the
//                               version, the expected scheme, verify_proof_cryptographic's pre-checks) with byte loads from the blob; one
//                               32-byte record per envelope -- the only per-envelope data the host reads
//   plan      host              rows per scheme in envelope order, a stride per scheme (ve_plan)
//   unpack    wave = envelope   blob -> row: aligned dword stores assembled from aligned source dwords, head and tail by bytes
//   apply     lane = envelope   row verdicts back to the caller's order; an envelope without a row gets 0
#pragma once
#include "zkp_common.h"
#include "batch_self_check.h"

namespace zkp {

constexpr uint64_t VE_MAX_TOTAL = 1ull << 20, VE_MAX_PAYLOAD = 900ull * 1024, VE_MAX_COMMITMENT = 256;      // utils/limits.rs
constexpr uint32_t VE_HEADER = 10, VE_VERSION = 2;
constexpr uint32_t VE_RANGE_PROOF_BYTES = 672;          // one 64-bit range proof inside a consistency envelope (bp_steps.h: RP_BYTES; venv_impl.inc asserts that they agree)
constexpr uint64_t VE_MAX_ROW_BYTES = 1ull << 32;       // rows of one scheme in one call

// what k_venv_classify leaves per envelope
struct VenvRecord {
    uint32_t scheme;        // 1..6: the envelope goes to that scheme's verifier; 0: rejected here
    uint32_t len;           // off[i + 1] - off[i] (0 for offsets that run backwards or leave the blob; 0xffffffff for anything longer)
    uint64_t p0, p1;        // range: min, max; threshold: the threshold; improvement: the old value; 0 otherwise
    uint32_t jobs;          // consistency: the k - 1 range proofs its k field announces (ve_consistency_jobs); 0 otherwise
    uint32_t reserved;
};
static_assert(sizeof(VenvRecord) == 32, "one 32-byte record per envelope");

ZKP_HD inline uint64_t ve_le(const uint8_t* p, uint32_t nbytes) {
    uint64_t x = 0;
    for (uint32_t b = 0; b < nbytes; b++) x |= (uint64_t)p[b] << (8 * b);
    return x;
}
// Jobs of a consistency envelope of `len` bytes, read from its own k field: k - 1 range proofs, 0 for an envelope whose length cannot hold
// what k announces (the device step of the verifier rejects it).  One copy for zkp_hip_verify_consistency_batch and k_venv_classify.
ZKP_HD inline uint32_t ve_consistency_jobs(const uint8_t* env, uint64_t len) {
    if (len < 14) return 0;
    const uint64_t k = ve_le(env + 10, 4);
    const bool fits = k >= 1 && k < (1u << 20) && 10 + 4 + 32 * k + (uint64_t)(4 + VE_RANGE_PROOF_BYTES + 32) * (k - 1) + 32 <= len;
    return fits ? (uint32_t)(k - 1) : 0u;
}
// the largest stride of a scheme's rows: what the per-scheme Python front ends cap theirs at.  A longer envelope keeps its recorded length
// and is rejected by the verifier (every one of them refuses a length beyond the stride).
ZKP_HD inline uint64_t ve_stride_cap(uint32_t scheme) { return scheme == 6 ? (1ull << 20) : scheme == 5 ? 8192u : 4096u; }

// Envelope i of n.  expect: nullptr, or per envelope 0 ("any") or the scheme it must have; any other value rejects.
// Only bytes of [off[0], off[n]) are read, and only those of envelope i.
ZKP_HD inline VenvRecord step_venv_classify(const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint64_t n, uint64_t i) {
    VenvRecord r{0, 0, 0, 0, 0, 0};
    const uint64_t lo = off[i], hi = off[i + 1];
    if (hi < lo || lo < off[0] || hi > off[n]) return r;          // offsets that run backwards, or an envelope outside the blob
    const uint64_t len = hi - lo;
    r.len = len > 0xffffffffull ? 0xffffffffu : (uint32_t)len;
    if (len < VE_HEADER || len > VE_MAX_TOTAL) return r;            // Proof::from_bytes (proof/mod.rs:38-85)
    const uint8_t* e = blob + lo;
    const uint64_t plen = ve_le(e + 2, 4), clen = ve_le(e + 6, 4);
    if (plen > VE_MAX_PAYLOAD || clen > VE_MAX_COMMITMENT || len != VE_HEADER + plen + clen) return r;
    if (e[0] != VE_VERSION) return r;
    const uint32_t s = e[1];
    if (expect && expect[i] != 0 && expect[i] != s) return r;
    const uint8_t* p = e + VE_HEADER;
    bool live = false;                                              // verify_proof_cryptographic's pre-checks (proof_helpers.rs:156-247)
    if (s == 1) {
        if (plen >= 20 && clen == 32) { r.p0 = ve_le(p, 8); r.p1 = ve_le(p + 8, 8); live = r.p0 <= r.p1; }
    } else if (s == 2) {
        live = clen == 32;
    } else if (s == 3) {
        if (plen >= 12 && clen == 32) { r.p0 = ve_le(p, 8); live = true; }
    } else if (s == 4) {
        if (clen == 32 && plen >= 4) { const uint64_t count = ve_le(p, 4); live = count >= 1 && count <= G16_MAX_SET && plen > 4 + 8 * count; }
    } else if (s == 5) {
        if (clen == 32 && plen >= 16) { r.p0 = ve_le(p, 8); live = true; }
    } else if (s == 6) {
        r.jobs = ve_consistency_jobs(e, len); live = true;
    }
    if (!live) { r.p0 = 0; r.p1 = 0; return r; }
    r.scheme = s;
    return r;
}

// The rows of one call (the SelfCheckView conventions: a scheme's rows are consecutive in the row arrays and start at a multiple of
// SC_ROW_ALIGN; its envelopes lie `stride` bytes apart from `base` in the row buffer).
struct VenvPlan {
    uint32_t rows[SC_KINDS], row0[SC_KINDS];
    uint64_t stride[SC_KINDS], base[SC_KINDS];
    uint32_t total_rows;          // length of the row arrays
    uint32_t live;                // envelopes that got a row
    uint64_t bytes;               // of the row buffer
};
constexpr uint64_t VE_BASE_ALIGN = 256;
// Rows per scheme in envelope order; stride = the longest live envelope of the scheme (at least 16), capped by ve_stride_cap.
// op_row[i] = the envelope's index in the row arrays, or SC_NO_ROW.  Returns 0, or the scheme whose rows would exceed VE_MAX_ROW_BYTES
// (nothing is allocated from a plan that fails).
ZKP_HD inline uint32_t ve_plan(uint64_t n, const VenvRecord* rec, uint32_t* op_row, VenvPlan& P) {
    uint64_t longest[SC_KINDS];
    for (uint32_t k = 0; k < SC_KINDS; k++) { P.rows[k] = 0; P.row0[k] = 0; P.stride[k] = 0; P.base[k] = 0; longest[k] = 0; }
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t s = rec[i].scheme;
        if (s == 0 || s >= SC_KINDS) continue;
        P.rows[s]++;
        if (rec[i].len > longest[s]) longest[s] = rec[i].len;
    }
    uint32_t next_row = 0; uint64_t next_byte = 0; uint32_t live = 0;
    for (uint32_t k = 1; k < SC_KINDS; k++) {
        if (!P.rows[k]) continue;
        const uint64_t cap = ve_stride_cap(k), want = longest[k] < 16 ? 16 : longest[k];
        P.stride[k] = want < cap ? want : cap;
        if (P.stride[k] * P.rows[k] > VE_MAX_ROW_BYTES) return k;
        P.row0[k] = next_row; P.base[k] = next_byte;
        next_row = (next_row + P.rows[k] + SC_ROW_ALIGN - 1) / SC_ROW_ALIGN * SC_ROW_ALIGN;
        next_byte = (next_byte + P.stride[k] * P.rows[k] + VE_BASE_ALIGN - 1) / VE_BASE_ALIGN * VE_BASE_ALIGN;
        live += P.rows[k];
    }
    P.total_rows = next_row; P.bytes = next_byte; P.live = live;
    uint32_t taken[SC_KINDS];
    for (uint32_t k = 0; k < SC_KINDS; k++) taken[k] = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t s = rec[i].scheme;
        op_row[i] = (s == 0 || s >= SC_KINDS) ? SC_NO_ROW : P.row0[s] + taken[s]++;
    }
    return 0;
}

// what the unpack and apply kernels see of a plan
struct VenvView {
    uint64_t n;
    const uint8_t* blob; const uint64_t* off;
    const VenvRecord* rec; const uint32_t* op_row;
    uint32_t row0[SC_KINDS]; uint64_t stride[SC_KINDS], base[SC_KINDS];
    uint8_t* rows;                                            // the row buffer
    uint32_t* row_len; uint64_t* row_p0; uint64_t* row_p1;    // [total_rows] lens / mins or thresholds or olds / maxs, as the verifier cores take them
    uint8_t* row_ok;                                          // [total_rows] their verdicts
};

ZKP_HD inline uint32_t ve_load_u32(const uint8_t* p) {          // p is 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t*>(p);
#else
    return (uint32_t)ve_le(p, 4);
#endif
}
ZKP_HD inline void ve_store_u32(uint8_t* p, uint32_t w) {       // p is 4-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint32_t*>(p) = w;
#else
    p[0] = (uint8_t)w; p[1] = (uint8_t)(w >> 8); p[2] = (uint8_t)(w >> 16); p[3] = (uint8_t)(w >> 24);
#endif
}
// Lane `lane` of `lanes` copies its share of src[0 .. len) to dst[0 .. len).  Bytes up to the first 4-byte boundary of dst and behind the
// last go one byte per lane; in between every lane stores aligned dwords, each assembled from the two aligned source dwords that hold
// its bytes (a byte funnel shift) when both lie inside [lo, hi), the readable bytes of the blob, and from four byte loads at its edges.
// Nothing outside src[0 .. len) is read unless it lies inside [lo, hi); nothing outside dst[0 .. len) is written.
ZKP_HD inline void step_venv_copy(uint8_t* dst, const uint8_t* src, uint32_t len, const uint8_t* lo, const uint8_t* hi, uint32_t lane, uint32_t lanes) {
    uint32_t head = (uint32_t)((4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u);
    if (head > len) head = len;
    const uint32_t body = (len - head) / 4, tail = (len - head) & 3u;
    for (uint32_t b = lane; b < head; b += lanes) dst[b] = src[b];
    const uint32_t sh = (uint32_t)((uintptr_t)(src + head) & 3u);
    for (uint32_t j = lane; j < body; j += lanes) {
        const uint8_t* s = src + head + 4ull * j;
        uint32_t w;
        if (sh == 0) w = ve_load_u32(s);
        else if (s - sh >= lo && s - sh + 8 <= hi) {
            const uint32_t w0 = ve_load_u32(s - sh), w1 = ve_load_u32(s - sh + 4);
            w = (w0 >> (8 * sh)) | (w1 << (32 - 8 * sh));
        } else w = (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
        ve_store_u32(dst + head + 4ull * j, w);
    }
    for (uint32_t b = lane; b < tail; b += lanes) { const uint32_t at = head + 4 * body + b; dst[at] = src[at]; }
}
// envelope i -> its row: the bytes (as many as the stride holds; the recorded length stays), and from lane 0 the row's length and parameters
ZKP_HD inline void step_venv_unpack(const VenvView& V, uint64_t i, uint32_t lane, uint32_t lanes) {
    const uint32_t g = V.op_row[i];
    if (g == SC_NO_ROW) return;
    const VenvRecord r = V.rec[i];
    uint64_t base = 0, stride = 0; uint32_t row0 = 0;
    ZKP_UNROLL for (uint32_t k = 1; k < SC_KINDS; k++) if (r.scheme == k) { base = V.base[k]; stride = V.stride[k]; row0 = V.row0[k]; }
    const uint32_t take = r.len <= stride ? r.len : (uint32_t)stride;
    step_venv_copy(V.rows + base + stride * (g - row0), V.blob + V.off[i], take, V.blob + V.off[0], V.blob + V.off[V.n], lane, lanes);
    if (lane == 0) { V.row_len[g] = r.len; V.row_p0[g] = r.p0; V.row_p1[g] = r.p1; }
}
ZKP_HD inline uint8_t step_venv_apply(const VenvView& V, uint64_t i) {
    const uint32_t g = V.op_row[i];
    return g == SC_NO_ROW ? (uint8_t)0 : (uint8_t)(V.row_ok[g] == 1);
}

// Weight of an envelope in the plan that cuts a host call over the registered shards (verify_shards.h), from a host peek at its scheme byte:
// a range envelope 2 jobs, a consistency envelope its k - 1, everything else 1 (vs_prefix counts a zero as 1).  The rule itself, for an
// envelope of `len` bytes at `env` whose scheme byte the caller has read (a container's inner envelope: composite_impl.inc):
ZKP_HD inline uint32_t ve_scheme_weight(uint8_t scheme, const uint8_t* env, uint64_t len) { return scheme == 1 ? 2u : scheme == 6 ? ve_consistency_jobs(env, len) : 1u; }
// ... and for envelope i of a packed list, 1 when its offsets run backwards, leave the blob or span no scheme byte
ZKP_HD inline uint32_t ve_weight(const uint8_t* blob, const uint64_t* off, uint64_t n, uint64_t i) {
    const uint64_t lo = off[i], hi = off[i + 1];
    if (hi < lo || lo < off[0] || hi > off[n] || hi - lo < 2) return 1;
    return ve_scheme_weight(blob[lo + 1], blob + lo, hi - lo);
}

}  // namespace zkp
