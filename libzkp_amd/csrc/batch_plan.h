// The host plan of a staged batch (zkp_hip_batch_stage): which shard proves which op, what the host validates, how large every envelope is,
// and one shard's staging up to the upload -- the layout of its three device blocks and every byte of its staging image.  No HIP call and no
// HIP header: compiled into the library (batch_impl.inc: stage_shard = this plan + the pinned buffer, four pool takes and one upload) and for
// the host by tests/emul/emul_batch_plan.cpp.
//
// A shard's ops are the ops gidx[0 .. n) of the caller's list, ascending (plan_shards); kinds are 1..6 (check_ops refuses others).  A VARIANT
// is the shard's ops of one kind; the plan keeps one VariantPlan per kind, indexed by kind:
//   rows    equality, membership and improvement are validated here and get arena rows for their VALID ops only; every range, threshold and
//           consistency op has a row (range is validated on the device; the framing leaves a refused op's row empty).  Row r = the variant's
//           r-th such op in op order.
//   stride  bytes per row: range 1478, equality 298, threshold 762, improvement STARK_MAX_ENVELOPE; membership: the largest envelope over the
//           VALID ops (0 without one); consistency: the largest consistency_envelope_bytes(count ? count : 1) over ALL its ops.
//   arena   offset of row 0 in the arena block.
//   row0    flagged batches (ZKP_HIP_OP_SELF_CHECK) only: the variant's first row in the self-check's row arrays; kinds in ascending order,
//           every variant's share rounded up to a multiple of SC_ROW_ALIGN.
// max_total = the sum of op_max_bytes over the shard's ops, valid or not.
// Layout: every block is a sequence of regions taken in this order, each padded to 256 bytes (R, E, T, M, I, C: the variants' rows):
//   image  i_rv 8R | i_rmin 8R | i_rmax 8R | i_rseed 32R | i_ev 8E | i_eseed 32E | i_mv 8M | i_msets 8*64*M | i_mlen 4M | i_mseed 32M |
//          i_io 8I | i_in 8I | i_tseed 32T | i_cseed 32C | i_ccount 4C | i_clen 4C | i_src 8n | i_lenf 4n | i_dix 4n | i_dkind n | i_stf 4n
//          flagged: | i_thr 8T | i_var n | i_rlen 4*rows | i_rop 4*rows | i_rok rows | i_oprow 4n | i_cnt 8     (rows: all variants' padded shares)
//   arena  range | equality | membership | improvement | threshold | consistency (stride x rows each) | a_dlen 4(R + I) | a_dst 4R
//   meta   m_off 8(n + 1) | m_status 4n | m_len 4n
// Image: row r of a variant holds its op's inputs -- range a, b, c (value, min, max); equality a; membership a, the set padded with zeros to
// 64 slots, its length; improvement a, b (old, new) -- and, except for improvement, the op's SEED: the 32 bytes at seeds + 32 * (the op's index
// in the CALLER's list).  i_ccount / i_clen: every consistency row's count and framed length.  Per local op j, the pack view's table:
//   src        arena + stride * r; 0 for an op without a row
//   len_fixed  range, improvement: LEN_DYN (the device reports it); equality 298; membership its envelope size; threshold, consistency: the
//              framed length (0 when the framing refused the op); 0 for an op without a row
//   dyn_ix     range r; improvement R + r (a_dlen: the range lengths, then the improvement lengths); else 0
//   dyn_kind   range DYN_LEN_STATUS, improvement DYN_LEN_ONLY, else DYN_NONE
//   status     ZKP_HIP_OK, or ZKP_HIP_INVALID_INPUT for an op refused here or by its framing
// Flagged: i_thr = every threshold row's threshold, i_var = op_variant; the other five regions are written on the device.  No other byte of
// the image is written.  Threshold and consistency rows are framed (frame_threshold, frame_consistency) into host images of their arena
// regions (thr_img, con_img, zero elsewhere) with the job lists that fill in proofs and commitments on the device: offsets relative to the
// variant's image, seed index = row.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>
#include "bp_steps.h"
#include "stark_steps.h"
#include "batch_self_check.h"
#include "plan_take.h"
#include "../../include/libzkp_hip.h"

namespace zkp {

// ---- envelope sizes, named once
constexpr uint32_t EQUALITY_ENVELOPE_BYTES = 298;                                         // scheme 2: 10 header | 256 proof | 32 commitment
static_assert(SC_EQ_BYTES == EQUALITY_ENVELOPE_BYTES, "batch_self_check.h reads the commitment of the same envelope");
inline uint64_t membership_envelope_bytes(uint32_t count) { return 10 + 4 + 8ull * count + 256 + 32; }      // scheme 4: 10 header | u32 count | count x u64 | 256 proof | 32 commitment
inline uint64_t threshold_envelope_bytes(uint32_t lg) { return 10 + 8 + 4 + 4 + rp_bytes(lg) + 32 + 32; }      // 762 for n_bits = 64
inline uint64_t consistency_envelope_bytes(uint32_t count) {
    if (count == 0) return 0;
    return 10 + 4 + 32ull * count + (uint64_t)(4 + RP_BYTES) * (count - 1) + 32ull * (count - 1) + 32;
}

// The reference's validation rules (utils/validation.rs), one predicate each, for the per-variant entry points and the batch scheduler
// (plan_stage_layout) alike.  The threshold rule is frame_threshold's.
inline bool equality_ok(uint64_t a, uint64_t b) { return a == b; }                                 // validation.rs:21-26
inline bool membership_ok(uint64_t value, const uint64_t* set, uint32_t count) {                 // validation.rs:47-60; sets of at most 64 (snark.rs:406-418)
    if (count == 0 || count > G16_MAX_SET) return false;
    for (uint32_t k = 0; k < count; k++) if (set[k] == value) return true;
    return false;
}
inline bool improvement_ok(uint64_t old_value, uint64_t new_value) { return new_value > old_value; }     // validation.rs:63-71
inline bool consistency_ok(const uint64_t* list, uint32_t count) {                                  // validation.rs:74-86: not empty, non-decreasing
    if (count == 0) return false;
    for (uint32_t j = 1; j < count; j++) if (list[j - 1] > list[j]) return false;
    return true;
}

// ---------------------------------------------------------------------------------------------------
// Host-described jobs (threshold / consistency framings have variable-length inputs, so their job lists are built on
// the host: pure bookkeeping, bulletproofs.rs:309-437).  The proving itself is the same device pipeline.
struct HostJobs {
    std::vector<uint64_t> v, proof_off, commit_off, ct_v, ct_off;
    std::vector<uint32_t> seed_ix, proof_ix, ct_seed_ix, ct_bl_ix;
    std::vector<int32_t> bl_plus, bl_minus;
    std::vector<uint8_t> kind;
    void add_job(uint64_t val, uint32_t seed, uint32_t pidx, int32_t plus, int32_t minus, uint8_t k, uint64_t poff, uint64_t coff) {
        v.push_back(val); seed_ix.push_back(seed); proof_ix.push_back(pidx); bl_plus.push_back(plus); bl_minus.push_back(minus);
        kind.push_back(k); proof_off.push_back(poff); commit_off.push_back(coff);
    }
    void add_commit(uint64_t val, uint32_t seed, uint32_t bl, uint64_t off) { ct_v.push_back(val); ct_seed_ix.push_back(seed); ct_bl_ix.push_back(bl); ct_off.push_back(off); }
};

inline void put_le_host(uint8_t* p, uint64_t x, int n) { for (int i = 0; i < n; i++) p[i] = (uint8_t)(x >> (8 * i)); }

// Framing of threshold proofs (threshold_proof.rs:12-32 -> bulletproofs.rs:309-366): validates every op, writes the envelope
// and body framing of the valid ones into `img` (n records of `stride` bytes, zeroed by the caller) and appends one proof
// job + one commitment task per valid op; seed index = op index.  Returns 1 if any op is invalid.
inline int frame_threshold(uint64_t n, const uint64_t* values, const uint32_t* counts, const uint64_t* thresholds, uint32_t lg,
                           uint8_t* img, uint64_t stride, uint32_t* out_len, int32_t* status, HostJobs& H) {
    const uint32_t RP = rp_bytes(lg), n_bits = 1u << lg;
    const uint64_t PB = threshold_envelope_bytes(lg);
    const uint64_t max_diff = lg >= 6 ? ~0ull : (1ull << (1u << lg)) - 1;   // bulletproofs.rs:330-336
    int any = 0; size_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        // validation.rs:30-47 / bulletproofs.rs:314-336
        bool ok = counts[i] > 0; uint64_t sum = 0;
        for (uint32_t k = 0; k < counts[i] && ok; k++) { const uint64_t x = values[pos + k]; if (sum + x < sum) ok = false; sum += x; }
        pos += counts[i];
        if (ok && sum < thresholds[i]) ok = false;
        if (ok && sum - thresholds[i] > max_diff) ok = false;
        status[i] = ok ? ZKP_HIP_OK : ZKP_HIP_INVALID_INPUT; out_len[i] = ok ? (uint32_t)PB : 0; any |= !ok;
        if (!ok) continue;
        uint8_t* o = img + i * stride; const uint64_t base = i * stride;
        o[0] = 2; o[1] = 3; put_le_host(o + 2, 8 + 4 + 4 + RP + 32, 4); put_le_host(o + 6, 32, 4);
        put_le_host(o + 10, thresholds[i], 8); put_le_host(o + 18, n_bits, 4); put_le_host(o + 22, RP, 4);
        H.add_job(sum - thresholds[i], (uint32_t)i, 0, 0, -1, KIND_THRESHOLD, base + 26, base + 26 + RP);
        H.add_commit(sum, (uint32_t)i, 0, base + 26 + RP + 32);
    }
    return any;
}
// Framing of consistency proofs (consistency_proof.rs:12-22 -> bulletproofs.rs:368-437): k commitment tasks and k - 1 proof
// jobs per valid op.  The envelope's commitment field (SHA-256 of the commitment list) is filled in after the device run.
inline int frame_consistency(uint64_t n, const uint64_t* data, const uint32_t* counts, uint8_t* img, uint64_t stride, uint32_t* out_len, int32_t* status, HostJobs& H) {
    int any = 0; size_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t k = counts[i]; const uint64_t* d = data + pos; pos += k;
        bool ok = consistency_ok(d, k);
        const uint64_t need = consistency_envelope_bytes(k);
        if (ok && need > stride) ok = false;                        // (callers size the stride from the counts; never reached through the ABI)
        status[i] = ok ? ZKP_HIP_OK : ZKP_HIP_INVALID_INPUT; out_len[i] = ok ? (uint32_t)need : 0; any |= !ok;
        if (!ok) continue;
        uint8_t* o = img + i * stride; const uint64_t base = i * stride;
        const uint64_t body = need - 10 - 32;
        o[0] = 2; o[1] = 6; put_le_host(o + 2, body, 4); put_le_host(o + 6, 32, 4);
        put_le_host(o + 10, k, 4);
        const uint64_t commits = base + 14, proofs = commits + 32ull * k, dcs = proofs + (uint64_t)(4 + RP_BYTES) * (k - 1);
        for (uint32_t j = 0; j < k; j++) H.add_commit(d[j], (uint32_t)i, j, commits + 32ull * j);
        for (uint32_t j = 1; j < k; j++) {
            put_le_host(img + proofs + (uint64_t)(4 + RP_BYTES) * (j - 1), RP_BYTES, 4);
            H.add_job(d[j] - d[j - 1], (uint32_t)i, j - 1, (int32_t)j, (int32_t)(j - 1), KIND_CONSISTENCY,
                      proofs + (uint64_t)(4 + RP_BYTES) * (j - 1) + 4, dcs + 32ull * (j - 1));
        }
    }
    return any;
}

// the op's kind without the batch-wide ZKP_HIP_OP_SELF_CHECK flag: every reader of `kind` goes through this
ZKP_HD inline uint32_t op_kind(const zkp_hip_op& o) { return o.kind & ~ZKP_HIP_OP_SELF_CHECK; }
inline uint64_t op_max_bytes(const zkp_hip_op& o) {
    switch (op_kind(o)) {
        case ZKP_HIP_OP_RANGE: return RANGE_PROOF_BYTES;
        case ZKP_HIP_OP_EQUALITY: return EQUALITY_ENVELOPE_BYTES;
        case ZKP_HIP_OP_THRESHOLD: return threshold_envelope_bytes(6);
        case ZKP_HIP_OP_MEMBERSHIP: return membership_envelope_bytes(o.count <= G16_MAX_SET ? o.count : 0);
        case ZKP_HIP_OP_IMPROVEMENT: return STARK_MAX_ENVELOPE;
        case ZKP_HIP_OP_CONSISTENCY: return consistency_envelope_bytes(o.count);
        default: return 0;
    }
}

// Which shard proves which op: every variant's bucket (ops of one kind, in the caller's order) is cut into `shards` contiguous
// slices whose sizes differ by at most one, so all GPUs run the same kernel mix.  Pure host logic.
inline void plan_shards(uint64_t n, const zkp_hip_op* ops, uint32_t shards, uint32_t* shard_of_op) {
    uint64_t count[7] = {0, 0, 0, 0, 0, 0, 0}, seen[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = 0; i < n; i++) count[op_kind(ops[i])]++;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t k = op_kind(ops[i]);
        const uint64_t q = seen[k]++, m = count[k];
        // slice s holds bucket positions [m*s/S, m*(s+1)/S): the owner of position q is the largest s with m*s/S <= q
        uint32_t s = (uint32_t)(((q + 1) * shards - 1) / m);
        while (s > 0 && m * s / shards > q) s--;
        while (s + 1 < shards && m * (s + 1) / shards <= q) s++;
        shard_of_op[i] = s;
    }
}

// ---- one shard's staging
constexpr uint32_t LEN_DYN = 0xffffffffu;          // the pack view's len_fixed / dyn_kind values (PackView, batch_impl.inc)
enum : uint8_t { DYN_NONE = 0, DYN_LEN_STATUS = 1, DYN_LEN_ONLY = 2 };

struct VariantPlan { uint32_t rows = 0; uint64_t stride = 0, arena = 0; uint32_t row0 = 0; };
struct StagePlan {
    uint32_t n = 0;
    std::vector<uint32_t> gidx;            // global op index of local op j (ascending)
    bool self_check = false;               // every op carries ZKP_HIP_OP_SELF_CHECK
    // ---- written by plan_stage_layout
    VariantPlan var[SC_KINDS];             // indexed by op kind (entry 0 stays empty)
    std::vector<uint8_t> row_ok;           // [n] 0: refused by the host's validation (equality, membership, improvement)
    uint64_t max_total = 0;
    size_t in_bytes = 0, arena_bytes = 0, meta_bytes = 0;
    // offsets into the image: the variants' input columns, then the pack view's per-op table
    size_t i_rv = 0, i_rmin = 0, i_rmax = 0, i_rseed = 0, i_ev = 0, i_eseed = 0, i_mv = 0, i_msets = 0, i_mlen = 0, i_mseed = 0, i_io = 0, i_in = 0,
           i_tseed = 0, i_cseed = 0, i_ccount = 0, i_clen = 0, i_src = 0, i_lenf = 0, i_dix = 0, i_dkind = 0, i_stf = 0;
    // self-check: the thresholds, every op's variant, the verifiers' lens / verdict rows and the row <-> op map (device-written), two counters
    size_t i_thr = 0, i_var = 0, i_rlen = 0, i_rop = 0, i_rok = 0, i_oprow = 0, i_cnt = 0;
    size_t a_dlen = 0, a_dst = 0;                    // arena, behind the rows: the lengths (range, then improvement) and statuses (range) the device reports
    size_t m_off = 0, m_status = 0, m_len = 0;       // result block: out_off[n + 1] | status[n] | len[n]
    // ---- written by fill_stage_image
    HostJobs thrJ, conJ;
    std::vector<uint8_t> thr_img, con_img;
    std::vector<uint32_t> con_counts, con_lens;
    std::vector<uint8_t> op_variant;       // [n] flagged batches: the op's kind when it has an arena row, else 0
};

// Pass 1 and the layout, from P.n and P.gidx: rows and strides per variant, row_ok, max_total, every offset and block size.
inline void plan_stage_layout(StagePlan& P, const zkp_hip_op* ops, const uint64_t* lists, bool self_check) {
    const uint32_t n = P.n;
    P.self_check = self_check;
    for (VariantPlan& v : P.var) v = VariantPlan();
    VariantPlan &R = P.var[ZKP_HIP_OP_RANGE], &E = P.var[ZKP_HIP_OP_EQUALITY], &T = P.var[ZKP_HIP_OP_THRESHOLD], &M = P.var[ZKP_HIP_OP_MEMBERSHIP],
                &I = P.var[ZKP_HIP_OP_IMPROVEMENT], &C = P.var[ZKP_HIP_OP_CONSISTENCY];
    R.stride = RANGE_PROOF_BYTES; E.stride = EQUALITY_ENVELOPE_BYTES; T.stride = threshold_envelope_bytes(6); I.stride = STARK_MAX_ENVELOPE;
    // ---- pass 1: count rows per variant, validate what the host validates (in locals: the byte stores into row_ok may alias P)
    P.row_ok.assign(n, 1);
    uint8_t* ok = P.row_ok.data();
    uint32_t rows[SC_KINDS] = {0, 0, 0, 0, 0, 0, 0};
    uint64_t max_total = 0;
    for (uint32_t j = 0; j < n; j++) {
        const zkp_hip_op& o = ops[P.gidx[j]];
        max_total += op_max_bytes(o);
        switch (op_kind(o)) {
            case ZKP_HIP_OP_EQUALITY: ok[j] = equality_ok(o.a, o.b); break;
            case ZKP_HIP_OP_MEMBERSHIP:
                ok[j] = membership_ok(o.a, lists + o.list_off, o.count);
                if (ok[j] && op_max_bytes(o) > M.stride) M.stride = op_max_bytes(o);
                break;
            case ZKP_HIP_OP_IMPROVEMENT: ok[j] = improvement_ok(o.a, o.b); break;
            case ZKP_HIP_OP_CONSISTENCY: if (consistency_envelope_bytes(o.count ? o.count : 1) > C.stride) C.stride = consistency_envelope_bytes(o.count ? o.count : 1); break;
            default: break;
        }
        rows[op_kind(o)] += ok[j];
    }
    for (uint32_t k = 0; k < SC_KINDS; k++) P.var[k].rows = rows[k];
    P.max_total = max_total;
    // ---- layout of the staging image, the arena and the result block
    PlanTake take;
    P.i_rv = take(8ull * R.rows); P.i_rmin = take(8ull * R.rows); P.i_rmax = take(8ull * R.rows); P.i_rseed = take(32ull * R.rows);
    P.i_ev = take(8ull * E.rows); P.i_eseed = take(32ull * E.rows);
    P.i_mv = take(8ull * M.rows); P.i_msets = take(8ull * G16_MAX_SET * M.rows); P.i_mlen = take(4ull * M.rows); P.i_mseed = take(32ull * M.rows);
    P.i_io = take(8ull * I.rows); P.i_in = take(8ull * I.rows);
    P.i_tseed = take(32ull * T.rows); P.i_cseed = take(32ull * C.rows); P.i_ccount = take(4ull * C.rows); P.i_clen = take(4ull * C.rows);
    P.i_src = take(8ull * n); P.i_lenf = take(4ull * n); P.i_dix = take(4ull * n); P.i_dkind = take(n); P.i_stf = take(4ull * n);
    if (self_check) {
        // what the verifier cores need beside the prover's inputs: the thresholds (the prover takes them through the framing), and rows of
        // lens / verdicts per variant, built on the device (k_self_check_rows); a variant's rows start at a multiple of SC_ROW_ALIGN
        uint32_t total = 0;
        for (VariantPlan& v : P.var) { v.row0 = total; total += (v.rows + SC_ROW_ALIGN - 1) / SC_ROW_ALIGN * SC_ROW_ALIGN; }
        P.i_thr = take(8ull * T.rows); P.i_var = take(n); P.i_rlen = take(4ull * total); P.i_rop = take(4ull * total); P.i_rok = take(total);
        P.i_oprow = take(4ull * n); P.i_cnt = take(8);
    }
    P.in_bytes = take.off;
    take.off = 0;
    for (VariantPlan* v : {&R, &E, &M, &I, &T, &C}) v->arena = take(v->stride * v->rows);
    P.a_dlen = take(4ull * (R.rows + I.rows)); P.a_dst = take(4ull * R.rows);
    P.arena_bytes = take.off;
    take.off = 0;
    P.m_off = take(8ull * (n + 1)); P.m_status = take(4ull * n); P.m_len = take(4ull * n);
    P.meta_bytes = take.off;
}

// The image of a planned shard into h (P.in_bytes bytes), and the host-side products of the framing.
inline void fill_stage_image(StagePlan& P, const zkp_hip_op* ops, const uint64_t* lists, const uint8_t* seeds, uint8_t* h) {
    const uint32_t n = P.n;
    const VariantPlan &R = P.var[ZKP_HIP_OP_RANGE], &E = P.var[ZKP_HIP_OP_EQUALITY], &T = P.var[ZKP_HIP_OP_THRESHOLD], &M = P.var[ZKP_HIP_OP_MEMBERSHIP],
                      &I = P.var[ZKP_HIP_OP_IMPROVEMENT], &C = P.var[ZKP_HIP_OP_CONSISTENCY];
    auto u64p = [&](size_t o) { return reinterpret_cast<uint64_t*>(h + o); };
    auto u32p = [&](size_t o) { return reinterpret_cast<uint32_t*>(h + o); };
    uint64_t* src = u64p(P.i_src); uint32_t* lenf = u32p(P.i_lenf); uint32_t* dix = u32p(P.i_dix); uint8_t* dkind = h + P.i_dkind;
    int32_t* stf = reinterpret_cast<int32_t*>(h + P.i_stf);
    // threshold / consistency inputs gathered for the framing helpers
    std::vector<uint64_t> t_vals, t_thr, c_vals; std::vector<uint32_t> t_counts, c_counts, t_at, c_at;
    uint32_t r = 0, e = 0, m = 0, s = 0;
    for (uint32_t j = 0; j < n; j++) {
        const uint64_t gi = P.gidx[j];
        const zkp_hip_op& o = ops[gi];
        const uint8_t* sd = seeds + 32 * gi;
        src[j] = 0; lenf[j] = 0; dix[j] = 0; dkind[j] = DYN_NONE; stf[j] = P.row_ok[j] ? ZKP_HIP_OK : ZKP_HIP_INVALID_INPUT;
        switch (op_kind(o)) {
            case ZKP_HIP_OP_RANGE:
                u64p(P.i_rv)[r] = o.a; u64p(P.i_rmin)[r] = o.b; u64p(P.i_rmax)[r] = o.c; memcpy(h + P.i_rseed + 32ull * r, sd, 32);
                src[j] = R.arena + R.stride * r; lenf[j] = LEN_DYN; dix[j] = r; dkind[j] = DYN_LEN_STATUS; r++;
                break;
            case ZKP_HIP_OP_EQUALITY:
                if (!P.row_ok[j]) break;
                u64p(P.i_ev)[e] = o.a; memcpy(h + P.i_eseed + 32ull * e, sd, 32);
                src[j] = E.arena + E.stride * e; lenf[j] = EQUALITY_ENVELOPE_BYTES; e++;
                break;
            case ZKP_HIP_OP_MEMBERSHIP:
                if (!P.row_ok[j]) break;
                u64p(P.i_mv)[m] = o.a; u32p(P.i_mlen)[m] = o.count; memcpy(h + P.i_mseed + 32ull * m, sd, 32);
                for (uint32_t k = 0; k < G16_MAX_SET; k++) u64p(P.i_msets)[(size_t)G16_MAX_SET * m + k] = k < o.count ? lists[o.list_off + k] : 0;
                src[j] = M.arena + M.stride * m; lenf[j] = (uint32_t)op_max_bytes(o); m++;
                break;
            case ZKP_HIP_OP_IMPROVEMENT:
                if (!P.row_ok[j]) break;
                u64p(P.i_io)[s] = o.a; u64p(P.i_in)[s] = o.b;
                src[j] = I.arena + I.stride * s; lenf[j] = LEN_DYN; dix[j] = R.rows + s; dkind[j] = DYN_LEN_ONLY; s++;
                break;
            case ZKP_HIP_OP_THRESHOLD:
                memcpy(h + P.i_tseed + 32ull * t_at.size(), sd, 32);
                t_thr.push_back(o.a); t_counts.push_back(o.count); t_vals.insert(t_vals.end(), lists + o.list_off, lists + o.list_off + o.count);
                t_at.push_back(j);
                break;
            default:
                memcpy(h + P.i_cseed + 32ull * c_at.size(), sd, 32);
                c_counts.push_back(o.count); c_vals.insert(c_vals.end(), lists + o.list_off, lists + o.list_off + o.count);
                c_at.push_back(j);
                break;
        }
    }
    if (T.rows) {
        P.thr_img.assign(T.stride * T.rows, 0);
        std::vector<uint32_t> lens(T.rows); std::vector<int32_t> st(T.rows);
        (void)frame_threshold(T.rows, t_vals.data(), t_counts.data(), t_thr.data(), 6, P.thr_img.data(), T.stride, lens.data(), st.data(), P.thrJ);
        for (uint32_t k = 0; k < T.rows; k++) { const uint32_t j = t_at[k]; src[j] = T.arena + T.stride * k; lenf[j] = lens[k]; stf[j] = st[k]; }
    }
    if (C.rows) {
        P.con_img.assign(C.stride * C.rows, 0);
        P.con_lens.assign(C.rows, 0); std::vector<int32_t> st(C.rows);
        (void)frame_consistency(C.rows, c_vals.data(), c_counts.data(), P.con_img.data(), C.stride, P.con_lens.data(), st.data(), P.conJ);
        P.con_counts = c_counts;
        for (uint32_t k = 0; k < C.rows; k++) {
            const uint32_t j = c_at[k]; src[j] = C.arena + C.stride * k; lenf[j] = P.con_lens[k]; stf[j] = st[k];
            u32p(P.i_ccount)[k] = c_counts[k]; u32p(P.i_clen)[k] = P.con_lens[k];
        }
    }
    if (P.self_check) {
        P.op_variant.assign(n, 0);
        for (uint32_t j = 0; j < n; j++) if (P.row_ok[j]) P.op_variant[j] = (uint8_t)op_kind(ops[P.gidx[j]]);      // (an op the host refused has no row)
        if (n) memcpy(h + P.i_var, P.op_variant.data(), n);
        if (T.rows) memcpy(h + P.i_thr, t_thr.data(), 8ull * T.rows);
    }
}

}  // namespace zkp
