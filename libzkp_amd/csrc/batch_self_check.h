// Self-check of a staged batch (ZKP_HIP_OP_SELF_CHECK, include/libzkp_hip.h): after proving, every variant's arena rows go through that
// scheme's verifier against the op's own staged parameters, and an op whose envelope is not accepted leaves the GPU as a failed op.  The
// verifiers are the library's own (bpv_impl.inc, g16_impl.inc, stark_impl.inc) on device pointers; what is here is the glue around them,
// per-lane step functions shared by the kernels (batch_impl.inc: k_self_check_*) and the host build of tests/emul/emul_self_check.cpp:
//
//   rows   lane = op     the envelope length of the op's row, as the pack kernels will take it (0 for an op that failed validation or proving,
//                        so its verifier rejects the row), and the row <-> op map
//   bind   lane = row    what the Groth16 verifiers leave to their callers (include/libzkp_hip.h: "callers compare those with what they
//                        expect"): the equality envelope's commitment is MiMC(a) of the staged value, the membership envelope's embedded
//                        set is the staged set, in the staged order
//   apply  lane = op     verdict rows back to op order: a refused op gets status 2 and length 0 before the lengths are prefix-summed
//   flip   one lane      the diagnostic switch ZKP_HIP_SELF_CHECK_FLIP
#pragma once
#include "zkp_common.h"
#include "g16_steps.h"

namespace zkp {

constexpr uint32_t SC_LEN_DYN = 0xffffffffu;          // PackView's LEN_DYN / DYN_* (batch_impl.inc asserts that they agree)
constexpr uint8_t SC_DYN_LEN_STATUS = 1;
constexpr int32_t SC_STATUS_REFUSED = 2;              // ZKP_HIP_PROOF_GENERATION_FAILED
constexpr uint32_t SC_NO_ROW = 0xffffffffu;
constexpr uint32_t SC_KINDS = 7;                      // variants are indexed by the op kind, 1..6
constexpr uint32_t SC_ROW_ALIGN = 64;                 // a variant's rows start at a multiple of this in the row arrays
constexpr uint32_t SC_EQ_COMMITMENT_AT = 266, SC_EQ_BYTES = 298;      // scheme 2: 10 header | 256 proof | 32 commitment
constexpr uint32_t SC_MEM_COUNT_AT = 10, SC_MEM_SET_AT = 14;          // scheme 4: 10 header | u32 count | count x u64 | 256 proof | 32 commitment

struct SelfCheckView {
    uint32_t n;                            // ops of the shard
    // the pack view's inputs (PackView, batch_impl.inc)
    const uint64_t* src_off; const uint32_t* len_fixed; const uint32_t* dyn_ix; const uint8_t* dyn_kind; const int32_t* status_fixed;
    const uint32_t* dyn_len; const int32_t* dyn_status;
    const uint8_t* op_variant;             // [n] the op's kind when it has an arena row, 0 when it has none (refused by host validation)
    uint64_t base[SC_KINDS], stride[SC_KINDS];      // the variant's rows in the arena
    uint32_t row0[SC_KINDS], rows[SC_KINDS];        // its slice of the row arrays below
    uint32_t* row_len; uint32_t* row_op; uint8_t* row_ok;      // [rows of all variants] lens / op of the row / verdict, as the verifiers take them
    uint32_t* op_row;                      // [n] the op's index in the row arrays, or SC_NO_ROW
    uint32_t* len; int32_t* status;        // [n] what k_batch_lens wrote
    // the Groth16 binding
    const uint8_t* arena; const uint64_t* eq_value; const uint64_t* mem_sets; const uint32_t* mem_len; const uint32_t* mimc_c;
};

// length and status of op i as k_batch_lens takes them
ZKP_HD inline uint32_t sc_op_len(const SelfCheckView& V, uint32_t i) {
    int32_t st = V.status_fixed[i];
    uint32_t l = V.len_fixed[i];
    if (st == 0 && l == SC_LEN_DYN) {
        const uint32_t k = V.dyn_ix[i];
        l = V.dyn_len[k];
        if (V.dyn_kind[i] == SC_DYN_LEN_STATUS) st = V.dyn_status[k];
    }
    return st != 0 ? 0u : l;
}
ZKP_HD inline void step_self_check_rows(const SelfCheckView& V, uint32_t i) {
    const uint32_t v = V.op_variant[i];
    uint64_t base = 0, stride = 1; uint32_t row0 = 0;
    ZKP_UNROLL for (uint32_t k = 1; k < SC_KINDS; k++) if (v == k) { base = V.base[k]; stride = V.stride[k]; row0 = V.row0[k]; }
    if (v == 0 || v >= SC_KINDS) { V.op_row[i] = SC_NO_ROW; return; }
    const uint32_t g = row0 + (uint32_t)((V.src_off[i] - base) / stride);
    V.row_len[g] = sc_op_len(V, i); V.row_op[g] = i; V.op_row[i] = g;
}

// the 32-byte commitment of an equality envelope is commit_value_snark(value): MiMC-5/110 of the value, little-endian canonical bytes
ZKP_HD inline bool sc_equality_bound(const uint8_t* env, uint64_t value, const uint32_t* mimc_c) {
    G16View M{}; M.mimc_c = mimc_c; M.z = nullptr;
    const fr h = g16_mimc_chain(M, 0, fp_from_u64<FrParams>(value), 0);
    uint32_t w[8]; fp_to_raw(w, h);
    uint32_t diff = 0;
    ZKP_UNROLL for (uint32_t k = 0; k < 8; k++) {
        const uint8_t* c = env + SC_EQ_COMMITMENT_AT + 4 * k;
        diff |= w[k] ^ ((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24));
    }
    return diff == 0;
}
// the count and the elements a membership envelope embeds are the staged set, element by element (`set`: the op's 64 padded slots)
ZKP_HD inline bool sc_membership_bound(const uint8_t* env, const uint64_t* set, uint32_t count) {
    if (count > G16_MAX_SET) return false;
    const uint8_t* c = env + SC_MEM_COUNT_AT;
    if (((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24)) != count) return false;
    bool same = true;
    for (uint32_t i = 0; i < count; i++) {
        const uint8_t* e = env + SC_MEM_SET_AT + 8 * i; uint64_t x = 0;
        for (int b = 0; b < 8; b++) x |= (uint64_t)e[b] << (8 * b);
        same = same && x == set[i];
    }
    return same;
}
// lane t: equality row t, then membership row t - rows[equality].  Rows the verifier refused stay refused.
ZKP_HD inline void step_self_check_bind_g16(const SelfCheckView& V, uint32_t t) {
    const uint32_t ne = V.rows[2], nm = V.rows[4];
    if (t >= ne + nm) return;
    const bool eq = t < ne;
    const uint32_t r = eq ? t : t - ne, g = (eq ? V.row0[2] : V.row0[4]) + r;
    if (!V.row_ok[g] || V.row_len[g] == 0) return;
    const uint8_t* env = V.arena + (eq ? V.base[2] + V.stride[2] * r : V.base[4] + V.stride[4] * r);
    const bool bound = eq ? sc_equality_bound(env, V.eq_value[r], V.mimc_c) : sc_membership_bound(env, V.mem_sets + (size_t)G16_MAX_SET * r, V.mem_len[r]);
    if (!bound) V.row_ok[g] = 0;
}

// bit 0: the op's envelope went through its verifier; bit 1: it was refused (status 2, no bytes).  Ops that failed before keep their status.
ZKP_HD inline uint32_t step_self_check_apply(const SelfCheckView& V, uint32_t i) {
    const uint32_t g = V.op_row[i];
    if (g == SC_NO_ROW || V.status[i] != 0) return 0;
    if (V.row_ok[g]) return 1;
    V.status[i] = SC_STATUS_REFUSED; V.len[i] = 0;
    return 3;
}

// ZKP_HIP_SELF_CHECK_FLIP: bit 0 of one byte of op j's arena record
ZKP_HD inline void step_self_check_flip(uint8_t* arena, const uint64_t* src_off, uint32_t j, uint32_t byte) { arena[src_off[j] + byte] ^= 1u; }

}  // namespace zkp
