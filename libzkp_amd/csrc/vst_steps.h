// Envelopes against the caller's statements (include/libzkp_hip_statements.h): n ops, the array zkp_hip_process_batch took, and the n envelopes
// proved from them, packed back to back as for the mixed verifier (venv_steps.h).  What is here decides steps 1 and 2 of that header -- the
// envelope, then the statement -- per lane; what survives them goes through the mixed verifier's spine unchanged (ve_plan, unpack, the
// verifier cores, apply).  Per-lane step functions shared by the kernels (vst_impl.inc: k_vst_*) and the host build of
// tests/emul/emul_verify_ops.cpp; no HIP call in them:
//
//   classify         lane = envelope   step_venv_classify, the scheme against the op's kind, then the statements that are plain words of the op
//                                      (range, threshold, improvement, equality by value: a == b; the list spans and counts of the others).  The
//                                      mixed verifier's 32-byte record comes out, scheme = 0 for a refusal, the reason in its `reserved` word
//   bind equality    lane = envelope   live equality envelopes only: the commitment is MiMC-5/110 of the value (the chain sc_equality_bound
//                                      runs), or the four list words of the commitment form
//   bind membership  wave = envelope   live membership envelopes only: lane k holds embedded element k and statement element k; the wave
//                                      decides multiset equality by multiplicity counting over lane broadcasts
//   apply            lane = envelope   step_venv_apply, and ZKP_STMT_PROOF for an envelope that had a row and was refused
#pragma once
#include "venv_steps.h"
#include "batch_plan.h"
#include "../../include/libzkp_hip_statements.h"

namespace zkp {

constexpr uint32_t VST_EQ_COMMITMENT_WORDS = 4;          // count of an equality op in the commitment form: 32 bytes as four list words

// A host test build (tests/emul/emul_verify_ops.cpp defines VST_COUNT_OUTSIDE_READS) counts list reads outside [0, n_lists) and gives them
// the value 0 in place of the read; everywhere else this is the load.
#if defined(VST_COUNT_OUTSIDE_READS)
inline uint64_t& vst_outside_reads() { static uint64_t c = 0; return c; }
#endif
ZKP_HD inline uint64_t vst_list_at(const uint64_t* lists, uint64_t n_lists, uint64_t k) {
#if defined(VST_COUNT_OUTSIDE_READS)
    if (k >= n_lists) { vst_outside_reads()++; return 0; }
#else
    (void)n_lists;
#endif
    return lists[k];
}
ZKP_HD inline bool vst_span_inside(uint64_t list_off, uint64_t count, uint64_t n_lists) { return list_off <= n_lists && count <= n_lists - list_off; }

// Envelope i of n against op i.  The record is the mixed verifier's; r.reserved = the reason (ZKP_STMT_*), 0 for an envelope that is live.
// A live equality or membership envelope still has to be bound (step_vst_bind_equality / the membership steps).  No list value is read.
ZKP_HD inline VenvRecord step_vst_classify(const uint8_t* blob, const uint64_t* off, const zkp_hip_op* ops, uint64_t n_lists, uint64_t n, uint64_t i) {
    VenvRecord r = step_venv_classify(blob, off, nullptr, n, i);
    const VenvRecord refused{0, r.len, 0, 0, 0, ZKP_STMT_ENVELOPE};
    if (r.scheme == 0) return refused;
    const zkp_hip_op o = ops[i];
    const uint32_t kind = op_kind(o);
    VenvRecord no_statement = refused; no_statement.reserved = ZKP_STMT_STATEMENT;
    if (kind < ZKP_HIP_OP_RANGE || kind > ZKP_HIP_OP_CONSISTENCY) return no_statement;
    if (r.scheme != kind) return refused;
    bool mine = true;
    if (kind == ZKP_HIP_OP_RANGE) mine = o.b <= o.c && r.p0 == o.b && r.p1 == o.c;
    else if (kind == ZKP_HIP_OP_THRESHOLD || kind == ZKP_HIP_OP_IMPROVEMENT) mine = r.p0 == o.a;
    else if (kind == ZKP_HIP_OP_EQUALITY) mine = o.count == 0 ? o.a == o.b : o.count == VST_EQ_COMMITMENT_WORDS && vst_span_inside(o.list_off, o.count, n_lists);
    else if (kind == ZKP_HIP_OP_MEMBERSHIP)
        mine = o.count >= 1 && o.count <= G16_MAX_SET && vst_span_inside(o.list_off, o.count, n_lists) && ve_le(blob + off[i] + SC_MEM_COUNT_AT, 4) == o.count;
    return mine ? r : no_statement;
}

// A live equality envelope (classified: 32 commitment bytes end it; a == b, or count == 4 with its span inside the lists): is its commitment
// the statement's?  Byte loads at whatever alignment the envelope has.
ZKP_HD inline bool step_vst_bind_equality(const uint8_t* blob, const uint64_t* off, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists,
                                          const uint32_t* mimc_c, uint64_t i) {
    const zkp_hip_op o = ops[i];
    const uint8_t* c = blob + off[i + 1] - 32;
    uint32_t diff = 0;
    if (o.count == 0) {
        G16View M{}; M.mimc_c = mimc_c; M.z = nullptr;
        const fr h = g16_mimc_chain(M, 0, fp_from_u64<FrParams>(o.a), 0);
        uint32_t w[8]; fp_to_raw(w, h);
        ZKP_UNROLL for (uint32_t k = 0; k < 8; k++) diff |= w[k] ^ (uint32_t)ve_le(c + 4 * k, 4);
    } else {
        ZKP_UNROLL for (uint32_t k = 0; k < VST_EQ_COMMITMENT_WORDS; k++) {
            const uint64_t x = vst_list_at(lists, n_lists, o.list_off + k) ^ ve_le(c + 8 * k, 8);
            diff |= (uint32_t)x | (uint32_t)(x >> 32);
        }
    }
    return diff == 0;
}

// A live membership envelope (classified: 1 <= count <= 64 = the embedded count, the embedded elements inside the envelope, the span inside
// the lists), one wave: lane k < count holds embedded element k and statement element k.  A lane >= count holds nothing that is compared:
// the counting loop runs over the lanes below count only, and such a lane's own vote is yes.
struct VstMemLane { uint64_t emb, stmt; };
ZKP_HD inline VstMemLane step_vst_mem_load(const uint8_t* blob, const uint64_t* off, const zkp_hip_op& o, const uint64_t* lists, uint64_t n_lists, uint64_t i, uint32_t lane) {
    VstMemLane L{0, 0};
    if (lane < o.count) { L.emb = ve_le(blob + off[i] + SC_MEM_SET_AT + 8ull * lane, 8); L.stmt = vst_list_at(lists, n_lists, o.list_off + lane); }
    return L;
}
// Both multisets have `count` elements, so they are equal iff every embedded element occurs as often in the statement as in the envelope:
// the multiplicities of the embedded elements then add up to count on the statement's side too, which leaves it no other element.
// lane_of(j) = lane j's VstMemLane (a broadcast; j < count, the same for every lane).  Returns this lane's vote; the wave ANDs them.
template <class LaneOf> ZKP_HD inline bool step_vst_mem_count(const VstMemLane& mine, uint32_t lane, uint32_t count, LaneOf lane_of) {
    uint32_t in_emb = 0, in_stmt = 0;
    for (uint32_t j = 0; j < count; j++) {
        const VstMemLane other = lane_of(j);
        in_emb += other.emb == mine.emb ? 1u : 0u;
        in_stmt += other.stmt == mine.emb ? 1u : 0u;
    }
    return lane >= count || in_emb == in_stmt;
}

// verdict and reason of envelope i behind the verifiers: the classification's reason for an envelope without a row
ZKP_HD inline uint8_t step_vst_apply(const VenvView& V, uint64_t i, uint8_t& why) {
    const uint8_t ok = step_venv_apply(V, i);
    why = V.op_row[i] == SC_NO_ROW ? (uint8_t)V.rec[i].reserved : ok ? (uint8_t)ZKP_STMT_ACCEPTED : (uint8_t)ZKP_STMT_PROOF;
    return ok;
}

// ---- host only: what one slice of a host-buffer call uploads of the lists (zkp_stmt_verify, spread over the shards)
struct VstListSpan { uint64_t lo, count; };          // lists[lo .. lo + count)
// The m ops of a slice: the span of `lists` its list-bearing ops name -- equality ops in the commitment form and membership ops whose count
// is a statement and whose span lies inside [0, n_lists) -- from the smallest list_off to the largest list_off + count, and the ops with
// list_off re-based to that span (`out`, m entries).  An op whose span the classification refuses keeps being refused: its list_off becomes
// ~0, which lies inside no span.  No such op: the empty span at 0.
inline VstListSpan vst_slice_ops(uint64_t m, const zkp_hip_op* ops, uint64_t n_lists, zkp_hip_op* out) {
    auto bears = [&](const zkp_hip_op& o) {
        const uint32_t kind = op_kind(o);
        const bool counts = kind == ZKP_HIP_OP_EQUALITY ? o.count == VST_EQ_COMMITMENT_WORDS : kind == ZKP_HIP_OP_MEMBERSHIP && o.count >= 1 && o.count <= G16_MAX_SET;
        return counts && vst_span_inside(o.list_off, o.count, n_lists);
    };
    uint64_t lo = ~0ull, hi = 0;
    for (uint64_t j = 0; j < m; j++) if (bears(ops[j])) {
        if (ops[j].list_off < lo) lo = ops[j].list_off;
        if (ops[j].list_off + ops[j].count > hi) hi = ops[j].list_off + ops[j].count;
    }
    if (hi == 0) lo = 0;
    for (uint64_t j = 0; j < m; j++) { out[j] = ops[j]; out[j].list_off = bears(ops[j]) ? ops[j].list_off - lo : ~0ull; }
    return VstListSpan{lo, hi - lo};
}

}  // namespace zkp
