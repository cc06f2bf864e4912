// TEST INFRASTRUCTURE: host build of the staging plan of a mixed batch (batch_plan.h): plan_shards, plan_stage_layout and fill_stage_image
// over plain arrays.  Loaded by tests/test_emul_batch_plan.py as a shared library; as a program of its own (it has a main) it stages a batch
// of all six kinds on two shards, flagged and unflagged, into buffers of exactly the planned size, which is the form to build with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../libzkp_amd/csrc/batch_plan.h"
using namespace zkp;

namespace {
StagePlan g_plan;          // the plan of the last emul_bp_plan call; emul_bp_fill and emul_bp_product go on from it
template <class T> uint64_t copy_out(const std::vector<T>& v, void* dst) {
    if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T));
    return v.size() * sizeof(T);
}
// a job list as rows of eight / a commitment task list as rows of four 64-bit words (signed fields sign-extended)
uint64_t jobs_out(const HostJobs& H, uint64_t* dst) {
    for (size_t i = 0; dst && i < H.v.size(); i++) {
        const uint64_t row[8] = {H.v[i], H.seed_ix[i], H.proof_ix[i], (uint64_t)(int64_t)H.bl_plus[i], (uint64_t)(int64_t)H.bl_minus[i], H.kind[i], H.proof_off[i], H.commit_off[i]};
        memcpy(dst + 8 * i, row, sizeof row);
    }
    return 64 * H.v.size();
}
uint64_t commits_out(const HostJobs& H, uint64_t* dst) {
    for (size_t i = 0; dst && i < H.ct_v.size(); i++) {
        const uint64_t row[4] = {H.ct_v[i], H.ct_seed_ix[i], H.ct_bl_ix[i], H.ct_off[i]};
        memcpy(dst + 4 * i, row, sizeof row);
    }
    return 32 * H.ct_v.size();
}
}  // namespace

extern "C" {
uint32_t emul_bp_layout_words(void) { return 4 + 4 * SC_KINDS + 21 + 7 + 2 + 3; }
void emul_bp_plan_shards(uint64_t n, const zkp_hip_op* ops, uint32_t shards, uint32_t* shard_of_op) { plan_shards(n, ops, shards, shard_of_op); }
// plan_stage_layout of the shard that holds the ops gidx[0 .. n).  layout (emul_bp_layout_words() words): max_total, in_bytes, arena_bytes,
// meta_bytes | rows, stride, arena, row0 of kinds 0..6 | the 21 offsets of the image in the order of the header's comment | the 7 self-check
// offsets | a_dlen, a_dst | m_off, m_status, m_len.  row_ok: n bytes.
void emul_bp_plan(uint32_t n, const uint32_t* gidx, const zkp_hip_op* ops, const uint64_t* lists, int self_check, uint64_t* layout, uint8_t* row_ok) {
    g_plan = StagePlan();
    StagePlan& P = g_plan;
    P.n = n; P.gidx.assign(gidx, gidx + n);
    plan_stage_layout(P, ops, lists, self_check != 0);
    uint64_t* w = layout;
    *w++ = P.max_total; *w++ = P.in_bytes; *w++ = P.arena_bytes; *w++ = P.meta_bytes;
    for (const VariantPlan& v : P.var) { *w++ = v.rows; *w++ = v.stride; *w++ = v.arena; *w++ = v.row0; }
    for (size_t o : {P.i_rv, P.i_rmin, P.i_rmax, P.i_rseed, P.i_ev, P.i_eseed, P.i_mv, P.i_msets, P.i_mlen, P.i_mseed, P.i_io, P.i_in, P.i_tseed, P.i_cseed, P.i_ccount, P.i_clen,
                     P.i_src, P.i_lenf, P.i_dix, P.i_dkind, P.i_stf, P.i_thr, P.i_var, P.i_rlen, P.i_rop, P.i_rok, P.i_oprow, P.i_cnt, P.a_dlen, P.a_dst, P.m_off, P.m_status, P.m_len}) *w++ = o;
    copy_out(P.row_ok, row_ok);
}
// fill_stage_image of the shard planned last into image (in_bytes of that plan; the caller's bytes stay where nothing is written)
void emul_bp_fill(const zkp_hip_op* ops, const uint64_t* lists, const uint8_t* seeds, uint8_t* image) { fill_stage_image(g_plan, ops, lists, seeds, image); }
// what the fill left beside the image: 0 thr_img, 1 con_img, 2 con_counts, 3 con_lens, 4 op_variant, 5 / 6 the threshold framing's jobs /
// commitment tasks, 7 / 8 the consistency framing's.  Returns the size in bytes; dst may be null.
uint64_t emul_bp_product(uint32_t which, void* dst) {
    const StagePlan& P = g_plan;
    switch (which) {
        case 0: return copy_out(P.thr_img, dst);
        case 1: return copy_out(P.con_img, dst);
        case 2: return copy_out(P.con_counts, dst);
        case 3: return copy_out(P.con_lens, dst);
        case 4: return copy_out(P.op_variant, dst);
        case 5: return jobs_out(P.thrJ, (uint64_t*)dst);
        case 6: return commits_out(P.thrJ, (uint64_t*)dst);
        case 7: return jobs_out(P.conJ, (uint64_t*)dst);
        case 8: return commits_out(P.conJ, (uint64_t*)dst);
        default: return 0;
    }
}
}

int main() {
    // two of every kind, interleaved, with an op of each host-validated kind refused and lists of different lengths
    std::vector<uint64_t> lists = {5, 6, 7, 1, 2, 3, 4, 9, 9, 8, 1, 2, 2, 5, 7};
    auto op = [](uint32_t kind, uint32_t count, uint64_t a, uint64_t b, uint64_t c, uint64_t list_off) { zkp_hip_op o; o.kind = kind; o.count = count; o.a = a; o.b = b; o.c = c; o.list_off = list_off; return o; };
    std::vector<zkp_hip_op> ops = {
        op(ZKP_HIP_OP_RANGE, 0, 5, 0, 10, 0), op(ZKP_HIP_OP_EQUALITY, 0, 7, 7, 0, 0), op(ZKP_HIP_OP_THRESHOLD, 3, 10, 0, 0, 0), op(ZKP_HIP_OP_MEMBERSHIP, 4, 3, 0, 0, 3),
        op(ZKP_HIP_OP_IMPROVEMENT, 0, 1, 2, 0, 0), op(ZKP_HIP_OP_CONSISTENCY, 5, 0, 0, 0, 10), op(ZKP_HIP_OP_RANGE, 0, 50, 0, 10, 0), op(ZKP_HIP_OP_EQUALITY, 0, 7, 8, 0, 0),
        op(ZKP_HIP_OP_THRESHOLD, 0, 1, 0, 0, 0), op(ZKP_HIP_OP_MEMBERSHIP, 2, 77, 0, 0, 7), op(ZKP_HIP_OP_IMPROVEMENT, 0, 2, 2, 0, 0), op(ZKP_HIP_OP_CONSISTENCY, 3, 0, 0, 0, 7)};
    const uint32_t n = (uint32_t)ops.size();
    std::vector<uint8_t> seeds(32 * n);
    for (size_t i = 0; i < seeds.size(); i++) seeds[i] = (uint8_t)(i * 7 + 1);
    int failures = 0;
    for (uint32_t shards : {1u, 2u}) for (int flagged = 0; flagged < 2; flagged++) {
        std::vector<zkp_hip_op> o = ops;
        if (flagged) for (auto& x : o) x.kind |= ZKP_HIP_OP_SELF_CHECK;
        std::vector<uint32_t> owner(n);
        plan_shards(n, o.data(), shards, owner.data());
        uint64_t total = 0, expect = 0;
        for (const auto& x : o) expect += op_max_bytes(x);
        for (uint32_t s = 0; s < shards; s++) {
            StagePlan P;
            for (uint32_t i = 0; i < n; i++) if (owner[i] == s) P.gidx.push_back(i);
            P.n = (uint32_t)P.gidx.size();
            plan_stage_layout(P, o.data(), lists.data(), flagged != 0);
            uint8_t* image = (uint8_t*)std::malloc(P.in_bytes ? P.in_bytes : 1);          // exactly the planned size: a write beyond it is the sanitizer's to find
            fill_stage_image(P, o.data(), lists.data(), seeds.data(), image);
            total += P.max_total;
            if (P.in_bytes % 256 || P.arena_bytes % 256 || P.meta_bytes % 256 || P.thr_img.size() != P.var[ZKP_HIP_OP_THRESHOLD].stride * P.var[ZKP_HIP_OP_THRESHOLD].rows) failures++;
            std::free(image);
        }
        if (total != expect) failures++;
    }
    if (failures) { std::fprintf(stderr, "emul_batch_plan: %d failure(s)\n", failures); return 1; }
    std::printf("emul_batch_plan ok\n");
    return 0;
}
