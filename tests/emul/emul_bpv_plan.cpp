// TEST INFRASTRUCTURE: host build of the Bulletproofs verifier's workspace plan (bpv_plan.h): the plan functions as rows of 64-bit words and
// the binder over a view whose every field holds a marker, given a fake base address (nothing is dereferenced).  Loaded by
// tests/test_emul_bpv_plan.py as a shared library.  Not part of the product library.
#include "../../libzkp_amd/csrc/bpv_plan.h"
using namespace zkp;

namespace {
// a job-array plan as JOB_WORDS words: nchunks, chunk_table[0], chunk_table[1], then the offsets in the order of the struct
constexpr uint32_t JOB_WORDS = 18;
uint64_t* jobs_out(const BpvJobArrays& J, uint64_t* o) {
    const uint64_t row[JOB_WORDS] = {J.nchunks, J.chunk_table[0], J.chunk_table[1], J.poff, J.voff, J.kind, J.lgn, J.bad, J.pts, J.scal, J.zero0, J.digits, J.vscal, J.zero1,
                                     J.partial, J.sums, J.enc, J.tcb};
    for (uint32_t i = 0; i < JOB_WORDS; i++) o[i] = row[i];
    return o + JOB_WORDS;
}
}  // namespace

extern "C" {
void emul_bpv_constants(uint32_t out[10]) {
    out[0] = VP_NUM; out[1] = VS_NUM; out[2] = NBASE; out[3] = DIGW; out[4] = GE_W; out[5] = RLC_NWIN; out[6] = RLC_NBUCKET; out[7] = RLC_NSEG; out[8] = RLC_NIELS_W; out[9] = JOB_WORDS;
}
// job_base, env_bad | the job arrays | rho, fterm, count, rzero1, niels, dig, start, cursor, sorted, bucket, seg, dig1, part1, sum1, result | total: 2 + 18 + 15 + 1 words
void emul_bpv_plan_batch(uint64_t n, uint32_t Mw, uint32_t nchunks, int batch_mode, uint32_t nchunks1, uint64_t* out) {
    const BpvBatchPlan P = bpv_plan_batch(n, Mw, nchunks, batch_mode != 0, nchunks1);
    out[0] = P.job_base; out[1] = P.env_bad;
    uint64_t* o = jobs_out(P.J, out + 2);
    const uint64_t row[16] = {P.rho, P.fterm, P.count, P.rzero1, P.niels, P.dig, P.start, P.cursor, P.sorted, P.bucket, P.seg, P.dig1, P.part1, P.sum1, P.result, P.total};
    for (int i = 0; i < 16; i++) o[i] = row[i];
}
// dig, part, gen, win, suspect, total
void emul_bpv_plan_segments(uint32_t count, uint32_t nchunks, uint64_t out[6]) {
    const BpvSegmentPlan P = bpv_plan_segments(count, nchunks);
    out[0] = P.dig; out[1] = P.part; out[2] = P.gen; out[3] = P.win; out[4] = P.suspect; out[5] = P.total;
}
// suspect, off | the job arrays | total: 2 + 18 + 1 words
void emul_bpv_plan_compact(uint32_t count, uint32_t Mc, uint32_t nchunks, uint64_t* out) {
    const BpvCompactPlan P = bpv_plan_compact(count, Mc, nchunks);
    out[0] = P.suspect; out[1] = P.off;
    *jobs_out(P.J, out + 2) = P.total;
}
// bpv_bind_jobs at `base` with the job arrays of M jobs taken behind `lead` bytes of other regions, into a view whose fields hold
// marker + their index in `view`: M, in, proof_off, venc_off, kind, lgn, bad, pts, scal, digits, vscal, partial, var_chunk0, table, wbits, rho,
// fterm, job_base, env_bad (19 words).  plan: the job arrays the binder was given.
void emul_bpv_bind(uint64_t base, uint64_t lead, uint32_t M, uint32_t nchunks, uint64_t marker, uint64_t* plan, uint64_t* view) {
    BpvTake take; take(lead);
    const BpvJobArrays J = bpv_plan_jobs(take, M, nchunks);
    jobs_out(J, plan);
    auto mk = [&](uint64_t i) { return (uintptr_t)(marker + i); };
    VfyView V{};
    V.M = (uint32_t)mk(0); V.in = (const uint8_t*)mk(1); V.proof_off = (uint64_t*)mk(2); V.venc_off = (uint64_t*)mk(3); V.kind = (uint8_t*)mk(4); V.lgn = (uint8_t*)mk(5);
    V.bad = (int32_t*)mk(6); V.pts = (uint32_t*)mk(7); V.scal = (uint32_t*)mk(8); V.digits = (uint32_t*)mk(9); V.vscal = (uint32_t*)mk(10); V.partial = (uint32_t*)mk(11);
    V.var_chunk0 = (uint32_t)mk(12); V.table = (const uint32_t*)mk(13); V.wbits = (uint32_t)mk(14); V.rho = (const uint32_t*)mk(15); V.fterm = (uint32_t*)mk(16);
    V.job_base = (const uint32_t*)mk(17); V.env_bad = (int32_t*)mk(18);
    bpv_bind_jobs(V, (uint8_t*)(uintptr_t)base, J);
    const uint64_t row[19] = {V.M, (uintptr_t)V.in, (uintptr_t)V.proof_off, (uintptr_t)V.venc_off, (uintptr_t)V.kind, (uintptr_t)V.lgn, (uintptr_t)V.bad, (uintptr_t)V.pts,
                              (uintptr_t)V.scal, (uintptr_t)V.digits, (uintptr_t)V.vscal, (uintptr_t)V.partial, V.var_chunk0, (uintptr_t)V.table, V.wbits, (uintptr_t)V.rho,
                              (uintptr_t)V.fterm, (uintptr_t)V.job_base, (uintptr_t)V.env_bad};
    for (int i = 0; i < 19; i++) view[i] = row[i];
}
}
