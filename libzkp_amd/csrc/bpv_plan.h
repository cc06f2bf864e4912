// The workspace plan of the Bulletproofs verifier's host path (bpv_impl.inc: verify_bp_device, localise_bp): where every device array of a
// call lies in the shard's two grow-only buffers.  Pure functions from sizes to byte offsets, and the binder that puts a planned block's job
// arrays into a VfyView.  No HIP call and no HIP header: compiled into the library and for the host by tests/emul/emul_bpv_plan.cpp.
//
// Every block is a sequence of regions taken in the order below from the block's offset 0, each padded to 256 bytes; `total` is the sum of
// the padded sizes, and every offset in a plan is relative to the block's start.
//
// JOB ARRAYS of M jobs walked with a layout of nchunks fixed-base chunks (bpv_plan_jobs; VfyView and ReduceView, bp_verify.h / bp_steps.h):
//   poff 8M | voff 8M | kind M | lgn M | bad 4M | pts VP_NUM*GE_W*4*M | scal VS_NUM*32*M | digits NBASE*DIGW*4*M | vscal VP_NUM*32*M |
//   partial (nchunks + VP_NUM)*GE_W*4*M | sums GE_W*4*M | enc 32M | tcb 4
//   [zero0, zero1) = digits u vscal, contiguous: what a call zeroes before a per-job or weighted pass (a rejected job contributes nothing).
//   tcb holds chunk_table = {0, nchunks + VP_NUM}: the one target of the per-job pass sums the fixed chunks and the 17 proof-point products.
// BATCH BLOCK of n envelopes (bpv_plan_batch; VfyState::buf), Mw = max(M, 1), N = VP_NUM * Mw, nchunks1 = the one-row layout's chunks:
//   job_base 4(n + 1) | env_bad 4n | the job arrays of Mw jobs
//   batch mode (the check's regions, RlcView; without it they take no space and their offsets are 0):
//   | rho 32Mw | fterm NBASE*32*Mw | count RLC_NWIN*(RLC_NBUCKET + 1)*4 | niels N*RLC_NIELS_W*4 | dig RLC_NWIN*N*2 |
//   start RLC_NWIN*(RLC_NBUCKET + 2)*4 | cursor RLC_NWIN*(RLC_NBUCKET + 1)*4 | sorted RLC_NWIN*N*4 | bucket RLC_NWIN*RLC_NBUCKET*GE_W*4 |
//   seg RLC_NWIN*RLC_NSEG*GE_W*4 | dig1 NBASE*DIGW*4 | part1 nchunks1*GE_W*4 | sum1 GE_W*4 | result 64
//   [fterm, rzero1) = fterm u count, contiguous: zeroed before the weighted pass.
// LOCALISATION BLOCK (VfyState::loc), two shapes one after the other over the same buffer, both from offset 0:
//   segment checks of `count` segments, nchunks = their layout's (bpv_plan_segments):
//     dig NBASE*DIGW*4*count | part nchunks*GE_W*4*count | gen GE_W*4*count | win count*RLC_NWIN*GE_W*4 | suspect count
//   the suspects' Mc jobs, compacted (bpv_plan_compact):  suspect count | off 4(count + 1) | the job arrays of Mc jobs
#pragma once
#include "bp_verify.h"
#include "plan_take.h"

namespace zkp {

using BpvTake = PlanTake;      // the helper's name before it moved to plan_take.h: host units written against this header keep compiling

struct BpvJobArrays { uint32_t nchunks; uint16_t chunk_table[2]; size_t poff, voff, kind, lgn, bad, pts, scal, zero0, digits, vscal, zero1, partial, sums, enc, tcb; };
inline BpvJobArrays bpv_plan_jobs(PlanTake& take, uint32_t M, uint32_t nchunks) {
    BpvJobArrays J{}; J.nchunks = nchunks; J.chunk_table[1] = (uint16_t)(nchunks + VP_NUM);
    J.poff = take(8ull * M); J.voff = take(8ull * M); J.kind = take(M); J.lgn = take(M); J.bad = take(4ull * M);
    J.pts = take((size_t)VP_NUM * GE_W * 4 * M); J.scal = take((size_t)VS_NUM * 32 * M);
    J.zero0 = take.off; J.digits = take((size_t)NBASE * DIGW * 4 * M); J.vscal = take((size_t)VP_NUM * 32 * M); J.zero1 = take.off;
    J.partial = take((size_t)(nchunks + VP_NUM) * GE_W * 4 * M); J.sums = take((size_t)GE_W * 4 * M); J.enc = take((size_t)32 * M); J.tcb = take(4);
    return J;
}
// the job arrays of a planned block at `base` into a view: every array pointer a job-array plan owns, and where the proof-point products go
inline void bpv_bind_jobs(VfyView& V, uint8_t* base, const BpvJobArrays& J) {
    V.proof_off = (uint64_t*)(base + J.poff); V.venc_off = (uint64_t*)(base + J.voff); V.kind = base + J.kind; V.lgn = base + J.lgn; V.bad = (int32_t*)(base + J.bad);
    V.pts = (uint32_t*)(base + J.pts); V.scal = (uint32_t*)(base + J.scal); V.digits = (uint32_t*)(base + J.digits); V.vscal = (uint32_t*)(base + J.vscal);
    V.partial = (uint32_t*)(base + J.partial); V.var_chunk0 = J.nchunks;
}

struct BpvBatchPlan { size_t job_base, env_bad; BpvJobArrays J; size_t rho, fterm, count, rzero1, niels, dig, start, cursor, sorted, bucket, seg, dig1, part1, sum1, result, total; };
inline BpvBatchPlan bpv_plan_batch(uint64_t n, uint32_t Mw, uint32_t nchunks, bool batch_mode, uint32_t nchunks1) {
    PlanTake take; BpvBatchPlan P{};
    P.job_base = take(4 * (n + 1)); P.env_bad = take(4 * n); P.J = bpv_plan_jobs(take, Mw, nchunks);
    if (batch_mode) {
        const size_t N = (size_t)VP_NUM * Mw;
        P.rho = take(32ull * Mw); P.fterm = take((size_t)NBASE * 32 * Mw); P.count = take((size_t)RLC_NWIN * (RLC_NBUCKET + 1) * 4); P.rzero1 = take.off;
        P.niels = take(N * RLC_NIELS_W * 4); P.dig = take(RLC_NWIN * N * 2); P.start = take((size_t)RLC_NWIN * (RLC_NBUCKET + 2) * 4);
        P.cursor = take((size_t)RLC_NWIN * (RLC_NBUCKET + 1) * 4); P.sorted = take(RLC_NWIN * N * 4);
        P.bucket = take((size_t)RLC_NWIN * RLC_NBUCKET * GE_W * 4); P.seg = take((size_t)RLC_NWIN * RLC_NSEG * GE_W * 4);
        P.dig1 = take((size_t)NBASE * DIGW * 4); P.part1 = take((size_t)nchunks1 * GE_W * 4); P.sum1 = take((size_t)GE_W * 4); P.result = take(64);
    }
    P.total = take.off; return P;
}

struct BpvSegmentPlan { size_t dig, part, gen, win, suspect, total; };
inline BpvSegmentPlan bpv_plan_segments(uint32_t count, uint32_t nchunks) {
    PlanTake take; BpvSegmentPlan P{};
    P.dig = take((size_t)NBASE * DIGW * 4 * count); P.part = take((size_t)nchunks * GE_W * 4 * count); P.gen = take((size_t)GE_W * 4 * count);
    P.win = take((size_t)count * RLC_NWIN * GE_W * 4); P.suspect = take(count);
    P.total = take.off; return P;
}
struct BpvCompactPlan { size_t suspect, off; BpvJobArrays J; size_t total; };
inline BpvCompactPlan bpv_plan_compact(uint32_t count, uint32_t Mc, uint32_t nchunks) {
    PlanTake take; BpvCompactPlan P{};
    P.suspect = take(count); P.off = take(4ull * (count + 1)); P.J = bpv_plan_jobs(take, Mc, nchunks);
    P.total = take.off; return P;
}

}  // namespace zkp
