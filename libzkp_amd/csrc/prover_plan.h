// The workspace plans of the two provers' host paths: where every device array of a call lies in the slot's grow-only buffer, and the binders
// that put a planned block's arrays into the kernels' views.  Pure functions from sizes to byte offsets.  No HIP call and no HIP header:
// compiled into the library (zkp_hip.hip, g16_impl.inc) and for the host by tests/emul/emul_prover_plan.cpp.
//
// A block is a sequence of regions taken in the order below from its offset 0, each padded to 256 bytes (plan_take.h); `total` is the sum of
// the padded sizes.  Sizes in bytes; S = 32M is one scalar slot ([8][M] words) and D = DIGW*4*M one digit slot of all M jobs.
//
// RANGE / THRESHOLD / CONSISTENCY PROVER, M jobs and C commitment tasks (bp_prove_plan; JobBuf, BpView, CtView, ReduceView of bp_steps.h).
// max_chunks: the most chunks of any of the shard's proof launches; ct_chunks: those of the commitment launch.
//   flag 256 (offset 0 whatever the sizes: the any-failed word of the device-pointer entry point)
//   the job arrays   v 8M | seed_ix 4M | proof_ix 4M | bl_plus 4M | bl_minus 4M | kind M | proof_off 8M | commit_off 8M |
//                    ct_v 8C | ct_seed_ix 4C | ct_bl_ix 4C | ct_off 8C
//   the proofs' work tape S*TAPE_SLOTS | gamma S | d1 D*P1_NSLOTS | d2 D*P2_NSLOTS | dr D*PR_NSLOTS | yinvpow S*64 | ypq S*32 | r0 S*64 |
//                    r1 S*64 | pp S*192 | ab S*256 | gh S*128 | scal S*SC_NUM | tstate 4*52*M | enc S*3
//   their sums       partial max_chunks*GE_W*4*M | sums 3*GE_W*4*M      (phase 1 has three targets)
//   the commitments  ct_digits 2*DIGW*4*C | ct_partial ct_chunks*GE_W*4*C | ct_enc 32C | ct_sums GE_W*4*C      (one target)
// GROTH16 PROVER, `rows` proofs of a circuit with nv variables and domain size m, digw digit words per scalar, and the chunk counts of its
// three launches A/B1, l/h and B2 (g16_prove_plan; G16View of g16_steps.h), nsc = nv + m + 3 scalars:
//   z 32*rows*nv | sdig digw*4*rows*nsc | rs 32*rows*2 | p1 nchunks_ab*G1_JAC_W*4*rows | p1c nchunks_c*G1_JAC_W*4*rows |
//   p2 nchunks_g2*G2_JAC_W*4*rows | s1 3*G1_JAC_W*4*rows (A, B1, the l/h part of C) | s2 G2_JAC_W*4*rows | t1 G16_CPARTS*G1_JAC_W*4*rows |
//   qe 3*36*m*rows (a, b, c: m nine-limb elements per row)
#pragma once
#include "bp_steps.h"
#include "g16_steps.h"
#include "plan_take.h"

namespace zkp {

struct BpProvePlan { size_t flag, v, seed_ix, proof_ix, bl_plus, bl_minus, kind, proof_off, commit_off, ct_v, ct_seed_ix, ct_bl_ix, ct_off, tape, gamma, d1, d2, dr, yinvpow, ypq, r0, r1, pp, ab, gh, scal, tstate, enc, partial, sums, ct_digits, ct_partial, ct_enc, ct_sums, total; };
inline BpProvePlan bp_prove_plan(uint32_t M, uint32_t C, uint32_t max_chunks, uint32_t ct_chunks) {
    PlanTake take; BpProvePlan P{};
    const size_t S = (size_t)8 * 4 * M, D = (size_t)DIGW * 4 * M; P.flag = take(256);
    P.v = take(8ull * M); P.seed_ix = take(4ull * M); P.proof_ix = take(4ull * M); P.bl_plus = take(4ull * M); P.bl_minus = take(4ull * M); P.kind = take(M); P.proof_off = take(8ull * M); P.commit_off = take(8ull * M);
    P.ct_v = take(8ull * C); P.ct_seed_ix = take(4ull * C); P.ct_bl_ix = take(4ull * C); P.ct_off = take(8ull * C);
    P.tape = take(S * TAPE_SLOTS); P.gamma = take(S); P.d1 = take(D * P1_NSLOTS); P.d2 = take(D * P2_NSLOTS); P.dr = take(D * PR_NSLOTS);
    P.yinvpow = take(S * 64); P.ypq = take(S * 32); P.r0 = take(S * 64); P.r1 = take(S * 64); P.pp = take(S * 192); P.ab = take(S * 256); P.gh = take(S * 128);
    P.scal = take(S * SC_NUM); P.tstate = take(4ull * 52 * M); P.enc = take(S * 3); P.partial = take((size_t)max_chunks * GE_W * 4 * M); P.sums = take((size_t)3 * GE_W * 4 * M);
    P.ct_digits = take((size_t)2 * DIGW * 4 * C); P.ct_partial = take((size_t)ct_chunks * GE_W * 4 * C); P.ct_enc = take((size_t)8 * 4 * C); P.ct_sums = take((size_t)GE_W * 4 * C);
    P.total = take.off; return P;
}
// what the prover's launches read of one workspace: the job arrays, the two views over them, and the arrays only the launchers see
struct Ws { JobBuf J; BpView V; CtView T; uint32_t *partial, *ct_partial, *ct_enc, *sums, *ct_sums; uint64_t* ct_off; int* flag; };
// A planned block at `base` into w: every array pointer, the counts the arrays are strided by (the TRUE M and C of the call, which may be 0
// where the plan was made for 1) and the digit radix.  n, lg, seeds and out of the views are the caller's.
inline void bp_prove_bind(Ws& w, uint8_t* base, const BpProvePlan& P, uint32_t M, uint32_t C, uint32_t wbits) {
    JobBuf& J = w.J; BpView& V = w.V; CtView& T = w.T;
    J.v = (uint64_t*)(base + P.v); J.seed_ix = (uint32_t*)(base + P.seed_ix); J.proof_ix = (uint32_t*)(base + P.proof_ix); J.bl_plus = (int32_t*)(base + P.bl_plus); J.bl_minus = (int32_t*)(base + P.bl_minus);
    J.kind = base + P.kind; J.proof_off = (uint64_t*)(base + P.proof_off); J.commit_off = (uint64_t*)(base + P.commit_off);
    J.ct_v = (uint64_t*)(base + P.ct_v); J.ct_seed_ix = (uint32_t*)(base + P.ct_seed_ix); J.ct_bl_ix = (uint32_t*)(base + P.ct_bl_ix); J.ct_off = (uint64_t*)(base + P.ct_off);
    V.M = M; V.wbits = wbits; V.v = J.v; V.seed_ix = J.seed_ix; V.proof_ix = J.proof_ix; V.bl_plus = J.bl_plus; V.bl_minus = J.bl_minus; V.kind = J.kind; V.proof_off = J.proof_off; V.commit_off = J.commit_off;
    auto words = [&](size_t off) { return (uint32_t*)(base + off); };
    V.tape = words(P.tape); V.gamma = words(P.gamma); V.d1 = words(P.d1); V.d2 = words(P.d2); V.dr = words(P.dr); V.yinvpow = words(P.yinvpow); V.ypq = words(P.ypq);
    V.r0 = words(P.r0); V.r1 = words(P.r1); V.pp = words(P.pp); V.ab = words(P.ab); V.gh = words(P.gh); V.scal = words(P.scal); V.tstate = words(P.tstate); V.enc = words(P.enc);
    T.C = C; T.wbits = wbits; T.v = J.ct_v; T.seed_ix = J.ct_seed_ix; T.bl_ix = J.ct_bl_ix; T.digits = words(P.ct_digits);
    w.partial = words(P.partial); w.sums = words(P.sums); w.ct_partial = words(P.ct_partial); w.ct_enc = words(P.ct_enc); w.ct_sums = words(P.ct_sums); w.ct_off = J.ct_off; w.flag = (int*)(base + P.flag);
}

struct G16ProvePlan { size_t z, sdig, rs, p1, p1c, p2, s1, s2, t1, qe, total; };
inline G16ProvePlan g16_prove_plan(uint32_t rows, uint32_t nv, uint32_t m, uint32_t digw, uint32_t nchunks_ab, uint32_t nchunks_c, uint32_t nchunks_g2) {
    PlanTake take; G16ProvePlan P{}; const size_t W = (size_t)32 * rows;
    P.z = take(W * nv); P.sdig = take((size_t)digw * 4 * rows * g16_nscalars(nv, m)); P.rs = take(W * 2);
    P.p1 = take((size_t)nchunks_ab * G1_JAC_W * 4 * rows); P.p1c = take((size_t)nchunks_c * G1_JAC_W * 4 * rows); P.p2 = take((size_t)nchunks_g2 * G2_JAC_W * 4 * rows);
    P.s1 = take((size_t)3 * G1_JAC_W * 4 * rows); P.s2 = take((size_t)G2_JAC_W * 4 * rows); P.t1 = take((size_t)G16_CPARTS * G1_JAC_W * 4 * rows); P.qe = take((size_t)3 * 36 * m * rows);
    P.total = take.off; return P;
}
// the view's four workspace arrays of a planned block at `base`; the chunk partials and sums, which only the launchers see, are returned
struct G16ProveBufs { uint32_t *p1, *p1c, *p2, *s1, *s2, *t1; };
inline G16ProveBufs g16_prove_bind(G16View& V, uint8_t* base, const G16ProvePlan& P) {
    auto words = [&](size_t off) { return (uint32_t*)(base + off); };
    V.z = words(P.z); V.sdig = words(P.sdig); V.rs = words(P.rs); V.qap_evals = words(P.qe);
    return {words(P.p1), words(P.p1c), words(P.p2), words(P.s1), words(P.s2), words(P.t1)};
}

}  // namespace zkp
