// TEST INFRASTRUCTURE: host build of the two provers' workspace plans (prover_plan.h): the plan functions as rows of 64-bit words and both
// binders over views whose every field holds a marker, given a fake base address (nothing is dereferenced).  Loaded by
// tests/test_emul_prover_plan.py as a shared library.  Not part of the product library.
#include "../../libzkp_amd/csrc/prover_plan.h"
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/g16_share.h"
using namespace zkp;

namespace {
constexpr uint32_t BP_WORDS = 35, G16_WORDS = 11, WS_WORDS = 55, G16_VIEW_WORDS = 25;
uint64_t ptr(const void* p) { return (uint64_t)(uintptr_t)p; }
}  // namespace

extern "C" {
// the sizes the header's formulas name, and the (nv, m) of the two shipped circuits
void emul_pp_constants(uint32_t out[18]) {
    const G16KeyShape eq = g16_key_shape(build_equality_r1cs()), mb = g16_key_shape(build_membership_r1cs());
    const uint32_t row[18] = {TAPE_SLOTS, P1_NSLOTS, P2_NSLOTS, PR_NSLOTS, SC_NUM, DIGW, GE_W, G1_JAC_W, G2_JAC_W, G16_CPARTS, eq.nv, eq.m, mb.nv, mb.m,
                              BP_WORDS, G16_WORDS, WS_WORDS, G16_VIEW_WORDS};
    for (int i = 0; i < 18; i++) out[i] = row[i];
}
// the offsets in the order of the struct (= take order), then total: 35 words
void emul_pp_bp_plan(uint32_t M, uint32_t C, uint32_t max_chunks, uint32_t ct_chunks, uint64_t* out) {
    const BpProvePlan P = bp_prove_plan(M, C, max_chunks, ct_chunks);
    const uint64_t row[BP_WORDS] = {P.flag, P.v, P.seed_ix, P.proof_ix, P.bl_plus, P.bl_minus, P.kind, P.proof_off, P.commit_off, P.ct_v, P.ct_seed_ix, P.ct_bl_ix, P.ct_off,
                                    P.tape, P.gamma, P.d1, P.d2, P.dr, P.yinvpow, P.ypq, P.r0, P.r1, P.pp, P.ab, P.gh, P.scal, P.tstate, P.enc, P.partial, P.sums,
                                    P.ct_digits, P.ct_partial, P.ct_enc, P.ct_sums, P.total};
    for (uint32_t i = 0; i < BP_WORDS; i++) out[i] = row[i];
}
// z, sdig, rs, p1, p1c, p2, s1, s2, t1, qe, total: 11 words
void emul_pp_g16_plan(uint32_t rows, uint32_t nv, uint32_t m, uint32_t digw, uint32_t nchunks_ab, uint32_t nchunks_c, uint32_t nchunks_g2, uint64_t* out) {
    const G16ProvePlan P = g16_prove_plan(rows, nv, m, digw, nchunks_ab, nchunks_c, nchunks_g2);
    const uint64_t row[G16_WORDS] = {P.z, P.sdig, P.rs, P.p1, P.p1c, P.p2, P.s1, P.s2, P.t1, P.qe, P.total};
    for (uint32_t i = 0; i < G16_WORDS; i++) out[i] = row[i];
}
// bp_prove_bind at `base` of the plan of (pm, pc, max_chunks, ct_chunks) for M jobs and C tasks, into a Ws whose fields hold marker + their
// index in `view` (55 words):
//   J: v seed_ix proof_ix bl_plus bl_minus kind proof_off commit_off ct_v ct_seed_ix ct_bl_ix ct_off
//   V: M n lg wbits v seed_ix proof_ix bl_plus bl_minus kind seeds proof_off commit_off out tape gamma d1 d2 dr yinvpow ypq r0 r1 pp ab gh scal tstate enc
//   T: C v seed_ix bl_ix seeds digits wbits
//   partial ct_partial ct_enc sums ct_sums ct_off flag
void emul_pp_bp_bind(uint64_t base, uint32_t pm, uint32_t pc, uint32_t max_chunks, uint32_t ct_chunks, uint32_t M, uint32_t C, uint32_t wbits, uint64_t marker, uint64_t* view) {
    uint64_t i = 0;
    auto mk = [&]() { return (uintptr_t)(marker + i++); };
    Ws w{}; JobBuf& J = w.J; BpView& V = w.V; CtView& T = w.T;
    J.v = (uint64_t*)mk(); J.seed_ix = (uint32_t*)mk(); J.proof_ix = (uint32_t*)mk(); J.bl_plus = (int32_t*)mk(); J.bl_minus = (int32_t*)mk(); J.kind = (uint8_t*)mk();
    J.proof_off = (uint64_t*)mk(); J.commit_off = (uint64_t*)mk(); J.ct_v = (uint64_t*)mk(); J.ct_seed_ix = (uint32_t*)mk(); J.ct_bl_ix = (uint32_t*)mk(); J.ct_off = (uint64_t*)mk();
    V.M = (uint32_t)mk(); V.n = (uint32_t)mk(); V.lg = (uint32_t)mk(); V.wbits = (uint32_t)mk();
    V.v = (const uint64_t*)mk(); V.seed_ix = (const uint32_t*)mk(); V.proof_ix = (const uint32_t*)mk(); V.bl_plus = (const int32_t*)mk(); V.bl_minus = (const int32_t*)mk();
    V.kind = (const uint8_t*)mk(); V.seeds = (const uint32_t*)mk(); V.proof_off = (const uint64_t*)mk(); V.commit_off = (const uint64_t*)mk(); V.out = (uint8_t*)mk();
    for (uint32_t** f : {&V.tape, &V.gamma, &V.d1, &V.d2, &V.dr, &V.yinvpow, &V.ypq, &V.r0, &V.r1, &V.pp, &V.ab, &V.gh, &V.scal, &V.tstate, &V.enc}) *f = (uint32_t*)mk();
    T.C = (uint32_t)mk(); T.v = (const uint64_t*)mk(); T.seed_ix = (const uint32_t*)mk(); T.bl_ix = (const uint32_t*)mk(); T.seeds = (const uint32_t*)mk();
    T.digits = (uint32_t*)mk(); T.wbits = (uint32_t)mk();
    for (uint32_t** f : {&w.partial, &w.ct_partial, &w.ct_enc, &w.sums, &w.ct_sums}) *f = (uint32_t*)mk();
    w.ct_off = (uint64_t*)mk(); w.flag = (int*)mk();
    bp_prove_bind(w, (uint8_t*)(uintptr_t)base, bp_prove_plan(pm, pc, max_chunks, ct_chunks), M, C, wbits);
    const uint64_t row[WS_WORDS] = {
        ptr(J.v), ptr(J.seed_ix), ptr(J.proof_ix), ptr(J.bl_plus), ptr(J.bl_minus), ptr(J.kind), ptr(J.proof_off), ptr(J.commit_off), ptr(J.ct_v), ptr(J.ct_seed_ix), ptr(J.ct_bl_ix), ptr(J.ct_off),
        V.M, V.n, V.lg, V.wbits, ptr(V.v), ptr(V.seed_ix), ptr(V.proof_ix), ptr(V.bl_plus), ptr(V.bl_minus), ptr(V.kind), ptr(V.seeds), ptr(V.proof_off), ptr(V.commit_off), ptr(V.out),
        ptr(V.tape), ptr(V.gamma), ptr(V.d1), ptr(V.d2), ptr(V.dr), ptr(V.yinvpow), ptr(V.ypq), ptr(V.r0), ptr(V.r1), ptr(V.pp), ptr(V.ab), ptr(V.gh), ptr(V.scal), ptr(V.tstate), ptr(V.enc),
        T.C, ptr(T.v), ptr(T.seed_ix), ptr(T.bl_ix), ptr(T.seeds), ptr(T.digits), T.wbits,
        ptr(w.partial), ptr(w.ct_partial), ptr(w.ct_enc), ptr(w.sums), ptr(w.ct_sums), ptr(w.ct_off), ptr(w.flag)};
    for (uint32_t k = 0; k < WS_WORDS; k++) view[k] = row[k];
}
// g16_prove_bind at `base` into a view whose fields hold marker + their index in `view` (25 words):
//   rows kind rx.wbits rx.digw n_inst n_wit nv m value set_vals set_len seeds mimc_c z sdig rs qap_evals out stride | the returned p1 p1c p2 s1 s2 t1
void emul_pp_g16_bind(uint64_t base, uint32_t rows, uint32_t nv, uint32_t m, uint32_t digw, uint32_t nchunks_ab, uint32_t nchunks_c, uint32_t nchunks_g2, uint64_t marker, uint64_t* view) {
    uint64_t i = 0;
    auto mk = [&]() { return (uintptr_t)(marker + i++); };
    G16View V{};
    V.rows = (uint32_t)mk(); V.kind = (uint32_t)mk(); V.rx.wbits = (uint32_t)mk(); V.rx.digw = (uint32_t)mk(); V.n_inst = (uint32_t)mk(); V.n_wit = (uint32_t)mk();
    V.nv = (uint32_t)mk(); V.m = (uint32_t)mk(); V.value = (const uint64_t*)mk(); V.set_vals = (const uint64_t*)mk(); V.set_len = (const uint32_t*)mk();
    V.seeds = (const uint32_t*)mk(); V.mimc_c = (const uint32_t*)mk(); V.z = (uint32_t*)mk(); V.sdig = (uint32_t*)mk(); V.rs = (uint32_t*)mk(); V.qap_evals = (uint32_t*)mk();
    V.out = (uint8_t*)mk(); V.stride = mk();
    const G16ProveBufs B = g16_prove_bind(V, (uint8_t*)(uintptr_t)base, g16_prove_plan(rows, nv, m, digw, nchunks_ab, nchunks_c, nchunks_g2));
    const uint64_t row[G16_VIEW_WORDS] = {V.rows, V.kind, V.rx.wbits, V.rx.digw, V.n_inst, V.n_wit, V.nv, V.m, ptr(V.value), ptr(V.set_vals), ptr(V.set_len), ptr(V.seeds), ptr(V.mimc_c),
                                          ptr(V.z), ptr(V.sdig), ptr(V.rs), ptr(V.qap_evals), ptr(V.out), V.stride, ptr(B.p1), ptr(B.p1c), ptr(B.p2), ptr(B.s1), ptr(B.s2), ptr(B.t1)};
    for (uint32_t k = 0; k < G16_VIEW_WORDS; k++) view[k] = row[k];
}
}
