// TEST INFRASTRUCTURE: the planning and the per-lane steps of the Bulletproofs localisation pass (bp_localise.h) on the CPU -- plain loops
// in place of lanes and kernel launches -- and the batch-mode verification steps summed per segment under weights the test chooses.
// Not part of the product library.
#include "../../libzkp_amd/csrc/bp_layout.h"
#include "../../libzkp_amd/csrc/bp_localise.h"
#include "../../libzkp_amd/csrc/edg.h"
#include <vector>
#include <cstring>
using namespace zkp;

static std::vector<uint32_t> g_table;
static void ensure_table() {
    if (!g_table.empty()) return;
    g_table.resize((size_t)NBASE * NWIN * SUBTAB_W);
    ge gens[NBASE]; host_generators(gens);
    for (uint32_t b = 0; b < NBASE; b++) host_build_table_for_base(g_table.data() + (size_t)b * NWIN * SUBTAB_W, gens[b]);
}
// affine-Niels row of a decoded point (Z = 1), as k_rlc_points stores it
static void niels_row(uint32_t* q, const ge& pt) {
    uint32_t w8[8];
    fe_towords(w8, fe_add(pt.Y, pt.X)); const fe ypx = fe_fromwords(w8);
    fe_towords(w8, fe_sub(pt.Y, pt.X)); const fe ymx = fe_fromwords(w8);
    fe_towords(w8, fe_mul(pt.T, fe_const_d2())); const fe xy2d = fe_fromwords(w8);
    for (int k = 0; k < 10; k++) { q[k] = ypx.v[k]; q[10 + k] = ymx.v[k]; q[20 + k] = xy2d.v[k]; }
}
// sum_i d_i P_i of window w over the jobs [j_lo, j_hi): the kernel's walk, its 64 lanes one after the other; *max_run = longest run of a lane in a tile
static ge window_sum(const RlcView& R, uint32_t M, uint32_t w, uint32_t j_lo, uint32_t j_hi, uint32_t* max_run) {
    BpLocTile T; ge B[BP_LOC_LANES];
    for (uint32_t t = 0; t < BP_LOC_LANES; t++) B[t] = ge_identity();
    for (uint32_t j0 = j_lo; j0 < j_hi; j0 += BP_LOC_TILE_JOBS) {
        const uint32_t nj = j_hi - j0 < BP_LOC_TILE_JOBS ? j_hi - j0 : BP_LOC_TILE_JOBS;
        memset(&T, 0xAB, sizeof T);
        for (uint32_t t = 0; t < BP_LOC_LANES; t++) T.cursor[t] = 0;
        for (uint32_t t = 0; t < BP_LOC_LANES; t++) bp_loc_step_sort(T, R, M, w, j0, nj, t, false);
        bp_loc_step_scan(T);
        for (uint32_t t = 0; t < BP_LOC_LANES; t++) bp_loc_step_sort(T, R, M, w, j0, nj, t, true);
        for (uint32_t t = 0; t < BP_LOC_LANES; t++) {
            if (max_run && T.start[t + 1] - T.start[t] > *max_run) *max_run = T.start[t + 1] - T.start[t];
            B[t] = bp_loc_step_walk(B[t], T, R, M, j0, nj, t);
        }
    }
    return bp_loc_combine(B);
}

extern "C" {
void emul_bp_loc_constants(uint32_t out[6]) {
    out[0] = BP_LOC_MAX_SEGMENTS; out[1] = BP_LOC_SEGMENT_QUANTUM; out[2] = BP_LOC_SEGMENT_MIN; out[3] = BP_LOC_TILE_JOBS; out[4] = BP_LOC_TILE_POINTS; out[5] = BP_LOC_LANES;
}
uint32_t emul_bp_loc_default_size(uint32_t n) { return bp_loc_default_size(n); }
void emul_bp_loc_segments(uint32_t n, uint32_t want, uint32_t out[2]) { const BpSegments g = bp_loc_segments(n, want); out[0] = g.size; out[1] = g.count; }
uint32_t emul_bp_loc_segment_of(uint32_t n, uint32_t want, uint32_t env) { return bp_loc_segment_of(bp_loc_segments(n, want), env); }
// envelopes [lo, hi) and jobs [jlo, jhi) of every segment; job_base = null: jobs_per jobs per envelope
void emul_bp_loc_bounds(uint32_t n, uint32_t want, uint32_t jobs_per, const uint32_t* job_base, uint32_t* lo, uint32_t* hi, uint32_t* jlo, uint32_t* jhi) {
    const BpSegments g = bp_loc_segments(n, want);
    for (uint32_t s = 0; s < g.count; s++) {
        lo[s] = bp_loc_lo(g, s); hi[s] = bp_loc_hi(g, n, s);
        jlo[s] = bp_loc_job_lo(g, s, jobs_per, job_base); jhi[s] = bp_loc_job_hi(g, n, s, jobs_per, job_base);
    }
}
uint32_t emul_bp_loc_offsets(uint32_t n, uint32_t want, uint32_t jobs_per, const uint32_t* job_base, const uint8_t* suspect, uint32_t* off) {
    return bp_loc_offsets(bp_loc_segments(n, want), n, jobs_per, job_base, suspect, off);
}
// the gather and scatter kernels' index arithmetic on one word per job
void emul_bp_loc_gather(uint32_t n, uint32_t want, uint32_t jobs_per, const uint32_t* job_base, const uint8_t* suspect, const uint32_t* off, const uint32_t* batch, uint32_t* compact) {
    const BpSegments g = bp_loc_segments(n, want);
    for (uint32_t s = 0; s < g.count; s++) {
        if (!suspect[s]) continue;
        const uint32_t lo = bp_loc_job_lo(g, s, jobs_per, job_base), hi = bp_loc_job_hi(g, n, s, jobs_per, job_base);
        for (uint32_t j = lo; j < hi; j++) compact[bp_loc_compact_index(off, s, lo, j)] = batch[j];
    }
}
void emul_bp_loc_scatter(uint32_t n, uint32_t want, uint32_t jobs_per, const uint32_t* job_base, const uint8_t* suspect, const uint32_t* off, const uint32_t* compact, uint32_t* batch) {
    const BpSegments g = bp_loc_segments(n, want);
    for (uint32_t s = 0; s < g.count; s++) {
        if (!suspect[s]) continue;
        const uint32_t lo = bp_loc_job_lo(g, s, jobs_per, job_base), hi = bp_loc_job_hi(g, n, s, jobs_per, job_base);
        for (uint32_t j = lo; j < hi; j++) batch[j] = compact[bp_loc_compact_index(off, s, lo, j)];
    }
}
int emul_bp_loc_whole_batch(uint32_t suspect_jobs, uint32_t M) { return bp_loc_whole_batch(suspect_jobs, M) ? 1 : 0; }

// Niels row of a ristretto encoding; 0 if it does not decode
int emul_bp_loc_niels(const uint32_t enc[8], uint32_t row[RLC_NIELS_W]) {
    ge p; if (!ge_ristretto_decode(p, enc)) return 0;
    memset(row, 0, 4 * RLC_NIELS_W); niels_row(row, p);
    return 1;
}
// one window: niels = [17 M][32], dig = [17 M] signed digits (index p * M + job); the sum over the jobs [j_lo, j_hi), ristretto-encoded
void emul_bp_loc_window_sum(uint32_t M, const uint32_t* niels, const int16_t* dig, uint32_t j_lo, uint32_t j_hi, uint32_t enc[8], uint32_t* max_run) {
    RlcView R{}; R.N = VP_NUM * M; R.niels = const_cast<uint32_t*>(niels); R.dig = const_cast<int16_t*>(dig);
    *max_run = 0;
    ge_ristretto_encode(enc, window_sum(R, M, 0, j_lo, j_hi, max_run));
}

// The batch-mode steps over n range envelopes under the weights `weights` (16 bytes per job, as the host draws them), then the check of
// every segment of `size` envelopes (seg_ok[s] = 1: its sum is the identity) and of the whole batch (*batch_ok): generator part from the
// summed weighted coefficients through the fixed-base tables, proof-point part through the segment kernel's steps, Horner over the windows.
int emul_bp_loc_range_checks(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* mins, const uint64_t* maxs, const uint8_t* weights,
                             uint32_t size, uint8_t* seg_ok, uint8_t* batch_ok) {
    ensure_table();
    const uint32_t M = (uint32_t)(2 * n), N = VP_NUM * M;
    const MsmLayout L = make_layout_even(targets_verify(), 4);
    std::vector<uint64_t> poff(M), voff(M); std::vector<uint8_t> kind(M), lgn(M); std::vector<int32_t> bad(M);
    std::vector<uint32_t> pts((size_t)VP_NUM * GE_W * M), scal((size_t)VS_NUM * 8 * M), vs((size_t)VP_NUM * 8 * M, 0), rho((size_t)8 * M), ft((size_t)NBASE * 8 * M, 0);
    VfyView V{}; V.M = M; V.in = proofs; V.proof_off = poff.data(); V.venc_off = voff.data(); V.kind = kind.data(); V.lgn = lgn.data(); V.bad = bad.data();
    V.pts = pts.data(); V.scal = scal.data(); V.vscal = vs.data(); V.table = g_table.data(); V.rho = rho.data(); V.fterm = ft.data();
    for (uint32_t j = 0; j < M; j++) {
        sc raw = sc_zero(); memcpy(raw.v, weights + 16ull * j, 16);
        const sc m = sc_from_raw256(raw);
        for (int k = 0; k < 8; k++) rho[(size_t)k * M + j] = m.v[k];
    }
    for (uint32_t i = 0; i < n; i++) step_vparse(V, i, proofs + stride * i, stride * i, lens[i] <= stride ? lens[i] : 0u, mins[i], maxs[i]);
    for (uint32_t p = 0; p < VP_NUM; p++) for (uint32_t j = 0; j < M; j++) step_vdecode(V, p, j);
    uint32_t st[50]; Strobe s; s.base = st; s.stride = 1;
    for (uint32_t j = 0; j < M; j++) { s.pos = 0; s.pos_begin = 0; step_vtranscript(V, j, s); }
    for (uint32_t i = 0; i < BP_N; i++) for (uint32_t j = 0; j < M; j++) step_vscalars(V, i, j);
    // the point terms as k_rlc_points leaves them
    std::vector<uint32_t> niels((size_t)N * RLC_NIELS_W, 0); std::vector<int16_t> dig((size_t)RLC_NWIN * N, 0);
    RlcView R{}; R.N = N; R.niels = niels.data(); R.dig = dig.data();
    for (uint32_t p = 0; p < VP_NUM; p++) for (uint32_t j = 0; j < M; j++) {
        if (bad[j] || !vpoint_present(p, lgn[j])) continue;
        const uint32_t idx = p * M + j;
        niels_row(niels.data() + (size_t)idx * RLC_NIELS_W, ld_ge(V.pts, p, j, M));
        uint32_t pk[(RLC_NWIN + 1) / 2] = {0};
        sc_recode_signed<(int)RLC_WBITS, (int)RLC_NWIN>(pk, ld_sc(V.vscal, p, j, M));
        for (uint32_t w = 0; w < RLC_NWIN; w++) dig[(size_t)w * N + idx] = (int16_t)(pk[w >> 1] >> (16 * (w & 1u)));
    }
    auto check = [&](uint32_t j_lo, uint32_t j_hi) {
        std::vector<uint32_t> d1((size_t)NBASE * DIGW, 0), partial((size_t)L.nchunks() * GE_W);
        for (uint32_t g = 0; g < NBASE; g++) {
            sc acc = sc_zero();
            for (uint32_t j = j_lo; j < j_hi; j++) acc = sc_add(acc, ld_sc(V.fterm, g, j, M));
            st_digits(d1.data(), g, 0, 1, acc);
        }
        MsmView m; m.rows = 1; m.nslots = L.nslots(); m.nchunks = L.nchunks(); m.table = g_table.data(); m.digits = d1.data();
        m.slot_base = L.slot_base.data(); m.slot_scalar = nullptr; m.slot_nwin = L.slot_nwin.data(); m.chunk_begin = L.chunk_begin.data(); m.chunk_win0 = L.chunk_win0.data(); m.chunk_nwin = L.chunk_nwin.data();
        m.partial = partial.data(); m.acc_init = nullptr;
        ge gen = ge_identity();
        for (uint32_t c = 0; c < L.nchunks(); c++) { msm_chunk_ref(m, c, 0); gen = ge_add(gen, ld_ge(partial.data(), c, 0, 1)); }
        ge acc = window_sum(R, M, RLC_NWIN - 1, j_lo, j_hi, nullptr);
        for (int w = (int)RLC_NWIN - 2; w >= 0; w--) {
            for (uint32_t k = 0; k < RLC_WBITS; k++) acc = ge_dbl(acc);
            acc = ge_add(acc, window_sum(R, M, (uint32_t)w, j_lo, j_hi, nullptr));
        }
        uint32_t e[8]; ge_ristretto_encode(e, ge_add(acc, gen));
        return words_are_zero(e);
    };
    const BpSegments g = bp_loc_segments((uint32_t)n, size);
    for (uint32_t sg = 0; sg < g.count; sg++) seg_ok[sg] = check(bp_loc_job_lo(g, sg, 2, nullptr), bp_loc_job_hi(g, (uint32_t)n, sg, 2, nullptr)) ? 1 : 0;
    *batch_ok = check(0, M) ? 1 : 0;
    return (int)g.count;
}
}
