// TEST INFRASTRUCTURE: the lane-per-proof QAP passes (g16_steps.h: g16_qap_pass_single / _pair / _triple, in the launch order of
// g16_qap_lane_schedule for either pass shape) run on the host for every task of every pass, against g16_qap_proof: all m - 1 digit rows of h, word for word.
// A program of its own so that it can be built with -fsanitize=address,undefined: every buffer has exactly the size the prover gives it.
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include <cstdio>
#include <vector>
using namespace zkp;

struct NoSync { void operator()() const {} };

static int run_kind(int kind, uint32_t shape) {
    const HostR1CS cs = kind == 0 ? build_equality_r1cs() : build_membership_r1cs();
    const HostCircuitTables T = build_circuit_tables(cs);
    ensure_mimc_constants();
    std::vector<uint32_t> mc; for (auto& c : g_mimc_host) put_fr(mc, c);
    const uint32_t rows = 3, nsc = g16_nscalars(T.nv, T.m);
    const G16Radix rx = g16_radix(G16_WBITS_DEFAULT);
    // 64-bit extremes; membership: sets of 1, 64 and 64 elements (the value first, last, in the middle)
    const uint64_t values[rows] = {0ull, 0xffffffffffffffffull, 0x0123456789abcdefull};
    const uint32_t set_len[rows] = {1, G16_MAX_SET, G16_MAX_SET};
    std::vector<uint64_t> sets((size_t)rows * G16_MAX_SET, 0);
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t i = 0; i < set_len[r]; i++) sets[(size_t)r * G16_MAX_SET + i] = 0x8000000000000000ull + 977ull * i + r;
    sets[0] = values[0]; sets[(size_t)1 * G16_MAX_SET + 63] = values[1]; sets[(size_t)2 * G16_MAX_SET + 31] = values[2];
    std::vector<uint32_t> seeds((size_t)rows * 8);
    for (size_t i = 0; i < seeds.size(); i++) seeds[i] = 0x9e3779b9u * (uint32_t)(i + 1 + 100 * kind);
    const uint64_t stride = 10 + 4 + 8 * G16_MAX_SET + 256 + 32;
    std::vector<uint8_t> out((size_t)rows * stride);
    std::vector<uint32_t> z((size_t)T.nv * 8 * rows), sdig((size_t)nsc * rx.digw * rows), rs((size_t)16 * rows);
    G16View V{}; V.rx = rx; V.rows = rows; V.kind = (uint32_t)kind; V.n_inst = T.n_inst; V.n_wit = T.n_wit; V.nv = T.nv; V.m = T.m;
    V.value = values; V.set_vals = sets.data(); V.set_len = set_len; V.seeds = seeds.data(); V.mimc_c = mc.data();
    V.z = z.data(); V.sdig = sdig.data(); V.rs = rs.data(); V.out = out.data(); V.stride = stride;
    for (uint32_t r = 0; r < rows; r++) step_g16_witness(V, r);
    G16Circuit C{}; C.n_rows = T.n_rows; C.m = T.m; C.logm = T.logm;
    C.a_ptr = T.ptr[0].data(); C.a_col = T.col[0].data(); C.a_coef = T.coef[0].data();
    C.b_ptr = T.ptr[1].data(); C.b_col = T.col[1].data(); C.b_coef = T.coef[1].data();
    C.c_ptr = T.ptr[2].data(); C.c_col = T.col[2].data(); C.c_coef = T.coef[2].data();
    C.tw = T.tw.data(); C.tw_inv = T.tw_inv.data(); C.coset = T.coset.data(); C.coset_inv = T.coset_inv.data(); C.zinv = T.zinv.data();

    // the reference: one proof at a time through the image g16_qap_proof keeps (its scratch: 2 x 9 x m words per proof)
    std::vector<uint32_t> want(sdig.size(), 0xaaaaaaaau), lds((size_t)9 * T.m), scratch((size_t)2 * 9 * T.m);
    G16View Vr = V; Vr.sdig = want.data();
    G16Lds L; L.base = lds.data(); L.m = T.m;
    for (uint32_t r = 0; r < rows; r++) g16_qap_proof(Vr, C, L, scratch.data(), r, 0, 1, NoSync());

    // the passes: every task of every launch, launches in order, the tasks of a launch from the last to the first (they are independent)
    std::vector<uint32_t> got(sdig.size(), 0x55555555u), qe((size_t)3 * 9 * T.m * rows, 0xdeadbeefu);
    G16View Vl = V; Vl.sdig = got.data(); Vl.qap_evals = qe.data();
    uint32_t launches = 0, passes = 0; bool known = true;
    g16_qap_lane_schedule(C.m, C.logm, shape, [&](bool dif, int nst, int head, int tail, uint32_t h, uint32_t ntasks, uint32_t npoly, uint32_t poly0) {
        launches++; passes += npoly;
        for (uint32_t p = 0; p < npoly; p++)
            for (uint32_t q = ntasks; q-- > 0;)
                for (uint32_t r = 0; r < rows; r++) known = g16_qap_lane_task(Vl, C, dif, nst, head, tail, h, poly0 + p, q, r) && known;
    });
    if (!known) { printf("kind %d: the schedule names a pass that has no step function\n", kind); return 1; }
    const size_t h0 = (size_t)g16_sc_h(V) * rx.digw * rows, h1 = (size_t)(g16_sc_h(V) + T.m - 1) * rx.digw * rows;
    size_t bad = 0, untouched = 0;
    for (size_t i = 0; i < got.size(); i++) {
        if (i >= h0 && i < h1) { if (got[i] != want[i]) { if (!bad) printf("kind %d: digit word %zu differs: %08x, want %08x\n", kind, i, got[i], want[i]); bad++; } }
        else if (got[i] != 0x55555555u || want[i] != 0xaaaaaaaau) untouched++;
    }
    if (untouched) { printf("kind %d: %zu digit words outside h were written\n", kind, untouched); return 1; }
    if (bad) { printf("kind %d: %zu of %zu digit words of h differ\n", kind, bad, h1 - h0); return 1; }
    printf("kind %d, passes of up to %u stages: m = %u, %u launches, %u polynomial passes, %u rows x %u digit rows of h identical\n", kind, shape, T.m, launches, passes, rows, T.m - 1);
    return 0;
}

int main() {
    for (uint32_t shape = 2; shape <= 3; shape++)
        for (int kind = 0; kind < 2; kind++) if (run_kind(kind, shape)) return 1;
    printf("ok\n");
    return 0;
}
