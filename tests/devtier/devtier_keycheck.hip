// TEST INFRASTRUCTURE, not part of libzkp_hip.so: the key check's kernels (g16_keycheck.h) through the product's own
// launchers, on tables the product's own builder made.  No zkp_hip_init, no keys.
//   devtier_kc_build      g16_launch_build_table for nslots base points: the stored table, word for word
//   devtier_kc_check      g16_launch_check_table over a table the caller hands in (the built one, or one it has changed): the kernel's
//                         output words, the per-pair counts, and how many words around its outputs and in and behind the table were written
//   devtier_kc_subgroup   g16_launch_subgroup: one byte per G2 point
//   devtier_kc_twin_sums  g16_launch_twin_weighted + g16_launch_sum: sum rho_i P_i as canonical affine words
// Cases and bigint references: tests/test_gpu_devtier_keycheck.py.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstring>
#include <vector>
#include "../../libzkp_amd/csrc/g16_launch.h"

using namespace zkp;

namespace {

constexpr size_t KC_MAX_BYTES = 256ull << 20, KC_SLACK = 64, KC_GUARD_WORDS = 1024;
constexpr uint32_t KC_FILL = 0xA5A5A5A5u;

struct Buf {
    void* p = nullptr;
    ~Buf() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <class T> T* as() { return static_cast<T*>(p); }
};
inline bool form_ok(uint32_t wbits, uint32_t uneven) { return wbits >= G16_WBITS_MIN && wbits <= G16_WBITS_MAX && uneven <= 1 && (!uneven || wbits == 14); }
// canonical words of the base points -> what the key loader uploads (g16_impl.inc: build_tables): Montgomery limbs, coordinate after coordinate
std::vector<uint32_t> base_limbs(const uint32_t* bases, uint32_t nslots, uint32_t nc) {
    std::vector<uint32_t> flat((size_t)nslots * nc * 10);
    for (size_t c = 0; c < (size_t)nslots * nc; c++) { const fq f = fq_from_raw(bases + 8 * c); for (int k = 0; k < 10; k++) flat[10 * c + k] = f.v[k]; }
    return flat;
}
size_t count_changed(const std::vector<uint32_t>& v, size_t from, size_t to) { size_t n = 0; for (size_t i = from; i < to; i++) n += v[i] != KC_FILL; return n; }

}  // namespace

extern "C" {

uint32_t devtier_kc_entry_words(int g2, int msm_form) { return g16_table_entry_words(g2 != 0, msm_form != 0); }
// geometry of a radix form as the product has it: out = {nwin, nent, slot_ent}
int devtier_kc_geom(uint32_t wbits, uint32_t uneven, uint32_t* out) {
    if (!form_ok(wbits, uneven) || !out) return -1;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    out[0] = rx.nwin; out[1] = rx.nent; out[2] = rx.slot_ent;
    return 0;
}

// bases: [nslots][16 | 32] canonical affine words; raw_out: [nslots * slot_ent * entry words]
int devtier_kc_build(int g2, int msm_form, uint32_t wbits, uint32_t uneven, const uint32_t* bases, uint32_t nslots, uint32_t* raw_out) {
    if (!form_ok(wbits, uneven) || nslots < 1 || nslots > 4 || !bases || !raw_out) return -1;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    const size_t words = (size_t)nslots * rx.slot_ent * g16_table_entry_words(g2 != 0, msm_form != 0);
    if (words * 4 > KC_MAX_BYTES) return -4;
    const std::vector<uint32_t> flat = base_limbs(bases, nslots, g2 ? 4 : 2);
    Buf d_bases, d_tab;
    hipError_t e = d_bases.alloc(flat.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_bases.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_tab.alloc(words * 4 + KC_SLACK);
    if (e == hipSuccess) { g16_launch_build_table(g2 != 0, d_bases.as<uint32_t>(), nslots, d_tab.as<uint32_t>(), nullptr, msm_form != 0, rx); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(raw_out, d_tab.p, words * 4, hipMemcpyDeviceToHost);
    return (int)e;
}

// raw: the table to check.  pair_bad_out: [nslots * nwin]; out4: the kernel's KC_OUT_WORDS; written3: words that differ from what they held
// before the launch {in the table and the guard behind it, in the guards around pair_bad, in the guards around the output words}
int devtier_kc_check(int g2, int msm_form, uint32_t wbits, uint32_t uneven, const uint32_t* bases, uint32_t nslots, const uint32_t* raw, uint32_t* pair_bad_out,
                     uint32_t* out4, uint32_t* written3) {
    if (!form_ok(wbits, uneven) || nslots < 1 || nslots > 4 || !bases || !raw || !pair_bad_out || !out4 || !written3) return -1;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    const size_t words = (size_t)nslots * rx.slot_ent * g16_table_entry_words(g2 != 0, msm_form != 0), npairs = (size_t)nslots * rx.nwin;
    if (words * 4 > KC_MAX_BYTES) return -4;
    const std::vector<uint32_t> flat = base_limbs(bases, nslots, g2 ? 4 : 2);
    const size_t G = KC_GUARD_WORDS;
    // table | guard ;  guard | pair_bad | guard ;  guard | out | guard
    std::vector<uint32_t> h_tab(words + G, KC_FILL), h_pairs(npairs + 2 * G, KC_FILL), h_out(KC_OUT_WORDS + 2 * G, KC_FILL);
    memcpy(h_tab.data(), raw, words * 4);
    Buf d_bases, d_tab, d_pairs, d_out;
    hipError_t e = d_bases.alloc(flat.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_bases.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_tab.alloc(h_tab.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_tab.p, h_tab.data(), h_tab.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_pairs.alloc(h_pairs.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_pairs.p, h_pairs.data(), h_pairs.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_out.alloc(h_out.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_out.p, h_out.data(), h_out.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = g16_launch_check_table(g2 != 0, d_bases.as<uint32_t>(), nslots, d_tab.as<uint32_t>(), msm_form != 0, rx, d_pairs.as<uint32_t>() + G, d_out.as<uint32_t>() + G, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<uint32_t> a_tab(h_tab.size());
    if (e == hipSuccess) e = hipMemcpy(a_tab.data(), d_tab.p, a_tab.size() * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_pairs.data(), d_pairs.p, h_pairs.size() * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_out.data(), d_out.p, h_out.size() * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    written3[0] = 0; for (size_t i = 0; i < a_tab.size(); i++) written3[0] += a_tab[i] != h_tab[i];
    written3[1] = (uint32_t)(count_changed(h_pairs, 0, G) + count_changed(h_pairs, G + npairs, h_pairs.size()));
    written3[2] = (uint32_t)(count_changed(h_out, 0, G) + count_changed(h_out, G + KC_OUT_WORDS, h_out.size()));
    memcpy(pair_bad_out, h_pairs.data() + G, npairs * 4);
    memcpy(out4, h_out.data() + G, KC_OUT_WORDS * 4);
    return 0;
}

// pts: [n][32] canonical affine G2 words; ok: [n] bytes
int devtier_kc_subgroup(const uint32_t* pts, uint32_t n, uint8_t* ok) {
    if (!pts || !ok || !n || n > 4096) return -1;
    const std::vector<uint32_t> flat = base_limbs(pts, n, 4);
    Buf d_pts, d_ok;
    hipError_t e = d_pts.alloc(flat.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_pts.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_ok.alloc(n);
    if (e == hipSuccess) e = hipMemset(d_ok.p, 0xA5, n);
    if (e == hipSuccess) { g16_launch_subgroup(d_pts.as<uint32_t>(), n, d_ok.as<uint8_t>(), nullptr); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(ok, d_ok.p, n, hipMemcpyDeviceToHost);
    return (int)e;
}

// pts: [n][16 | 32] canonical affine words; rho: [n][4] words; out: [17 | 33] = canonical affine words of sum rho_i P_i and a flag (1: the
// sum is the point at infinity)
int devtier_kc_twin_sum(int g2, const uint32_t* pts, const uint32_t* rho, uint32_t n, uint32_t* out) {
    if (!pts || !rho || !out || !n || n > 4096) return -1;
    const uint32_t nc = g2 ? 4 : 2, JW = g2 ? G2_JAC_W : G1_JAC_W;
    const std::vector<uint32_t> flat = base_limbs(pts, n, nc);
    const uint16_t tcb[2] = {0, (uint16_t)n};
    Buf d_pts, d_rho, d_part, d_sum, d_tcb;
    hipError_t e = d_pts.alloc(flat.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(d_pts.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_rho.alloc(16 * (size_t)n);
    if (e == hipSuccess) e = hipMemcpy(d_rho.p, rho, 16 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = d_part.alloc((size_t)JW * 4 * n);
    if (e == hipSuccess) e = d_sum.alloc((size_t)JW * 4);
    if (e == hipSuccess) e = d_tcb.alloc(sizeof tcb);
    if (e == hipSuccess) e = hipMemcpy(d_tcb.p, tcb, sizeof tcb, hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
    g16_launch_twin_weighted(g2 != 0, d_pts.as<uint32_t>(), d_rho.as<uint32_t>(), n, d_part.as<uint32_t>(), nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    ReduceView R{}; R.rows = 1; R.ntargets = 1; R.partial = d_part.as<uint32_t>(); R.target_chunk_begin = d_tcb.as<uint16_t>();
    g16_launch_sum(g2 != 0, R, d_sum.as<uint32_t>(), nullptr);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    uint32_t sum[G2_JAC_W];
    if ((e = hipDeviceSynchronize()) != hipSuccess || (e = hipMemcpy(sum, d_sum.p, (size_t)JW * 4, hipMemcpyDeviceToHost)) != hipSuccess) return (int)e;
    memset(out, 0, (nc * 8 + 1) * 4);
    if (!g2) { g1_aff a; if (jac_to_aff(a, ld_g1_jac(sum, 0, 0, 1))) { fq_to_raw(out, a.x); fq_to_raw(out + 8, a.y); } else out[16] = 1; }
    else { g2_aff a; if (jac_to_aff(a, ld_g2_jac(sum, 0, 0, 1))) { fq_to_raw(out, a.x.c0); fq_to_raw(out + 8, a.x.c1); fq_to_raw(out + 16, a.y.c0); fq_to_raw(out + 24, a.y.c1); } else out[32] = 1; }
    return 0;
}

}  // extern "C"
