// TEST INFRASTRUCTURE, part of tests/devtier/devtier.hip (included at its end): the Groth16 key tables, digit recodings and their join.
//   devtier_g16_table      k_g16_build_table through g16_launch_build_table: every stored entry read back, raw and as canonical affine words
//   devtier_g16_digits     g16_recode at its nine radix forms and sc_recode_signed_rt at the ed25519 radices, host loop or one lane per case
//   devtier_g16_plan       the step list the product's planner makes for a two-slot launch (g16_plan_chunks + make_gather_steps)
//   devtier_g16_fixed_mul  builder, recoder (on the device), planner, k_msm_gather and k_sum_t in one chain: acc_init + s_0 P_0 + s_1 P_1 per row
// Every view is validated on the host before a launch; cases and bigint references: tests/devtier_g16_cases.py.
#include "../../libzkp_amd/csrc/g16_share.h"

namespace {

constexpr size_t G16T_MAX_BYTES = 256ull << 20, G16T_SLACK = 64, G16T_GUARD = 4096;      // g16_impl.inc allocates words * 4 + 64; the guard lies behind that
constexpr uint32_t G16_NFORMS = 14;

inline bool g16_form_ok(uint32_t wbits, uint32_t uneven) { return wbits >= G16_WBITS_MIN && wbits <= G16_WBITS_MAX && uneven <= 1 && (!uneven || wbits == 14); }
// canonical words of ncoord Fq coordinates -> what the key loader uploads (g16_impl.inc: build_tables): Montgomery limbs, x | y
inline void g16_base_limbs(uint32_t* dst, const uint32_t* w, uint32_t ncoord) {
    for (uint32_t c = 0; c < ncoord; c++) { const fq f = fq_from_raw(w + 8 * c); for (int k = 0; k < 10; k++) dst[10 * c + k] = f.v[k]; }
}
// a stored entry -> canonical words, by the product's own conversions
inline void g16_entry_words(uint32_t* out, const uint32_t* e, uint32_t ncoord, bool msm_form) {
    for (uint32_t c = 0; c < ncoord; c++) fq_to_raw(out + 8 * c, msm_form ? fq9_to_fq(fq9_unpack8(e + 8 * c)) : ld<fq, 10>(e + 10 * c));
}

// the table of nslots points as the loader allocates and fills it, plus `behind` bytes after the loader's own 64; all of it 0xA5 before the launch
struct G16Table { DevBuf tab, bases; size_t words = 0; uint32_t ow = 0; };
int g16_build(G16Table& T, bool g2, bool msm_form, const G16Radix& rx, const uint32_t* bases, uint32_t nslots, size_t behind) {
    const uint32_t nc = g2 ? 4 : 2;
    std::vector<uint32_t> flat((size_t)nslots * nc * 10);
    for (uint32_t s = 0; s < nslots; s++) g16_base_limbs(flat.data() + (size_t)s * nc * 10, bases + (size_t)s * nc * 8, nc);
    T.ow = g16_table_entry_words(g2, msm_form);
    T.words = (size_t)nslots * rx.slot_ent * T.ow;
    const size_t bytes = T.words * 4 + G16T_SLACK + behind;
    hipError_t e = T.bases.put(flat.data(), flat.size() * 4);
    if (e == hipSuccess) e = T.tab.alloc(bytes);
    if (e == hipSuccess) e = hipMemset(T.tab.p, 0xA5, bytes);
    if (e == hipSuccess) { g16_launch_build_table(g2, T.bases.as<uint32_t>(), nslots, T.tab.as<uint32_t>(), nullptr, msm_form, rx); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return (int)e;
}

// form 0..7: g16_recode at the even radix 2^(8 + form); 8: its uneven form; 9..13: sc_recode_signed_rt at radix 2^(11 + form - 9) with the
// digit count of edg_geom.  a: eight raw canonical scalar words; result: G16_DIGW_MAX words, written where the recoding writes them
struct G16DigCase {
    ZKP_HD static Shape shape(int op) { return op >= 0 && op < (int)G16_NFORMS ? Shape{8, 0, 0, G16_DIGW_MAX} : Shape{0, 0, 0, 0}; }
    ZKP_HD static void run(int op, const uint32_t* a, const uint32_t*, const uint32_t*, uint32_t* out) {
        const sc raw = ld<sc, 8>(a);
        if (op <= 8) { g16_recode(out, raw, op == 8 ? g16_radix(14, true) : g16_radix(8u + (uint32_t)op)); return; }
        const EdgGeom g = edg_geom(11u + (uint32_t)op - 9u);
        sc_recode_signed_rt(out, 1, raw, g.wbits, g.nwin);
    }
};
int g16_digits(int form, uint32_t n, const uint32_t* scalars, uint32_t* out, int on_device) {
    if (G16DigCase::shape(form).o == 0 || !n || n > MAX_CASES || !scalars || !out) return -1;
    if (!on_device) for (size_t i = 0; i < (size_t)n * G16_DIGW_MAX; i++) out[i] = 0xA5A5A5A5u;      // the device leg's output is filled by run_family
    return run_family<G16DigCase>(form, n, scalars, nullptr, nullptr, out, on_device);
}

// two slots (bases 0 and 1, scalar rows 0 and 1, every window) as ONE target in `chunks` chunks: the product's planner and step list
bool g16_two_slot_walk(const G16Radix& rx, uint32_t chunks, std::vector<uint32_t>& steps, std::vector<uint32_t>& step0) {
    const std::vector<SlotList> targets = {SlotList{{(uint16_t)0, (uint8_t)rx.nwin}, {(uint16_t)1, (uint8_t)rx.nwin}}};
    const G16Chunks C = g16_plan_chunks(targets, std::vector<uint16_t>{0, 1}, G16_PART_ALL, chunks);
    const GatherShape shape{rx.nent, rx.slot_ent, rx.uneven ? 1u : 0u, rx.digw};
    return make_gather_steps(C.L, C.scal.data(), shape, steps, step0) && step0.size() >= 2;
}

template <class B>
int run_fixed_mul(bool g2, const G16Radix& rx, int form, const uint32_t* bases, const uint32_t* scalars, uint32_t rows, uint32_t chunks, const uint32_t* acc_init, const uint32_t* corr, uint32_t* out) {
    std::vector<uint32_t> steps, step0;
    if (!g16_two_slot_walk(rx, chunks, steps, step0)) return -3;
    const uint32_t nchunks = (uint32_t)step0.size() - 1, nsteps = step0[nchunks];
    const uint64_t table_entries = 2ull * rx.slot_ent;
    // the recoder's device leg: case (row, slot) -> G16_DIGW_MAX words, then the digit rows [slot][digw][rows] the kernels read
    std::vector<uint32_t> pk((size_t)rows * 2 * G16_DIGW_MAX), digits((size_t)2 * rx.digw * rows);
    int rc = g16_digits(form, rows * 2, scalars, pk.data(), 1);
    if (rc) return rc;
    for (uint32_t r = 0; r < rows; r++) for (uint32_t s = 0; s < 2; s++) for (uint32_t k = 0; k < rx.digw; k++)
        digits[((size_t)s * rx.digw + k) * rows + r] = pk[((size_t)r * 2 + s) * G16_DIGW_MAX + k];
    const uint32_t digit_rows = 2 * rx.digw;
    for (uint32_t t = 0; t < nsteps; t++) {                                 // as run_msm: nothing a lane can fetch lies outside the allocation
        const uint32_t wrow = steps[2 * t + 1] >> 1, half = steps[2 * t + 1] & 1u;
        if (wrow >= digit_rows) return -4;
        for (uint32_t r = 0; r < rows; r++) {
            const int32_t d = (int32_t)(int16_t)(digits[(size_t)wrow * rows + r] >> (16 * half));
            if (d && (uint64_t)steps[2 * t] + (uint32_t)((d < 0 ? -d : d) - 1) >= table_entries) return -5;
        }
    }
    G16Table T;
    if ((rc = g16_build(T, g2, true, rx, bases, 2, 0))) return rc;
    DevBuf dsteps, dstep0, ddigits, dacc, dpartial, dbegin, dcorr, dsums;
    uint32_t a[B::ACC_W], cr[B::ACC_W];
    B::store(a, 0, 0, 1, acc_init, false, 5);
    const uint16_t begin[2] = {0, (uint16_t)nchunks};
    const size_t pwords = (size_t)nchunks * B::ACC_W * rows, swords = (size_t)B::ACC_W * rows;
    hipError_t e = dsteps.put(steps.data(), steps.size() * 4);
    if (e == hipSuccess) e = dstep0.put(step0.data(), step0.size() * 4);
    if (e == hipSuccess) e = ddigits.put(digits.data(), digits.size() * 4);
    if (e == hipSuccess) e = dacc.put(a, sizeof a);
    if (e == hipSuccess) e = dbegin.put(begin, sizeof begin);
    if (e == hipSuccess && corr) { B::store(cr, 0, 0, 1, corr, false, 3); e = dcorr.put(cr, sizeof cr); }
    if (e == hipSuccess) e = dpartial.alloc(pwords * 4);
    if (e == hipSuccess) e = hipMemset(dpartial.p, 0xA5, pwords * 4);
    if (e == hipSuccess) e = dsums.alloc(swords * 4);
    if (e == hipSuccess) e = hipMemset(dsums.p, 0xA5, swords * 4);
    if (e != hipSuccess) return (int)e;
    MsmView m{};
    m.rows = rows; m.nslots = 2; m.nchunks = nchunks; m.table = T.tab.as<uint32_t>(); m.digits = ddigits.as<uint32_t>(); m.partial = dpartial.as<uint32_t>();
    m.acc_init = dacc.as<uint32_t>(); m.nwin = rx.nwin; m.nent = rx.nent; m.digw = rx.digw; m.slot_ent = rx.slot_ent; m.uneven = rx.uneven;
    m.steps = dsteps.as<uint32_t>(); m.chunk_step0 = dstep0.as<uint32_t>();
    B::launch_msm(m, false);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return (int)e;
    ReduceView R{};
    R.rows = rows; R.ntargets = 1; R.partial = dpartial.as<uint32_t>(); R.target_chunk_begin = dbegin.as<uint16_t>(); R.corr = corr ? dcorr.as<uint32_t>() : nullptr;
    B::launch_sum(R, dsums.as<uint32_t>());
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    std::vector<uint32_t> sums(swords);
    if (e == hipSuccess) e = hipMemcpy(sums.data(), dsums.p, swords * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    for (uint32_t r = 0; r < rows; r++) B::words(out + (size_t)r * (B::AFF_W + 1), sums.data(), 0, r, rows);
    return 0;
}

}  // namespace

extern "C" {
// The table of nslots points at radix 2^wbits (uneven: the 18-window form of 2^14), packed (msm_form) or plain.  bases: [nslots][16 | 32]
// canonical affine words.  raw_out: [nslots][slot_ent][16 | 32 packed, 20 | 40 plain] stored words; aff_out: [nslots][slot_ent][16 | 32]
// canonical words; guard_out: [0] words behind the table (the loader's 64 bytes and a 4 KB guard) that are no longer 0xA5, [1] entries that
// still are, [2] packed form: 1 when BnG1::entry / BnG2::entry of every base equals the stored entry 1 of window 0.
// Below zero, nothing launched: -1 radix form, -2 nslots, -3 a null pointer, -4 a table above 256 MB.
int devtier_g16_table(int g2, int msm_form, uint32_t wbits, uint32_t uneven, const uint32_t* bases, uint32_t nslots, uint32_t* raw_out, uint32_t* aff_out, uint32_t* guard_out) {
    if (!g16_form_ok(wbits, uneven)) return -1;
    if (nslots < 1 || nslots > 4) return -2;
    if (!bases || !raw_out || !aff_out || !guard_out) return -3;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    const uint32_t nc = g2 ? 4 : 2, ow = g16_table_entry_words(g2 != 0, msm_form != 0);
    const size_t words = (size_t)nslots * rx.slot_ent * ow, behind = (G16T_SLACK + G16T_GUARD) / 4, entries = (size_t)nslots * rx.slot_ent;
    if (words * 4 > G16T_MAX_BYTES) return -4;
    G16Table T;
    const int rc = g16_build(T, g2 != 0, msm_form != 0, rx, bases, nslots, G16T_GUARD);
    if (rc) return rc;
    std::vector<uint32_t> guard(behind);
    hipError_t e = hipMemcpy(raw_out, T.tab.p, words * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(guard.data(), T.tab.as<uint32_t>() + words, behind * 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    guard_out[0] = guard_out[1] = 0; guard_out[2] = 1;
    for (uint32_t x : guard) guard_out[0] += x != 0xA5A5A5A5u;
    for (size_t i = 0; i < entries; i++) {
        const uint32_t* ent = raw_out + i * ow;
        bool stale = true; for (uint32_t k = 0; k < ow; k++) stale = stale && ent[k] == 0xA5A5A5A5u;
        guard_out[1] += stale;
        g16_entry_words(aff_out + i * nc * 8, ent, nc, msm_form != 0);
    }
    if (msm_form) for (uint32_t s = 0; s < nslots; s++) {
        uint32_t want[32];
        if (g2) BnG2::entry(want, bases + (size_t)s * 32); else BnG1::entry(want, bases + (size_t)s * 16);
        for (uint32_t k = 0; k < ow; k++) if (want[k] != raw_out[(size_t)s * rx.slot_ent * ow + k]) guard_out[2] = 0;
    }
    return 0;
}
// n raw canonical scalars [n][8] through recoding `form` (G16DigCase); out: [n][G16_DIGW_MAX], 0xA5A5A5A5 wherever the recoding wrote nothing
int devtier_g16_digits(int form, uint32_t n, const uint32_t* scalars, uint32_t* out, int on_device) { return g16_digits(form, n, scalars, out, on_device); }
// the planner's walk of the two-slot launch: steps_out [2 * 2 * nwin] as MsmView::steps, step0_out [chunks + 1]; returns the number of chunks
int devtier_g16_plan(uint32_t wbits, uint32_t uneven, uint32_t chunks, uint32_t* steps_out, uint32_t* step0_out) {
    if (!g16_form_ok(wbits, uneven)) return -1;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    if (!chunks || chunks > 2 * rx.nwin || !steps_out || !step0_out) return -2;
    std::vector<uint32_t> steps, step0;
    if (!g16_two_slot_walk(rx, chunks, steps, step0) || step0.size() > chunks + 1 || step0.back() != 2 * rx.nwin) return -3;
    for (uint32_t i = 0; i < 2 * step0.back(); i++) steps_out[i] = steps[i];
    for (size_t i = 0; i < step0.size(); i++) step0_out[i] = step0[i];
    return (int)step0.size() - 1;
}
// bases: [2][16 | 32] canonical affine words; scalars: [rows][2][8] raw canonical words; acc_init: affine words of the point every chunk
// starts from; corr: optional affine words of the point added to the sum (-(chunks - 1) acc_init); out: [rows][17 | 33]
int devtier_g16_fixed_mul(int g2, uint32_t wbits, uint32_t uneven, const uint32_t* bases, const uint32_t* scalars, uint32_t rows, uint32_t chunks, const uint32_t* acc_init, const uint32_t* corr, uint32_t* out) {
    if (!g16_form_ok(wbits, uneven)) return -1;
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    if (!rows || rows > (1u << 12) || !chunks || chunks > 2 * rx.nwin || !bases || !scalars || !acc_init || !out) return -2;
    if ((size_t)2 * rx.slot_ent * g16_table_entry_words(g2 != 0, true) * 4 > G16T_MAX_BYTES) return -4;
    const int form = uneven ? 8 : (int)wbits - 8;
    return g2 ? run_fixed_mul<BnG2>(true, rx, form, bases, scalars, rows, chunks, acc_init, corr, out) : run_fixed_mul<BnG1>(false, rx, form, bases, scalars, rows, chunks, acc_init, corr, out);
}
}
