// TEST INFRASTRUCTURE: the shared key points of the Groth16 sums A and B1 (libzkp_amd/csrc/g16_share.h) on the CPU -- which variables
// of a key share a point, the three slot lists A' | S | B1' and the two overlapping chunk ranges the sums read, and one A / B1 launch
// walked through its step list (bp_layout.h) against double-and-add.  A program of its own (it is also run under the host sanitizers):
//   emul_g16_shared_points <equality proving key> <membership proving key>
// prints one line "ok <check>" or "FAIL <check> ..." per check and returns the number of failures.  Compiled and run by
// tests/test_emul_g16_shared_points.py; not part of the product.
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/g16_share.h"
#include <array>
#include <cstdio>
#include <map>
#include <string>
#include <tuple>
#include <vector>
using namespace zkp;

static int g_fail = 0;
static void report(const std::string& name, bool ok, const std::string& detail = "") {
    printf("%s %s%s%s\n", ok ? "ok" : "FAIL", name.c_str(), detail.empty() ? "" : " ", detail.c_str());
    if (!ok) g_fail++;
}

// ---- a proving key's G1 part, and the G1 slots of the A / B1 launch.  build_slots is a COPY of what load_key_body (g16_impl.inc) does with
// g16_ab_slots' lists -- A' + delta + alpha | S | B1' + delta + beta -- and must be kept in step with it; the loader itself and the
// offset corrections of get_chunking are covered by the byte-identity tests on the GPU (tests/test_gpu_g16_shared_points.py)
struct Key { G1Pt alpha, beta, delta; std::vector<G1Pt> aq, b1q; std::vector<uint8_t> cls; };
static bool read_key(const char* path, int kind, Key& K) {
    FILE* f = fopen(path, "rb"); if (!f) return false;
    std::vector<uint8_t> blob; uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    KeyReader R{blob.data(), blob.size()}; G16VkBlob B;
    if (g16_read_key_prefix(R, B) != G16_BLOB_PROVING_KEY) return false;
    K.alpha = B.alpha_g1;
    if (parse_g1(R, K.beta.inf, K.beta.p) || parse_g1(R, K.delta.inf, K.delta.p) || parse_vec_g1(R, K.aq) || parse_vec_g1(R, K.b1q)) return false;
    const HostR1CS cs = kind == 0 ? build_equality_r1cs() : build_membership_r1cs();
    K.cls = cs.inst_nwin; K.cls.insert(K.cls.end(), cs.wit_nwin.begin(), cs.wit_nwin.end());
    return K.cls.size() == K.aq.size() && K.aq.size() == K.b1q.size();
}
// scalar rows: z_k = k, r = nv, s = nv + 1, one = nv + 2
struct Slots { std::vector<SlotList> lists; std::vector<g1_aff> bases; std::vector<uint16_t> scal; size_t shared = 0; };   // lists: A' | S | B1', (slot, windows)
static Slots build_slots(const Key& K, const G16Radix& rx, bool share) {
    Slots S; S.lists.resize(3);
    const uint32_t nv = (uint32_t)K.aq.size();
    const G16AbSlots ab = g16_ab_slots(K.aq, K.b1q, K.cls, share);
    S.shared = ab.s.size();
    auto add = [&](int t, const G1Pt& pt, uint32_t row, uint8_t nwin) {
        if (pt.inf) return;
        S.lists[t].push_back({(uint16_t)S.bases.size(), nwin}); S.bases.push_back(pt.p); S.scal.push_back((uint16_t)row);
    };
    for (auto& sl : ab.a) add(0, K.aq[sl.first], sl.first, g16_class_nwin(sl.second, rx));
    add(0, K.delta, nv, (uint8_t)rx.nwin); add(0, K.alpha, nv + 2, 1);
    for (auto& sl : ab.s) add(1, K.aq[sl.first], sl.first, g16_class_nwin(sl.second, rx));
    for (auto& sl : ab.b) add(2, K.b1q[sl.first], sl.first, g16_class_nwin(sl.second, rx));
    add(2, K.delta, nv + 1, (uint8_t)rx.nwin); add(2, K.beta, nv + 2, 1);
    return S;
}
// what the loader did before points were shared, written out on its own: every finite a_query point, delta, alpha | every finite
// b_g1_query point, delta, beta
static Slots parent_slots(const Key& K, const G16Radix& rx) {
    Slots S; S.lists.resize(2);
    const uint32_t nv = (uint32_t)K.aq.size();
    auto add = [&](int t, const G1Pt& pt, uint32_t row, uint8_t nwin) {
        if (pt.inf) return;
        S.lists[t].push_back({(uint16_t)S.bases.size(), nwin}); S.bases.push_back(pt.p); S.scal.push_back((uint16_t)row);
    };
    for (uint32_t k = 0; k < nv; k++) add(0, K.aq[k], k, g16_class_nwin(K.cls[k], rx));
    add(0, K.delta, nv, (uint8_t)rx.nwin); add(0, K.alpha, nv + 2, 1);
    for (uint32_t k = 0; k < nv; k++) add(1, K.b1q[k], k, g16_class_nwin(K.cls[k], rx));
    add(1, K.delta, nv + 1, (uint8_t)rx.nwin); add(1, K.beta, nv + 2, 1);
    return S;
}
static uint64_t windows_of(const std::vector<SlotList>& lists) { uint64_t w = 0; for (auto& t : lists) for (auto& sl : t) w += sl.second; return w; }
static bool same_layout(const MsmLayout& a, const MsmLayout& b) {
    return a.slot_base == b.slot_base && a.slot_nwin == b.slot_nwin && a.chunk_begin == b.chunk_begin && a.chunk_win0 == b.chunk_win0 && a.chunk_nwin == b.chunk_nwin &&
           a.target_chunk_begin == b.target_chunk_begin;
}

// ---- the terms of a sum: (point, scalar row, window) -> how often
using Term = std::tuple<std::array<uint32_t, 16>, uint32_t, uint32_t>;
static std::array<uint32_t, 16> point_words(const g1_aff& p) { std::array<uint32_t, 16> w; fq_to_raw(w.data(), p.x); fq_to_raw(w.data() + 8, p.y); return w; }
static uint32_t window_of_offset(const G16Radix& rx, uint32_t off) { for (uint32_t w = 0; w < rx.nwin; w++) if (g16_win_off(rx, w) == off) return w; return ~0u; }
struct Walk { MsmLayout L; std::vector<uint32_t> steps, step0; std::vector<uint16_t> scal; };
static bool make_walk(Walk& W, const Slots& S, const std::vector<SlotList>& targets, uint32_t chunks, const G16Radix& rx) {
    W.L = make_layout_even(targets, chunks);
    W.scal.clear(); for (uint16_t b : W.L.slot_base) W.scal.push_back(S.scal[b]);
    const GatherShape shape{rx.nent, rx.slot_ent, rx.uneven ? 1u : 0u, rx.digw};
    return make_gather_steps(W.L, W.scal.data(), shape, W.steps, W.step0);
}
// the terms the chunks [c0, c1) walk, read back from the step list alone
static bool terms_of_chunks(std::map<Term, int>& out, const Walk& W, const Slots& S, const G16Radix& rx, uint32_t c0, uint32_t c1) {
    for (uint32_t i = W.step0[c0]; i < W.step0[c1]; i++) {
        const uint32_t first = W.steps[2 * i], ds = W.steps[2 * i + 1];
        const uint32_t base = first / rx.slot_ent, w = window_of_offset(rx, first % rx.slot_ent);
        if (base >= S.bases.size() || w == ~0u || (ds & 1u) != (w & 1u) || (ds >> 1) % rx.digw != w / 2) return false;
        out[Term{point_words(S.bases[base]), (ds >> 1) / rx.digw, w}]++;
    }
    return true;
}
static std::map<Term, int> terms_of_list(const Slots& S, const SlotList& t) {
    std::map<Term, int> out;
    for (auto& sl : t) for (uint32_t w = 0; w < sl.second; w++) out[Term{point_words(S.bases[sl.first]), S.scal[sl.first], w}]++;
    return out;
}
static bool each_once(const std::map<Term, int>& m) { for (auto& kv : m) if (kv.second != 1) return false; return true; }

static void check_committed_key(const char* path, int kind) {
    const std::string tag = kind == 0 ? "equality" : "membership";
    Key K;
    if (!read_key(path, kind, K)) { report("read_key_" + tag, false, path); return; }
    for (uint32_t wbits : {13u, 8u}) {
        const G16Radix rx = g16_radix(wbits);
        const Slots S = build_slots(K, rx, true), off = build_slots(K, rx, false), P = parent_slots(K, rx);
        const std::string r = tag + "_w" + std::to_string(wbits);
        if (wbits == 13) report("shared_count_" + tag, S.shared == 110, std::to_string(S.shared));
        report("windows_fall_" + r, windows_of(P.lists) - windows_of(S.lists) == 110ull * rx.nwin && S.bases.size() + 110 == P.bases.size(),
               std::to_string(windows_of(P.lists)) + " -> " + std::to_string(windows_of(S.lists)));
        // the switch off: the parent's lists, bases and scalar rows
        bool same_off = off.lists[1].empty() && off.lists[0] == P.lists[0] && off.lists[2] == P.lists[1] && off.scal == P.scal && off.bases.size() == P.bases.size();
        for (size_t i = 0; same_off && i < P.bases.size(); i++) same_off = point_words(off.bases[i]) == point_words(P.bases[i]);
        report("switch_off_is_parent_" + r, same_off);
        // A' u S == A and S u B1' == B1, every (point, scalar row, window) once, through the step lists of several chunkings
        bool ok = true;
        const std::vector<SlotList> targets = g16_ab_targets(S.lists[0], S.lists[1], S.lists[2]);
        const std::map<Term, int> wantA = terms_of_list(P, P.lists[0]), wantB = terms_of_list(P, P.lists[1]);
        ok = ok && targets.size() == 3 && each_once(wantA) && each_once(wantB);
        for (uint32_t chunks : {3u, 7u, 64u, 229u}) {
            Walk W;
            if (!make_walk(W, S, targets, chunks, rx)) { ok = false; break; }
            const G16AbRanges ab = g16_ab_ranges(W.L);
            ok = ok && W.L.ntargets() == 3 && ab.begin[0] == 0 && ab.begin[1] > ab.begin[0] && ab.end[0] > ab.begin[1] && ab.end[1] > ab.end[0] && ab.end[1] == W.L.nchunks();
            std::map<Term, int> gotA, gotB;
            ok = ok && terms_of_chunks(gotA, W, S, rx, ab.begin[0], ab.end[0]) && terms_of_chunks(gotB, W, S, rx, ab.begin[1], ab.end[1]);
            ok = ok && gotA == wantA && gotB == wantB;
        }
        report("each_term_once_" + r, ok);
    }
}

// ---- synthetic keys: points k * G from small multipliers (0 = the point at infinity)
static g1_jac mul_ref(const g1_jac& p, const uint32_t k[8]) {          // plain double-and-add over the 256 bits of k
    g1_jac acc = jac_infinity<fq>();
    for (int bit = 255; bit >= 0; bit--) { acc = jac_dbl(acc); if ((k[bit >> 5] >> (bit & 31)) & 1u) acc = jac_add(acc, p); }
    return acc;
}
static G1Pt small_point(uint32_t m) {
    G1Pt r{}; r.inf = m == 0;
    if (m) { const uint32_t k[8] = {m, 0, 0, 0, 0, 0, 0, 0}; jac_to_aff(r.p, mul_ref(jac_from_aff(g1_aff{fq_from_u64(1), fq_from_u64(2)}), k)); }
    return r;
}
static Key synthetic_key(const std::vector<uint32_t>& a, const std::vector<uint32_t>& b, const std::vector<uint8_t>& cls) {
    Key K; K.alpha = small_point(1001); K.beta = small_point(1002); K.delta = small_point(1003); K.cls = cls;
    for (uint32_t m : a) K.aq.push_back(small_point(m));
    for (uint32_t m : b) K.b1q.push_back(small_point(m));
    return K;
}
static bool same_jac(const g1_jac& p, const g1_jac& q) {
    g1_aff a, b; const bool fa = jac_to_aff(a, p), fb = jac_to_aff(b, q);
    return fa == fb && (!fa || (fq_eq(a.x, b.x) && fq_eq(a.y, b.y)));
}

static void check_synthetic() {
    const uint8_t F = G16_NW_FULL, U = G16_NW_U64;
    {   // no coincidence: the parent's slot lists, and layouts identical to the parent's for every chunk count
        const Key K = synthetic_key({3, 5, 0, 7, 9, 11, 13, 15}, {4, 0, 6, 8, 10, 0, 12, 14}, {1, F, F, U, F, 1, F, F});
        bool ok = true;
        for (uint32_t wbits : {8u, 13u}) {
            const G16Radix rx = g16_radix(wbits);
            const Slots S = build_slots(K, rx, true), P = parent_slots(K, rx);
            ok = ok && S.shared == 0 && S.lists[1].empty() && S.lists[0] == P.lists[0] && S.lists[2] == P.lists[1] && S.scal == P.scal;
            const std::vector<SlotList> targets = g16_ab_targets(S.lists[0], S.lists[1], S.lists[2]);
            ok = ok && targets == P.lists;
            for (uint32_t c = 2; c <= 40; c++) {
                const MsmLayout a = make_layout_even(targets, c), b = make_layout_even(P.lists, c);
                const G16AbRanges r = g16_ab_ranges(a);
                ok = ok && same_layout(a, b) && a.ntargets() == 2 && r.begin[0] == b.target_chunk_begin[0] && r.end[0] == b.target_chunk_begin[1] &&
                     r.begin[1] == b.target_chunk_begin[1] && r.end[1] == b.target_chunk_begin[2];
            }
        }
        report("no_coincidence_is_parent_layout", ok);
    }
    {   // equal but at infinity: no slot anywhere
        const Key K = synthetic_key({3, 0, 5, 7}, {4, 0, 6, 8}, {F, F, F, F});
        const G16AbSlots ab = g16_ab_slots(K.aq, K.b1q, K.cls, true);
        report("infinity_pair_ignored", ab.s.empty() && ab.a == SlotList{{0, F}, {2, F}, {3, F}} && ab.b == SlotList{{0, F}, {2, F}, {3, F}});
    }
    {   // equal at different indices: two terms with two scalars, two slots
        const Key K = synthetic_key({3, 5, 7, 9}, {4, 6, 5, 8}, {F, F, F, F});
        const G16AbSlots ab = g16_ab_slots(K.aq, K.b1q, K.cls, true);
        report("different_index_ignored", ab.s.empty() && ab.a.size() == 4 && ab.b.size() == 4);
    }
    {   // the negation of a point is another point
        Key K = synthetic_key({3, 5}, {3, 5}, {F, F});
        K.b1q[1].p = aff_neg(K.b1q[1].p);
        const G16AbSlots ab = g16_ab_slots(K.aq, K.b1q, K.cls, true);
        report("negation_not_shared", ab.s == SlotList{{0, F}} && ab.a == SlotList{{1, F}} && ab.b == SlotList{{1, F}});
    }
    // One A / B1 launch on the host: 10 variables, 3 shared (one of each window class), an infinite pair, a finite point against an infinite
    // one both ways, a pair equal at different indices.  Chunk accumulators start from an offset point O and the sums take -(chunks) O,
    // as on the device; entries are rebuilt by double-and-add from the (point, window, |digit|) a step's entry index stands for.
    const Key K = synthetic_key({21, 22, 23, 0, 24, 0, 25, 26, 27, 28}, {21, 32, 23, 0, 0, 35, 22, 26, 37, 38}, {F, F, U, F, F, F, F, 1, U, F});
    const uint32_t nv = (uint32_t)K.aq.size(), nrows = nv + 3;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    std::vector<sc> scalars(nrows);
    for (uint32_t k = 0; k < nrows; k++) {
        sc s{}; const uint8_t c = k < nv ? K.cls[k] : F;
        if (k == nv + 2) s.v[0] = 1;                                      // the row "one"
        else if (c == 1) s.v[0] = (uint32_t)(rnd() & 1u);
        else if (c == U) { const uint64_t v = k == 2 ? ~0ull : rnd(); s.v[0] = (uint32_t)v; s.v[1] = (uint32_t)(v >> 32); }
        else { for (int i = 0; i < 8; i += 2) { const uint64_t v = rnd(); s.v[i] = (uint32_t)v; s.v[i + 1] = (uint32_t)(v >> 32); } s.v[7] &= 0x1fffffffu; }   // < 2^253 < r
        scalars[k] = s;
    }
    auto direct = [&](const std::vector<G1Pt>& q, const G1Pt& last, uint32_t row_delta) {
        g1_jac acc = jac_from_aff(last.p);
        for (uint32_t k = 0; k < nv; k++) if (!q[k].inf) acc = jac_add(acc, mul_ref(jac_from_aff(q[k].p), scalars[k].v));
        return jac_add(acc, mul_ref(jac_from_aff(K.delta.p), scalars[row_delta].v));
    };
    const g1_jac wantA = direct(K.aq, K.alpha, nv), wantB = direct(K.b1q, K.beta, nv + 1);
    const g1_jac O = jac_from_aff(small_point(77777).p);
    for (int form = 0; form < 3; form++) {
        const G16Radix rx = form == 0 ? g16_radix(8) : form == 1 ? g16_radix(13) : g16_radix(14, true);
        const Slots S = build_slots(K, rx, true);
        std::vector<uint32_t> digits((size_t)nrows * rx.digw);
        for (uint32_t k = 0; k < nrows; k++) { uint32_t pk[G16_DIGW_MAX]; g16_recode(pk, scalars[k], rx); for (uint32_t j = 0; j < rx.digw; j++) digits[(size_t)k * rx.digw + j] = pk[j]; }
        bool ok = S.shared == 3 && S.lists[1].size() == 3;
        const std::vector<SlotList> targets = g16_ab_targets(S.lists[0], S.lists[1], S.lists[2]);
        for (uint32_t chunks : {3u, 5u, 16u}) {
            Walk W;
            if (!make_walk(W, S, targets, chunks, rx)) { ok = false; break; }
            std::vector<g1_jac> partial(W.L.nchunks());
            for (uint32_t c = 0; c < W.L.nchunks(); c++) {
                g1_jac acc = O;
                for (uint32_t i = W.step0[c]; i < W.step0[c + 1]; i++) {
                    const uint32_t first = W.steps[2 * i], ds = W.steps[2 * i + 1];
                    const int32_t d = (int32_t)(int16_t)(digits[ds >> 1] >> (16 * (ds & 1u)));
                    if (d == 0) continue;
                    const uint32_t base = first / rx.slot_ent, w = window_of_offset(rx, first % rx.slot_ent), mag = (uint32_t)(d < 0 ? -d : d);
                    if (base >= S.bases.size() || w == ~0u || mag > g16_win_ent(rx, w)) { ok = false; continue; }
                    g1_jac p = jac_from_aff(S.bases[base]);
                    for (uint32_t b = 0; b < g16_win_bit(rx, w); b++) p = jac_dbl(p);
                    const uint32_t km[8] = {mag, 0, 0, 0, 0, 0, 0, 0};
                    p = mul_ref(p, km);
                    acc = jac_add(acc, d < 0 ? jac_neg(p) : p);
                }
                partial[c] = acc;
            }
            const G16AbRanges ab = g16_ab_ranges(W.L);
            for (int t = 0; t < 2; t++) {
                g1_jac sum = jac_infinity<fq>(), corr = jac_infinity<fq>();
                for (uint32_t c = ab.begin[t]; c < ab.end[t]; c++) { sum = jac_add(sum, partial[c]); corr = jac_add(corr, O); }
                sum = jac_add(sum, jac_neg(corr));
                ok = ok && same_jac(sum, t == 0 ? wantA : wantB);
            }
        }
        report(std::string("msm_walk_") + (form == 0 ? "w8" : form == 1 ? "w13" : "w14_uneven"), ok);
    }
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s <equality proving key> <membership proving key>\n", argv[0]); return 100; }
    check_committed_key(argv[1], 0);
    check_committed_key(argv[2], 1);
    check_synthetic();
    return g_fail;
}
