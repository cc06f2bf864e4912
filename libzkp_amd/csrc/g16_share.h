// Groth16 key loader (host only): key points that the sums A and B1 share.  A = alpha + sum z_k a_query[k] + r delta and
// B1 = beta + sum z_k b_g1_query[k] + s delta walk the same scalar rows z_k, and where a_query[k] and b_g1_query[k] are one point the
// two sums hold the same term: such a variable gets ONE slot (one table, one gather, one mixed addition per window), and the chunks that
// hold those slots are added into both sums.  The A / B1 launch is laid out A' | S | B1' (S: the shared slots); the sums read the two
// overlapping chunk ranges A' u S and S u B1' (ReduceView::target_chunk_end, bp_steps.h).  The rule reads the key's points only -- nothing
// about the circuit.  Below it: the plan of all of a key's slots, and of a launch's chunks.  Compiled for the host by tests/emul/emul_g16_shared_points.cpp too.
#pragma once
#include <cstdint>
#include <vector>
#include "bp_layout.h"
#include "g16_circuit.h"
#include "g16_keyblob.h"

namespace zkp {

// Variable k is shared when a_query[k] and b_g1_query[k] are both finite and equal as affine points.  Both would read scalar row k with
// the window class of variable k, so the same index is the whole of "same scalar, same windows": a_query[k] == b_g1_query[j] with j != k
// is two different terms and stays two slots.
inline bool g16_shared_point(const G1Pt& a, const G1Pt& b) { return !a.inf && !b.inf && fq_eq(a.p.x, b.p.x) && fq_eq(a.p.y, b.p.y); }

// The variables of the three slot lists as (variable index, window class of that variable), each in index order; points at infinity get
// no slot.  share = false (ZKP_HIP_G16_SHARE_AB=0), or a key without a shared pair: s is empty, a and b are every finite point of their
// query.  The loader appends delta and alpha / beta to a and b, so those two are never empty.
struct G16AbSlots { SlotList a, s, b; };
inline G16AbSlots g16_ab_slots(const std::vector<G1Pt>& aq, const std::vector<G1Pt>& b1q, const std::vector<uint8_t>& cls, bool share) {
    G16AbSlots out;
    const size_t n = aq.size() < b1q.size() ? aq.size() : b1q.size();
    for (size_t k = 0; k < aq.size(); k++) {
        if (aq[k].inf) continue;
        if (share && k < n && g16_shared_point(aq[k], b1q[k])) out.s.push_back({(uint16_t)k, cls[k]});
        else out.a.push_back({(uint16_t)k, cls[k]});
    }
    for (size_t k = 0; k < b1q.size(); k++) {
        if (b1q[k].inf || (share && k < n && g16_shared_point(aq[k], b1q[k]))) continue;
        out.b.push_back({(uint16_t)k, cls[k]});
    }
    return out;
}

// The targets of the A / B1 launch from the key's lists A' | S | B1': without shared slots exactly the two lists A, B1 (no empty target),
// with them three, in that order.
inline std::vector<SlotList> g16_ab_targets(const SlotList& a, const SlotList& s, const SlotList& b) {
    if (s.empty()) return {a, b};
    return {a, s, b};
}
// The chunk ranges [begin[t], end[t]) that the sums t = 0 (A) and 1 (B1) read in a layout of those targets
struct G16AbRanges { uint16_t begin[2], end[2]; };
inline G16AbRanges g16_ab_ranges(const MsmLayout& L) {
    const auto& t = L.target_chunk_begin;
    if (L.ntargets() == 3) return {{t[0], t[1]}, {t[2], t[3]}};
    return {{t[0], t[1]}, {t[1], t[2]}};
}

// ---- The key loader's plan: every finite key point is a slot of one of the G1 lists A' | S | B1' | C or of the G2 list, with its own
// window table, the digit row of the scalar it is multiplied by and the windows that scalar can occupy:
//   A = alpha + sum z_k a_query[k] + r delta ; B (G1 and G2) = beta + sum z_k b_query[k] + s delta ; C' = sum aux_k l_query[k] + sum h_i h_query[i] - rs delta
// Windows follow from the radix, which the loader chooses from the plan's point counts: the plan carries window classes (g16_plan_targets).
inline G16KeyShape g16_key_shape(const HostR1CS& cs) { return {cs.n_inst + cs.n_wit, 1u << g16_domain_log2(cs), cs.n_wit, cs.n_inst}; }

struct G16KeyPlan {
    // the finite key points in layout order: base b is slot b of the lists below, taken one after the other (make_layout and
    // make_layout_even keep a list's order), so a table index, a slot of the all-targets layout and an entry of `row` are one number
    std::vector<g1_aff> bases_g1; std::vector<g2_aff> bases_g2;
    std::vector<uint16_t> row_g1, row_g2;              // digit row per base
    std::vector<SlotList> cls_g1, cls_g2;              // G1: A' | S | B1' | C, G2: one list; entries (base, window class of g16_class_nwin)
    // The point counts the radix is chosen for (choose_radix).  They are the file's vector lengths -- a, b1 less the points they share,
    // l, h + delta x3, alpha, beta | b2 + delta, beta -- and so count points at infinity, which get no table: the sizes choose_radix
    // compares with the budget are upper bounds.  What a loaded key reports (table_bytes) counts bases_g1 / bases_g2, the finite ones.
    size_t radix_points_g1 = 0, radix_points_g2 = 0;
};
// pk: checked by g16_read_proving_key against g16_key_shape(cs).  Returns the message of the rule the circuit breaks, or nullptr.
inline const char* g16_plan_key(G16KeyPlan& P, const G16VkBlob& vk, const G16PkBlob& pk, const HostR1CS& cs, bool share_ab) {
    const G16KeyShape sh = g16_key_shape(cs);
    if (sh.nv + sh.m + 3 > 65535 || 3ull * sh.nv + sh.m + 8 > 65535) return "circuit too large for 16-bit slot indices";
    const uint32_t SC_H = sh.nv, SC_R = sh.nv + sh.m - 1, SC_S = SC_R + 1, SC_NRS = SC_R + 2, SC_ONE = SC_R + 3;     // scalar rows: z_k (nv) | h_i (m-1) | r | s | -rs | one
    std::vector<uint8_t> cls(cs.inst_nwin); cls.insert(cls.end(), cs.wit_nwin.begin(), cs.wit_nwin.end());
    P = G16KeyPlan(); P.cls_g1.resize(4); P.cls_g2.resize(1);
    auto add1 = [&](int list, const G1Pt& pt, uint32_t row, uint8_t c) {
        if (pt.inf) return;
        P.cls_g1[list].push_back({(uint16_t)P.bases_g1.size(), c}); P.bases_g1.push_back(pt.p); P.row_g1.push_back((uint16_t)row);
    };
    auto add2 = [&](const G2Pt& pt, uint32_t row, uint8_t c) {
        if (pt.inf) return;
        P.cls_g2[0].push_back({(uint16_t)P.bases_g2.size(), c}); P.bases_g2.push_back(pt.p); P.row_g2.push_back((uint16_t)row);
    };
    const G16AbSlots ab = g16_ab_slots(pk.a_query, pk.b_g1_query, cls, share_ab);
    for (auto& sl : ab.a) add1(0, pk.a_query[sl.first], sl.first, sl.second);
    add1(0, pk.delta_g1, SC_R, G16_NW_FULL); add1(0, vk.alpha_g1, SC_ONE, 1);
    for (auto& sl : ab.s) add1(1, pk.a_query[sl.first], sl.first, sl.second);
    for (auto& sl : ab.b) add1(2, pk.b_g1_query[sl.first], sl.first, sl.second);
    add1(2, pk.delta_g1, SC_S, G16_NW_FULL); add1(2, pk.beta_g1, SC_ONE, 1);
    for (uint32_t k = 0; k < sh.n_wit; k++) add1(3, pk.l_query[k], sh.n_inst + k, cls[sh.n_inst + k]);
    for (uint32_t i = 0; i + 1 < sh.m; i++) add1(3, pk.h_query[i], SC_H + i, G16_NW_FULL);
    add1(3, pk.delta_g1, SC_NRS, G16_NW_FULL);
    for (uint32_t k = 0; k < sh.nv; k++) add2(pk.b_g2_query[k], k, cls[k]);
    add2(vk.delta_g2, SC_S, G16_NW_FULL); add2(vk.beta_g2, SC_ONE, 1);
    P.radix_points_g1 = pk.a_query.size() + pk.b_g1_query.size() - ab.s.size() + pk.l_query.size() + pk.h_query.size() + 5;
    P.radix_points_g2 = pk.b_g2_query.size() + 2;
    return nullptr;
}
inline std::vector<SlotList> g16_plan_targets(const std::vector<SlotList>& cls, const G16Radix& rx) {      // the slot lists (base, windows) at a radix
    std::vector<SlotList> out = cls;
    for (auto& t : out) for (auto& sl : t) sl.second = g16_class_nwin(sl.second, rx);
    return out;
}
inline uint64_t g16_windows(const std::vector<SlotList>& targets) { uint64_t w = 0; for (auto& t : targets) for (auto& sl : t) w += sl.second; return w; }

// `part` selects the targets of a launch: G16_PART_ALL (G2), or for G1 the two launches of the split pipeline (run_g16):
// G16_PART_AB = A and B1 (scalars z only, ready after the witness step), G16_PART_C = the l / h sum (needs the QAP step).
// The A / B1 launch of a key with shared points has three targets A' | S | B1' and still two sums, over the ranges g16_ab_ranges names.
enum { G16_PART_ALL = 0, G16_PART_AB = 1, G16_PART_C = 2 };
inline std::vector<SlotList> g16_part_targets(const std::vector<SlotList>& all, int part) {
    if (part == G16_PART_ALL) return all;
    if (part == G16_PART_AB) return g16_ab_targets(all[0], all[1], all[2]);          // (S may be empty: no layout target)
    return std::vector<SlotList>(all.begin() + 3, all.end());
}
// One chunking of a launch: the layout, the digit row of each of its slots, and per sum how many of its chunks started from the offset
// point O -- every chunk of the sum's own range, so the sum is corrected by -(that many) O
struct G16Chunks { MsmLayout L; std::vector<uint16_t> scal; std::vector<uint32_t> offsets; };
inline G16Chunks g16_plan_chunks(const std::vector<SlotList>& targets, const std::vector<uint16_t>& row, int part, uint32_t chunks) {
    G16Chunks C; C.L = make_layout_even(targets, chunks);
    for (uint16_t b : C.L.slot_base) C.scal.push_back(row[b]);
    if (part == G16_PART_AB) { const G16AbRanges ab = g16_ab_ranges(C.L); for (int t = 0; t < 2; t++) C.offsets.push_back((uint32_t)ab.end[t] - ab.begin[t]); }
    else for (uint32_t t = 0; t < C.L.ntargets(); t++) C.offsets.push_back((uint32_t)C.L.target_chunk_begin[t + 1] - C.L.target_chunk_begin[t]);
    return C;
}

}  // namespace zkp
