// Groth16 key loader (host only): key points that the sums A and B1 share.  A = alpha + sum z_k a_query[k] + r delta and
// B1 = beta + sum z_k b_g1_query[k] + s delta walk the same scalar rows z_k, and where a_query[k] and b_g1_query[k] are one point the
// two sums hold the same term: such a variable gets ONE slot (one table, one gather, one mixed addition per window), and the chunks that
// hold those slots are added into both sums.  The A / B1 launch is laid out A' | S | B1' (S: the shared slots); the sums read the two
// overlapping chunk ranges A' u S and S u B1' (ReduceView::target_chunk_end, bp_steps.h).  The rule reads the key's points only -- nothing
// about the circuit.  Compiled for the host by tests/emul/emul_g16_shared_points.cpp too.
#pragma once
#include <cstdint>
#include <vector>
#include "bp_layout.h"
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

}  // namespace zkp
