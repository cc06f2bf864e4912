// Groth16 key check: the step functions of the kernels that check what a key puts on the device -- the window tables
// k_g16_build_table builds, the G2 points of the key file, and the weighted sums of the b_g1_query / b_g2_query twins.  Host and device
// (ZKP_HD): tests/emul/emul_g16_keycheck.cpp runs the same functions against bigint entries.
//
// A slot's tables at radix rx hold, for window w, the entries e = 0 .. g16_win_ent(rx, w) - 1 with entry[e] = (e + 1) * 2^g16_win_bit(rx, w) * P
// in affine form.  They are right exactly when
//   (a) entry 0 of window 0 is P,
//   (b) entry[e] == entry[e - 1] + entry[0] for every e >= 1 of a window            (e = 1 is a doubling),
//   (c) 2 * (last entry of window w) == entry 0 of window w + 1                     (the uneven 2^14 form included: 2 * 2^14 entries of
//       window 16 end at 2^239 P, where window 17 begins)
// -- (a) pins the first entry, (c) every other window's first entry, (b) the rest of each window.  No scalar multiplication, no inversion:
// the two affine operands are added into Jacobian form (Z = the difference of the x coordinates) and the stored entry is compared
// projectively, X == x Z^2 and Y == y Z^3.  Stored coordinates need not be canonical (packed entries are < 2.4 p, plain ones < 2 p): every
// comparison is modulo p (f_is_zero).
#pragma once
#include "g16_verify.h"      // g2_in_subgroup

namespace zkp {

// ---- one stored coordinate -> bn254_fq.h's form.  fmt9: the MSM loops' packed nine-limb form (eight words); otherwise ten plain limbs
ZKP_HD inline fq kc_ld_fq(const uint32_t* w, bool fmt9) {
    if (fmt9) return fq9_to_fq(fq9_unpack8(w));
    fq r; ZKP_UNROLL for (int k = 0; k < 10; k++) r.v[k] = w[k];
    return fq_reduce_weak(r);
}
template <class F> struct KcEntry;
template <> struct KcEntry<fq> {
    static constexpr uint32_t NC = 2;
    static ZKP_HD inline Aff<fq> load(const uint32_t* e, bool fmt9) { const uint32_t cw = fmt9 ? 8u : 10u; return Aff<fq>{kc_ld_fq(e, fmt9), kc_ld_fq(e + cw, fmt9)}; }
};
template <> struct KcEntry<fq2> {      // x.c0, x.c1, y.c0, y.c1
    static constexpr uint32_t NC = 4;
    static ZKP_HD inline Aff<fq2> load(const uint32_t* e, bool fmt9) {
        const uint32_t cw = fmt9 ? 8u : 10u;
        return Aff<fq2>{fq2{kc_ld_fq(e, fmt9), kc_ld_fq(e + cw, fmt9)}, fq2{kc_ld_fq(e + 2 * cw, fmt9), kc_ld_fq(e + 3 * cw, fmt9)}};
    }
};
// words of a stored entry (g16_table_entry_words of the launchers, as a constant expression)
template <class F> ZKP_HD constexpr uint32_t kc_entry_words(bool fmt9) { return KcEntry<F>::NC * (fmt9 ? 8u : 10u); }

// ---- the predicates
// the affine point `ent` is the projective point j
template <class F> ZKP_HD inline bool kc_is_point(const Jac<F>& j, const Aff<F>& ent) {
    if (jac_is_inf(j)) return false;
    const F zz = f_sq(j.Z);
    return f_is_zero(f_sub(j.X, f_mul(ent.x, zz))) && f_is_zero(f_sub(j.Y, f_mul(ent.y, f_mul(zz, j.Z))));
}
// rule (a), and every comparison of two stored points: equal modulo p
template <class F> ZKP_HD inline bool kc_same_point(const Aff<F>& a, const Aff<F>& b) { return f_is_zero(f_sub(a.x, b.x)) && f_is_zero(f_sub(a.y, b.y)); }
// prev + first, both affine and finite, in Jacobian form with Z = x_first - x_prev (7 M + 2 S):
//   X = r^2 - H^2 (x_prev + x_first), Y = r (x_prev H^2 - X) - y_prev H^3, Z = H      with H = x_first - x_prev, r = y_first - y_prev
// H == 0: the doubling (prev == first, entry 1 of a window), or prev == -first, the point at infinity (which no entry is).
template <class F> ZKP_HD inline Jac<F> kc_add_affine(const Aff<F>& prev, const Aff<F>& first) {
    const F H = f_sub(first.x, prev.x), r = f_sub(first.y, prev.y);
    if (f_is_zero(H)) return f_is_zero(r) ? jac_dbl(jac_from_aff(prev)) : jac_infinity<F>();
    const F HH = f_sq(H), HHH = f_mul(HH, H);
    Jac<F> s;
    s.X = f_sub(f_sq(r), f_mul(HH, f_add(prev.x, first.x)));
    s.Y = f_sub(f_mul(r, f_sub(f_mul(prev.x, HH), s.X)), f_mul(prev.y, HHH));
    s.Z = H;
    return s;
}
// rule (b): ent == prev + first
template <class F> ZKP_HD inline bool kc_entry_follows(const Aff<F>& prev, const Aff<F>& first, const Aff<F>& ent) { return kc_is_point(kc_add_affine(prev, first), ent); }
// rule (c): next0 == 2 * last
template <class F> ZKP_HD inline bool kc_window_joins(const Aff<F>& last, const Aff<F>& next0) { return kc_is_point(jac_dbl(jac_from_aff(last)), next0); }

// ---- the table check's lane: entry t of slot `slot`'s block (t < rx.slot_ent).  Adjacent t are adjacent entries of one window, so a wave
// reads consecutive entries and its window's first entry is the same address for all of its lanes (windows are multiples of 64 entries).
// Entry 0 of a window checks rule (a) in window 0 and rule (c) against the window below otherwise: a broken join is reported at
// (window, entry 0) of the UPPER window.
struct KcTableView {
    const uint32_t* table; const uint32_t* bases;      // bases: [nslots] plain affine points (20 / 40 words), as k_g16_build_table reads them
    uint32_t nslots, fmt9; G16Radix rx;
    uint32_t* pair_bad;                                 // [nslots * rx.nwin]: bad entries of each (slot, window), zeroed by the launcher
    uint32_t* out;                                      // KC_OUT_WORDS words, see below
};
// out[0]: number of (slot, window) pairs with a bad entry; out[1]: bad entries in all; out[2], out[3]: low and high word of the least
// key slot << 40 | window << 32 | entry over the bad entries (all ones when there is none) -- the first bad location in table order
constexpr uint32_t KC_OUT_WORDS = 4;
ZKP_HD inline uint64_t kc_location_key(uint32_t slot, uint32_t win, uint32_t ent) { return (uint64_t)slot << 40 | (uint64_t)win << 32 | ent; }
ZKP_HD inline void kc_window_of(const G16Radix& rx, uint32_t t, uint32_t& win, uint32_t& ent) {      // entry t of a slot's block -> (window, entry)
    win = t / rx.nent; ent = t % rx.nent;
    if (rx.uneven && win >= 16u) { win = t < 18u * rx.nent ? 16u : 17u; ent = t - g16_win_off(rx, win); }
}
template <class F> ZKP_HD inline bool kc_table_entry_ok(const KcTableView& V, uint32_t slot, uint32_t win, uint32_t ent) {
    const bool fmt9 = V.fmt9 != 0;
    const uint32_t OW = kc_entry_words<F>(fmt9);
    const uint32_t* blk = V.table + (size_t)slot * V.rx.slot_ent * OW;
    const uint32_t* w0 = blk + (size_t)g16_win_off(V.rx, win) * OW;
    const Aff<F> e = KcEntry<F>::load(w0 + (size_t)ent * OW, fmt9);
    if (ent) return kc_entry_follows(KcEntry<F>::load(w0 + (size_t)(ent - 1) * OW, fmt9), KcEntry<F>::load(w0, fmt9), e);
    if (win == 0) return kc_same_point(KcEntry<F>::load(V.bases + (size_t)slot * kc_entry_words<F>(false), false), e);
    const uint32_t* below = blk + ((size_t)g16_win_off(V.rx, win - 1) + g16_win_ent(V.rx, win - 1) - 1) * OW;
    return kc_window_joins(KcEntry<F>::load(below, fmt9), e);
}

// ---- the subgroup check's lane: point i of [n] plain affine G2 points (40 words each) -> ok[i] = 1 inside the prime-order subgroup.
// r * Q is the identity, as g2_in_subgroup (g16_verify.h) has it, by plain double-and-add over the bits of r: g2_in_subgroup's windowed
// ladder keeps sixteen multiples of Q in an array it indexes by the digit -- 4 KB of scratch per lane, which the runtime reserves for
// every wave slot of the device (2 GB) from the first launch on.  A REFUSED load, or a key check in a process that only verifies, must
// not leave that behind; here the cost is 127 more mixed additions per point, once per load.  tests/emul/emul_g16_keycheck.cpp holds the two forms against each other.
ZKP_HD inline bool kc_g2_in_subgroup(const g2_aff& q) {
    g2_jac acc = jac_from_aff(q);                       // bit 253, the top bit of r
    for (int i = 252; i >= 0; i--) {
        acc = jac_dbl(acc);
        if ((FrParams::mod(i >> 5) >> (i & 31)) & 1u) acc = jac_madd(acc, q);
    }
    return jac_is_inf(acc);
}
ZKP_HD inline void step_kc_subgroup(const uint32_t* pts, uint8_t* ok, uint32_t i) { ok[i] = kc_g2_in_subgroup(KcEntry<fq2>::load(pts + (size_t)i * 40, false)) ? 1 : 0; }

// ---- the twin sums' lane: rho_i * point i for a 128-bit weight (four words each) -> partial i of a one-row sum (k_sum_t reads them).
// Plain double-and-add for the same reason as above: no table of multiples, no scratch.
template <class F> ZKP_HD inline Jac<F> kc_weighted(const uint32_t* pts, const uint32_t* rho, uint32_t i) {
    const Aff<F> p = KcEntry<F>::load(pts + (size_t)i * kc_entry_words<F>(false), false);
    const uint32_t* k = rho + 4 * (size_t)i;
    Jac<F> acc = jac_infinity<F>();
    for (int b = 127; b >= 0; b--) {
        acc = jac_dbl(acc);                             // (the point at infinity stays there: Z = 0)
        if ((k[b >> 5] >> (b & 31)) & 1u) acc = jac_madd(acc, p);
    }
    return acc;
}

}  // namespace zkp
