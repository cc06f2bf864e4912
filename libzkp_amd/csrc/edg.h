// Fixed-base tables of the 130 Bulletproofs generators sized for HBM, and the steps that build and read them.
//
// Round 4.  The ed25519 MSMs of the range prover (bulletproofs.rs:138,150 -> RangeProof::prove_single) walked
// radix-1024 tables streamed through LDS: 60 KB sub-tables, 26 additions per 253-bit scalar, one 1024-lane workgroup per CU.  Measured this
// round (tools/gather_calib.hip, profiles/r04_gather_calib.jsonl): lanes that gather ONE entry each from a sub-table of a few hundred KB
// somewhere in a multi-GB table are served at ~48 G gathers/s whether the entry is 64 or 128 bytes -- the memory system is bound by
// requests, not bytes, for this pattern -- so the tables move to HBM at radix 2^16: 16 windows of 32 768 affine-Niels entries per
// generator, 128-byte slots, 8.7 GB for the 130 generators; **16 additions per scalar instead of 26**, no LDS, no barrier, 256-lane
// workgroups of four independent waves that fit beside the Groth16 gather kernels' waves (a 1024-lane, 120 KB workgroup had to wait
// for a whole CU to drain).  Digits are limb-aligned: a 32-bit word of the scalar is two signed 16-bit digits.
//
// Entry e of (generator b, window w) = (e + 1) * 2^(16 w) * G_b as (y + x, y - x, 2 d x y), each the canonical 255-bit integer in
// eight 32-bit words; words 24..31 of the slot are padding (one 128-byte line per gather).
//
// Smaller radices for devices with less free HBM (DESIGN.md "Generator tables sized to free HBM"): the geometry is a run-time EdgGeom,
// 2^10 .. 2^16, chosen when the table is built.  The EDG_* constants and the geometry-less functions below are its radix-2^16 instance.
#pragma once
#include "bp_steps.h"

namespace zkp {

constexpr uint32_t EDG_WBITS = 16, EDG_NWIN = 16, EDG_NENT = 1u << 15, EDG_DIGW = 8, EDG_NWIN_U64 = 5;
constexpr uint32_t EDG_SLOT_W = 32, EDG_ENTRY_W = 24;                       // words per table slot / payload words
constexpr uint32_t EDG_SEG = 64, EDG_NSEG = EDG_NENT / EDG_SEG, EDG_INV = 8;   // builder: 64-entry runs, one inversion per 8 entries

// Table geometry at radix 2^wbits, wbits = 10..16: nwin windows cover a scalar below l < 2^253 plus the carry of the signed recoding
// (nwin * wbits >= 254), nwin_u64 a 64-bit value plus its carry (>= 65); nent = 2^(wbits - 1) entries per window (|digit| <= nent),
// nseg builder runs of EDG_SEG entries.  Every nwin is <= 26 = 2 * DIGW, so the digit rows keep their 13-word pitch.
struct EdgGeom { uint32_t wbits, nwin, nwin_u64, nent, nseg; };
constexpr uint32_t EDG_WBITS_MIN = 10, EDG_WBITS_MAX = 16;
ZKP_HD constexpr EdgGeom edg_geom(uint32_t wbits) {
    return EdgGeom{wbits, sc_signed_ndigits(wbits, 254), sc_signed_ndigits(wbits, 65), 1u << (wbits - 1), (1u << (wbits - 1)) / EDG_SEG};
}
static_assert(edg_geom(EDG_WBITS).nwin == EDG_NWIN && edg_geom(EDG_WBITS).nwin_u64 == EDG_NWIN_U64 && edg_geom(EDG_WBITS).nent == EDG_NENT &&
              edg_geom(EDG_WBITS).nseg == EDG_NSEG, "the EDG_* constants are the radix-2^16 geometry");
static_assert(edg_geom(EDG_WBITS_MIN).nwin <= 2 * DIGW, "digit rows hold 2 * DIGW digits");
ZKP_HD constexpr size_t edg_table_words(const EdgGeom& g) { return (size_t)NBASE * g.nwin * g.nent * EDG_SLOT_W; }
ZKP_HD constexpr size_t edg_slot(const EdgGeom& g, uint32_t b, uint32_t w, uint32_t e) { return (((size_t)b * g.nwin + w) * g.nent + e) * EDG_SLOT_W; }
ZKP_HD constexpr size_t edg_table_words() { return edg_table_words(edg_geom(EDG_WBITS)); }
ZKP_HD constexpr size_t edg_slot(uint32_t b, uint32_t w, uint32_t e) { return edg_slot(edg_geom(EDG_WBITS), b, w, e); }

ZKP_HD inline ge_niels edg_unpack(const uint32_t e[EDG_ENTRY_W]) {
    ge_niels n; n.ypx = fe_fromwords(e); n.ymx = fe_fromwords(e + 8); n.xy2d = fe_fromwords(e + 16);
    return n;
}
// acc + d * (window base), the entry |d| - 1 of the window already fetched
ZKP_HD inline ge edg_accumulate(const ge& acc, int32_t d, const uint32_t e[EDG_ENTRY_W]) {
    ge_niels n = edg_unpack(e);
    n = ge_niels_select(d < 0, ge_niels_neg(n), n);
    return ge_madd(acc, n);
}
// reference form of one chunk (host emulation, tests): entries read straight from the table
ZKP_HD inline ge edg_accumulate_from(const EdgGeom& g, const ge& acc, int32_t d, const uint32_t* table, uint32_t base, uint32_t w) {
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
    return edg_accumulate(acc, d, table + edg_slot(g, base, w, mag - 1));
}
ZKP_HD inline ge edg_accumulate_from(const ge& acc, int32_t d, const uint32_t* table, uint32_t base, uint32_t w) { return edg_accumulate_from(edg_geom(EDG_WBITS), acc, d, table, base, w); }

// ---- table construction (one-time, on the device; each function is the body of one lane).  The geometry-less forms build radix 2^16.
// 1. window bases: 2^(wbits w) * G_b for w = 0..nwin-1.            lane = generator
ZKP_HD inline void edg_step_bases(const EdgGeom& g, const uint32_t* gens /*[NBASE][40]*/, uint32_t* bases /*[NBASE][nwin][40]*/, uint32_t b) {
    ge p = ld_ge(gens, b, 0, 1);
    for (uint32_t w = 0; w < g.nwin; w++) {
        st_ge(bases, b * g.nwin + w, 0, 1, p);
        for (uint32_t k = 0; k < g.wbits; k++) p = ge_dbl(p);
    }
}
// 2. run starts: (64 s + 1) * P for s = 0..nseg-1, P = window base.     lane = (generator, window)
ZKP_HD inline void edg_step_starts(const EdgGeom& g, const uint32_t* bases, uint32_t* starts /*[NBASE * nwin][nseg][40]*/, uint32_t bw) {
    const ge p = ld_ge(bases, bw, 0, 1);
    ge step = p;
    for (uint32_t k = 0; k < 6; k++) step = ge_dbl(step);                 // 64 P
    ge acc = p;
    for (uint32_t s = 0; s < g.nseg; s++) { st_ge(starts, (size_t)bw * g.nseg + s, 0, 1, acc); acc = ge_add(acc, step); }
}
// 3. a run of 64 consecutive multiples, left in their slots as projective (X, Y, Z) limbs.     lane = (generator, window, run)
ZKP_HD inline void edg_step_fill(const EdgGeom& g, const uint32_t* bases, const uint32_t* starts, uint32_t* table, uint32_t bw, uint32_t s) {
    const ge p = ld_ge(bases, bw, 0, 1);
    ge acc = ld_ge(starts, (size_t)bw * g.nseg + s, 0, 1);
    uint32_t* q = table + ((size_t)bw * g.nent + (size_t)s * EDG_SEG) * EDG_SLOT_W;
    for (uint32_t e = 0; e < EDG_SEG; e++) {
        ZKP_UNROLL for (int k = 0; k < 10; k++) { q[k] = acc.X.v[k]; q[10 + k] = acc.Y.v[k]; q[20 + k] = acc.Z.v[k]; }
        q += EDG_SLOT_W;
        acc = ge_add(acc, p);
    }
}
ZKP_HD inline void edg_step_bases(const uint32_t* gens, uint32_t* bases, uint32_t b) { edg_step_bases(edg_geom(EDG_WBITS), gens, bases, b); }
ZKP_HD inline void edg_step_starts(const uint32_t* bases, uint32_t* starts, uint32_t bw) { edg_step_starts(edg_geom(EDG_WBITS), bases, starts, bw); }
ZKP_HD inline void edg_step_fill(const uint32_t* bases, const uint32_t* starts, uint32_t* table, uint32_t bw, uint32_t s) { edg_step_fill(edg_geom(EDG_WBITS), bases, starts, table, bw, s); }
// 4. eight slots from projective to packed affine Niels with ONE field inversion (Montgomery's trick).     lane = 8 consecutive slots
// (every geometry: nent is a multiple of EDG_INV, so a group never straddles two windows)
ZKP_HD inline fe edg_fe_invert(const fe& z) {              // z^(p-2) = (z^(2^252-3))^8 * z^3
    fe t = fe_pow22523(z);
    t = fe_sq(fe_sq(fe_sq(t)));
    return fe_mul(t, fe_mul(fe_sq(z), z));
}
ZKP_HD inline void edg_step_affine(uint32_t* table, size_t group) {
    uint32_t* q0 = table + group * EDG_INV * EDG_SLOT_W;
    fe pre[EDG_INV];
    fe run = fe_one();
    for (uint32_t i = 0; i < EDG_INV; i++) {
        fe z; ZKP_UNROLL for (int k = 0; k < 10; k++) z.v[k] = q0[(size_t)i * EDG_SLOT_W + 20 + k];
        pre[i] = run; run = fe_mul(run, z);
    }
    fe inv = edg_fe_invert(run);
    const fe d2 = fe_const_d2();
    for (uint32_t i = EDG_INV; i-- > 0;) {
        uint32_t* q = q0 + (size_t)i * EDG_SLOT_W;
        fe X, Y, Z; ZKP_UNROLL for (int k = 0; k < 10; k++) { X.v[k] = q[k]; Y.v[k] = q[10 + k]; Z.v[k] = q[20 + k]; }
        const fe zi = fe_mul(inv, pre[i]);
        inv = fe_mul(inv, Z);
        const fe x = fe_mul(X, zi), y = fe_mul(Y, zi);
        fe_towords(q, fe_add(y, x));
        fe_towords(q + 8, fe_sub(y, x));
        fe_towords(q + 16, fe_mul(fe_mul(x, y), d2));
        ZKP_UNROLL for (int k = EDG_ENTRY_W; k < (int)EDG_SLOT_W; k++) q[k] = 0;
    }
}
// 5. self-check of the finished table, all of it: entry[e] + entry[0] == entry[e + 1] inside a window, 2 * entry[nent - 1]
// of window w == entry[0] of window w + 1 (2^wbits * the window base), and entry[0] of window 0 == the generator.  By induction every slot then holds the multiple it stands for.
// lane = (generator, window, e); returns false on a mismatch
ZKP_HD inline bool edg_niels_equals(const ge& p, const uint32_t e[EDG_ENTRY_W]) {       // projective p against an affine entry
    const ge_niels n = edg_unpack(e);
    return fe_eq(fe_add(p.Y, p.X), fe_mul(n.ypx, p.Z)) && fe_eq(fe_sub(p.Y, p.X), fe_mul(n.ymx, p.Z));
}
ZKP_HD inline ge edg_point_of(const uint32_t e[EDG_ENTRY_W]) {                          // affine entry -> extended point
    const ge_niels n = edg_unpack(e);
    // y = (ypx + ymx) / 2, x = (ypx - ymx) / 2: keep the factor 2 projectively (X : Y : Z) = (ypx - ymx : ypx + ymx : 2)
    ge p; p.X = fe_carry(fe_sub(n.ypx, n.ymx)); p.Y = fe_carry(fe_add(n.ypx, n.ymx)); p.Z = fe_zero(); p.Z.v[0] = 2;
    // T = X Y / Z: scale to (2X : 2Y : 4) so that T = X Y is exact
    p.T = fe_mul(p.X, p.Y); p.X = fe_carry(fe_add(p.X, p.X)); p.Y = fe_carry(fe_add(p.Y, p.Y)); p.Z.v[0] = 4;
    return p;
}
ZKP_HD inline bool edg_step_check(const EdgGeom& g, const uint32_t* table, const uint32_t* gens, uint32_t b, uint32_t w, uint32_t e) {
    const uint32_t* cur = table + edg_slot(g, b, w, e);
    if (e + 1 < g.nent) {
        const ge sum = ge_madd(edg_point_of(cur), edg_unpack(table + edg_slot(g, b, w, 0)));
        if (!edg_niels_equals(sum, cur + EDG_SLOT_W)) return false;
    } else if (w + 1 < g.nwin) {
        if (!edg_niels_equals(ge_dbl(edg_point_of(cur)), table + edg_slot(g, b, w + 1, 0))) return false;
    }
    if (w == 0 && e == 0 && !edg_niels_equals(ld_ge(gens, b, 0, 1), cur)) return false;
    return true;
}
ZKP_HD inline bool edg_step_check(const uint32_t* table, const uint32_t* gens, uint32_t b, uint32_t w, uint32_t e) { return edg_step_check(edg_geom(EDG_WBITS), table, gens, b, w, e); }

}  // namespace zkp
