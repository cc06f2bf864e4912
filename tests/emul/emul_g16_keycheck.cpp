// TEST INFRASTRUCTURE: the key check's step functions (libzkp_amd/csrc/g16_keycheck.h) and its view of a key blob (g16_keyblob.h) on
// the CPU.  Entries arrive in their STORED form -- packed (eight words per coordinate, the integer x * 2^261 mod p plus a multiple of p) or
// plain (ten 26-bit limbs of x * 2^260 mod p plus a multiple of p) -- built from bigints by tests/test_emul_g16_keycheck.py.  Compiled by
// build_emul; not part of the product.
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/g16_share.h"
#include "../../libzkp_amd/csrc/g16_keycheck.h"
using namespace zkp;

namespace {
template <class F> int follows(const uint32_t* prev, const uint32_t* first, const uint32_t* ent, bool fmt9) {
    return kc_entry_follows(KcEntry<F>::load(prev, fmt9), KcEntry<F>::load(first, fmt9), KcEntry<F>::load(ent, fmt9)) ? 1 : 0;
}
template <class F> int joins(const uint32_t* last, const uint32_t* next0, bool fmt9) { return kc_window_joins(KcEntry<F>::load(last, fmt9), KcEntry<F>::load(next0, fmt9)) ? 1 : 0; }
template <class F> int same(const uint32_t* base, const uint32_t* ent, bool fmt9) { return kc_same_point(KcEntry<F>::load(base, false), KcEntry<F>::load(ent, fmt9)) ? 1 : 0; }
}  // namespace

extern "C" {

uint32_t emul_kc_entry_words(int g2, int fmt9) { return g2 ? kc_entry_words<fq2>(fmt9 != 0) : kc_entry_words<fq>(fmt9 != 0); }
// rule (b): ent == prev + first
int emul_kc_entry_follows(int g2, int fmt9, const uint32_t* prev, const uint32_t* first, const uint32_t* ent) {
    return g2 ? follows<fq2>(prev, first, ent, fmt9 != 0) : follows<fq>(prev, first, ent, fmt9 != 0);
}
// rule (c): next0 == 2 * last
int emul_kc_window_joins(int g2, int fmt9, const uint32_t* last, const uint32_t* next0) { return g2 ? joins<fq2>(last, next0, fmt9 != 0) : joins<fq>(last, next0, fmt9 != 0); }
// rule (a): the stored entry is the base point (plain limbs, as the loader uploads it)
int emul_kc_same_point(int g2, int fmt9, const uint32_t* base_plain, const uint32_t* ent) { return g2 ? same<fq2>(base_plain, ent, fmt9 != 0) : same<fq>(base_plain, ent, fmt9 != 0); }

// the geometry the check walks: out = {nwin, slot_ent}; win[w] = {first entry, entries, first bit} by g16_win_off / _ent / _bit
int emul_kc_geom(uint32_t wbits, uint32_t uneven, uint32_t* out, uint32_t* win) {
    const G16Radix rx = g16_radix(wbits, uneven != 0);
    out[0] = rx.nwin; out[1] = rx.slot_ent;
    for (uint32_t w = 0; w < rx.nwin; w++) { win[3 * w] = g16_win_off(rx, w); win[3 * w + 1] = g16_win_ent(rx, w); win[3 * w + 2] = g16_win_bit(rx, w); }
    return 0;
}
// entry t of a slot's block -> out = {window, entry} (the kernel's lane mapping)
void emul_kc_window_of(uint32_t wbits, uint32_t uneven, uint32_t t, uint32_t* out) { kc_window_of(g16_radix(wbits, uneven != 0), t, out[0], out[1]); }
// the whole lane of the table check on a host copy of a table: 1 ok, 0 bad
int emul_kc_table_entry_ok(int g2, int fmt9, uint32_t wbits, uint32_t uneven, const uint32_t* table, const uint32_t* bases_plain, uint32_t nslots, uint32_t slot, uint32_t win, uint32_t ent) {
    KcTableView V{table, bases_plain, nslots, fmt9 ? 1u : 0u, g16_radix(wbits, uneven != 0), nullptr, nullptr};
    return (g2 ? kc_table_entry_ok<fq2>(V, slot, win, ent) : kc_table_entry_ok<fq>(V, slot, win, ent)) ? 1 : 0;
}

// POINTS without a device: the blob of circuit `kind` parsed as the loader parses it, its finite G2 points tested by g2_in_subgroup on the
// host.  out = {format (0 proving key, 1 verifying key), finite G2 points, of those outside the subgroup, the first such point's report
// index or 0xffffffff, twins (both finite), infinity mismatches, b_g1_query points at infinity, b_g2_query points at infinity}.
// Returns 0, -1 malformed, -2 refused by the shape rules, -3 if kc_g2_in_subgroup and g2_in_subgroup disagree on a point.
int emul_kc_points(int kind, const uint8_t* blob, uint64_t len, uint32_t* out) {
    const HostR1CS cs = kind == G16_EQUALITY ? build_equality_r1cs() : build_membership_r1cs();
    KeyReader R{blob, len};
    G16VkBlob B; G16PkBlob Q;
    const int format = g16_read_key_prefix(R, B);
    if (format == G16_BLOB_MALFORMED) return -1;
    const bool is_pk = format == G16_BLOB_PROVING_KEY;
    if (is_pk ? g16_read_proving_key(R, B, g16_key_shape(cs), Q) : g16_check_verifying_key(B, cs.n_inst)) return -2;
    const G16G2List L = g16_key_g2_points(B, is_pk ? &Q : nullptr);
    out[0] = (uint32_t)format; out[1] = (uint32_t)L.pts.size(); out[2] = 0; out[3] = 0xffffffffu;
    for (size_t i = 0; i < L.pts.size(); i++) {
        uint32_t plain[40]; memcpy(plain, &L.pts[i], sizeof plain);
        uint8_t ok = 0; step_kc_subgroup(plain, &ok, 0);
        if (!ok) { if (!out[2]) out[3] = L.index[i]; out[2]++; }
        if ((ok != 0) != g2_in_subgroup(L.pts[i])) return -3;          // the check's double-and-add against the verifier's windowed ladder
    }
    const G16Twins T = g16_key_twins(Q);
    out[4] = (uint32_t)T.index.size(); out[5] = T.inf_mismatches; out[6] = out[7] = 0;
    for (auto& e : Q.b_g1_query) out[6] += e.inf;
    for (auto& e : Q.b_g2_query) out[7] += e.inf;
    return 0;
}
// the name a loader message gives report index `index`
void emul_kc_point_name(uint32_t index, char* out, uint32_t cap) { g16_g2_point_name(out, cap, index); }

}
