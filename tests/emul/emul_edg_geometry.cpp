// TEST INFRASTRUCTURE: the generator tables of every radix 2^10 .. 2^16 (libzkp_amd/csrc/edg.h: EdgGeom) on the CPU -- the digit
// recoding the prover's steps store, the table builder's steps and self-check, and one MSM launch walked the way k_msm_gather walks it
// (step list of bp_layout.h over edg-format entries).  Compiled by tests/test_emul_edg_geometry.py itself; not part of the product.
#include "../../libzkp_amd/csrc/bp_layout.h"
#include "../../libzkp_amd/csrc/bp_verify.h"
#include "../../libzkp_amd/csrc/edg.h"
#include <vector>
#include <cstdlib>
#include <cstring>
using namespace zkp;

static sc sc_of(const uint32_t raw[8]) { sc r; for (int k = 0; k < 8; k++) r.v[k] = raw[k]; return r; }
// k * P by plain double-and-add over the 256 bits of k (the independent route everything here is checked against)
static ge mul_ref(const ge& p, const sc& k) {
    ge acc = ge_identity();
    for (int bit = 255; bit >= 0; bit--) { acc = ge_dbl(acc); if ((k.v[bit >> 5] >> (bit & 31)) & 1u) acc = ge_add(acc, p); }
    return acc;
}
// (e + 1) * 2^(wbits w) * G as packed affine-Niels words
static void ref_entry(const EdgGeom& g, const ge& gen, uint32_t w, uint32_t e, uint32_t out[EDG_ENTRY_W]) {
    ge p = gen;
    for (uint32_t k = 0; k < g.wbits * w; k++) p = ge_dbl(p);
    const sc m = sc_words(e + 1, 0, 0, 0, 0, 0, 0, 0);
    const ge acc = mul_ref(p, m);
    const fe zi = host_fe_invert(acc.Z);
    const fe x = fe_mul(acc.X, zi), y = fe_mul(acc.Y, zi);
    fe_towords(out, fe_add(y, x)); fe_towords(out + 8, fe_sub(y, x)); fe_towords(out + 16, fe_mul(fe_mul(x, y), fe_const_d2()));
}
static bool same_point(const ge& a, const ge& b) {
    uint32_t x[8], y[8]; ge_ristretto_encode(x, a); ge_ristretto_encode(y, b);
    return memcmp(x, y, 32) == 0;
}

extern "C" {
// out = {wbits, nwin, nwin_u64, nent, nseg}
void emul_edg_geom(uint32_t wbits, uint32_t out[5]) { const EdgGeom g = edg_geom(wbits); out[0] = g.wbits; out[1] = g.nwin; out[2] = g.nwin_u64; out[3] = g.nent; out[4] = g.nseg; }

// the digit row st_digits_raw stores for `raw` at radix 2^wbits (the prover's and the verifier's steps): DIGW words, two 16-bit digits each
void emul_edg_digits(uint32_t wbits, const uint32_t raw[8], uint32_t out[DIGW]) {
    for (uint32_t k = 0; k < DIGW; k++) out[k] = 0;
    st_digits_raw(out, 0, 0, 1, sc_of(raw), wbits);
}

// Builds window w of generator `gen` (all nent slots, plus the first run of window w + 1) with the builder's own steps at radix 2^wbits,
// runs the self-check over window w, compares entries 0, nent - 1 and `nsample` - 2 seeded others with double-and-add, checks the
// padding words, and flips one word to see the self-check catch it.  Returns the number of failures of any kind.
int emul_edg_window_geom(uint32_t wbits, uint32_t gen, uint32_t w, uint32_t nsample, uint32_t seed) {
    const EdgGeom g = edg_geom(wbits);
    ge gens[NBASE]; host_generators(gens);
    std::vector<uint32_t> g1(GE_W); st_ge(g1.data(), 0, 0, 1, gens[gen]);
    std::vector<uint32_t> bases((size_t)g.nwin * GE_W), starts((size_t)g.nwin * g.nseg * GE_W), table(edg_table_words(g) / NBASE, 0xDEADBEEFu);
    edg_step_bases(g, g1.data(), bases.data(), 0);
    const uint32_t last = w + 1 < g.nwin ? w + 1 : w;
    for (uint32_t ww = w; ww <= last; ww++) {
        edg_step_starts(g, bases.data(), starts.data(), ww);
        const uint32_t runs = ww == w ? g.nseg : 1;
        for (uint32_t s = 0; s < runs; s++) edg_step_fill(g, bases.data(), starts.data(), table.data(), ww, s);
        for (size_t q = 0; q < (size_t)runs * EDG_SEG / EDG_INV; q++) edg_step_affine(table.data(), (size_t)ww * g.nent / EDG_INV + q);
    }
    int bad = 0;
    for (uint32_t e = 0; e < g.nent; e++) if (!edg_step_check(g, table.data(), g1.data(), 0, w, e)) bad++;
    uint32_t x = seed * 2654435761u + 1;
    for (uint32_t k = 0; k < nsample; k++) {
        x = x * 1664525u + 1013904223u;
        const uint32_t e = k == 0 ? 0 : k == 1 ? g.nent - 1 : (x >> 8) % g.nent;
        uint32_t want[EDG_ENTRY_W]; ref_entry(g, gens[gen], w, e, want);
        if (memcmp(want, table.data() + edg_slot(g, 0, w, e), sizeof want) != 0) bad++;
        for (uint32_t pad = EDG_ENTRY_W; pad < EDG_SLOT_W; pad++) if (table[edg_slot(g, 0, w, e) + pad] != 0) bad++;
    }
    const uint32_t e = (x >> 4) % (g.nent - 1);
    table[edg_slot(g, 0, w, e + 1) + 5] ^= 0x100u;
    if (edg_step_check(g, table.data(), g1.data(), 0, w, e) && edg_step_check(g, table.data(), g1.data(), 0, w, e + 1)) bad++;
    return bad;
}

// One MSM launch of the prover's phase 1 for `rows` proofs of n bits at radix 2^wbits: the layout's slots get seeded scalars (raw < l for
// full-width slots, 64-bit values for the value slot, +1 / 0 / -1 single-window digits for A's bit slots), stored by st_digits_raw; every
// chunk is walked through its flat step list (make_gather_steps) -- digit word, half, entry index = step's first entry + |d| - 1 -- with
// the entry built by double-and-add from the (generator, window, entry) the index stands for; the chunk sums of each target must equal
// sum s_i * G_i computed directly.  Checked for the slot-aligned and the even chunkings.  Returns the number of (layout, target, row)
// mismatches, or -1 when an entry index falls outside the table.
int emul_edg_msm_phase1(uint32_t wbits, uint32_t n, uint32_t rows, uint32_t seed) {
    const EdgGeom g = edg_geom(wbits);
    ge gens[NBASE]; host_generators(gens);
    const std::vector<SlotList> targets = targets_phase1(n, (uint8_t)g.nwin, (uint8_t)g.nwin_u64);
    uint32_t nslots = 0; for (auto& t : targets) nslots += (uint32_t)t.size();
    const sc L = sc_words(0x5cf5d3edu, 0x5812631au, 0xa2f79cd6u, 0x14def9deu, 0u, 0u, 0u, 0x10000000u);
    std::vector<uint32_t> digits((size_t)nslots * DIGW * rows, 0);
    std::vector<ge> want(targets.size() * rows, ge_identity());
    uint64_t x = seed * 0x9E3779B97F4A7C15ull + 7;
    auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
    uint32_t slot = 0;
    for (size_t t = 0; t < targets.size(); t++)
        for (const auto& sl : targets[t]) {
            for (uint32_t row = 0; row < rows; row++) {
                sc k = sc_zero();
                if (sl.second == 1) {                                   // A's bit terms: one window, digit +1 / 0 / -1
                    const uint32_t c = (uint32_t)(rnd() % 3);
                    digits[(size_t)slot * DIGW * rows + row] = c == 0 ? 1u : c == 1 ? 0u : 0xFFFFu;
                    k = c == 0 ? sc_words(1, 0, 0, 0, 0, 0, 0, 0) : c == 1 ? sc_zero() : sc_words(L.v[0] - 1, L.v[1], L.v[2], L.v[3], 0, 0, 0, L.v[7]);
                } else {
                    const uint64_t a = rnd(), b = rnd(), c = rnd(), d = rnd();
                    if (slot == P1_V) k = sc_words((uint32_t)a, (uint32_t)(a >> 32), 0, 0, 0, 0, 0, 0);          // v * B: nwin_u64 windows
                    else k = sc_words((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32), (uint32_t)c, (uint32_t)(c >> 32), (uint32_t)d, (uint32_t)(d >> 32) & 0x0fffffffu);
                    if (row == 0 && slot == P1_V + 1) k = sc_words(L.v[0] - 1, L.v[1], L.v[2], L.v[3], 0, 0, 0, L.v[7]);      // l - 1
                    if (row == 0 && slot == P1_A) k = sc_words(~0u, ~0u, ~0u, ~0u, ~0u, ~0u, ~0u, 0x1fffffffu);               // 2^253 - 1
                    if (row == 1 && slot == P1_V) k = sc_words(~0u, ~0u, 0, 0, 0, 0, 0, 0);                                   // 2^64 - 1
                    st_digits_raw(digits.data(), slot, row, rows, k, wbits);
                }
                want[t * rows + row] = ge_add(want[t * rows + row], mul_ref(gens[sl.first], k));
            }
            slot++;
        }
    const GatherShape shape{g.nent, g.nwin * g.nent, 0u, DIGW};
    const uint64_t table_entries = (uint64_t)NBASE * g.nwin * g.nent;
    int bad = 0;
    for (int variant = 0; variant < 2; variant++) {
        const MsmLayout Lo = variant == 0 ? make_layout(targets, 32) : make_layout_even(targets, 12);
        std::vector<uint32_t> steps, step0;
        if (!make_gather_steps(Lo, nullptr, shape, steps, step0)) return -1;
        for (uint32_t row = 0; row < rows; row++)
            for (uint32_t t = 0; t < Lo.ntargets(); t++) {
                ge sum = ge_identity();
                for (uint32_t c = Lo.target_chunk_begin[t]; c < Lo.target_chunk_begin[t + 1]; c++) {
                    ge acc = ge_identity();
                    for (uint32_t i = step0[c]; i < step0[c + 1]; i++) {
                        const uint32_t first = steps[2 * i], ds = steps[2 * i + 1];
                        const uint32_t word = digits[(size_t)(ds >> 1) * rows + row];
                        const int32_t d = (int32_t)(int16_t)(word >> (16 * (ds & 1u)));
                        if (d == 0) continue;
                        const uint64_t idx = (uint64_t)first + (uint32_t)(d < 0 ? -d : d) - 1;
                        if (idx >= table_entries || (uint32_t)(d < 0 ? -d : d) > g.nent) return -1;
                        const uint32_t b = (uint32_t)(idx / (g.nwin * g.nent)), w = (uint32_t)(idx / g.nent % g.nwin), e = (uint32_t)(idx % g.nent);
                        uint32_t entry[EDG_ENTRY_W]; ref_entry(g, gens[b], w, e, entry);
                        acc = edg_accumulate(acc, d, entry);
                    }
                    sum = ge_add(sum, acc);
                }
                if (!same_point(sum, want[t * rows + row])) bad++;
            }
    }
    return bad;
}
}
