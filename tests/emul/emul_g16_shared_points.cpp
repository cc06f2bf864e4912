// TEST INFRASTRUCTURE: the key loader's host plan (libzkp_amd/csrc/g16_share.h, g16_keyblob.h) on the CPU -- which
// variables of a key share a point, the slot lists A' | S | B1' | C and G2 with their scalar rows and windows, the two overlapping chunk
// ranges the sums A and B1 read and the offset corrections of every sum, the proving-key reader's rules, and one A / B1 launch walked
// through its step list (bp_layout.h) against double-and-add.  A program of its own (it is also run under the host sanitizers):
//   emul_g16_shared_points <equality proving key> <membership proving key>
// prints one line "ok <check>" or "FAIL <check> ..." per check and returns the number of failures.  Compiled and run by
// tests/test_emul_g16_shared_points.py; not part of the product.
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

// ---- a proving key as the loader reads it (vk, pk, cs: what g16_plan_key takes), and the fields parent_slots reads
struct Key {
    G1Pt alpha, beta, delta; std::vector<G1Pt> aq, b1q; std::vector<uint8_t> cls;
    G16VkBlob vk; G16PkBlob pk; HostR1CS cs; std::vector<uint8_t> blob;
};
static void fill_parent_fields(Key& K) {
    K.alpha = K.vk.alpha_g1; K.beta = K.pk.beta_g1; K.delta = K.pk.delta_g1; K.aq = K.pk.a_query; K.b1q = K.pk.b_g1_query;
    K.cls = K.cs.inst_nwin; K.cls.insert(K.cls.end(), K.cs.wit_nwin.begin(), K.cs.wit_nwin.end());
}
static const char* read_blob(const std::vector<uint8_t>& blob, const HostR1CS& cs, G16VkBlob& vk, G16PkBlob& pk) {
    KeyReader R{blob.data(), blob.size()};
    if (g16_read_key_prefix(R, vk) != G16_BLOB_PROVING_KEY) return "not a proving key";
    return g16_read_proving_key(R, vk, g16_key_shape(cs), pk);
}
static bool read_key(const char* path, int kind, Key& K) {
    FILE* f = fopen(path, "rb"); if (!f) return false;
    uint8_t buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) K.blob.insert(K.blob.end(), buf, buf + n);
    fclose(f);
    K.cs = kind == 0 ? build_equality_r1cs() : build_membership_r1cs();
    if (read_blob(K.blob, K.cs, K.vk, K.pk)) return false;
    fill_parent_fields(K);
    return true;
}
// The scalar rows of a proof are z_k (nv) | h_i (m - 1) | r | s | -rs | one.  parent_slots below numbers the rows of the A / B1 launch
// without the h_i and -rs: z_k = k, r = nv, s = nv + 1, one = nv + 2; model_row takes a plan's row to that numbering (0xffff: a row the
// A / B1 launch has no business reading)
static uint16_t model_row(const Key& K, uint32_t row) {
    const uint32_t nv = (uint32_t)K.pk.a_query.size(), r = nv + (uint32_t)K.pk.h_query.size();
    return (uint16_t)(row < nv ? row : row == r ? nv : row == r + 1 ? nv + 1 : row == r + 3 ? nv + 2 : 0xffffu);
}
struct Slots { std::vector<SlotList> lists; std::vector<g1_aff> bases; std::vector<uint16_t> scal; size_t shared = 0; };   // lists: A' | S | B1', (slot, windows)
// the A / B1 part of the loader's plan: its first three lists at the radix, their bases, their rows in parent_slots' numbering
static Slots plan_slots(const Key& K, const G16Radix& rx, bool share) {
    Slots S; S.lists.resize(3);
    G16KeyPlan P;
    if (g16_plan_key(P, K.vk, K.pk, K.cs, share)) return S;
    const std::vector<SlotList> t = g16_plan_targets(P.cls_g1, rx);
    S.lists.assign(t.begin(), t.begin() + 3); S.shared = t[1].size();
    const size_t n = t[0].size() + t[1].size() + t[2].size();
    S.bases.assign(P.bases_g1.begin(), P.bases_g1.begin() + n);
    for (size_t i = 0; i < n; i++) S.scal.push_back(model_row(K, P.row_g1[i]));
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
struct Walk { MsmLayout L; std::vector<uint32_t> steps, step0, offsets; std::vector<uint16_t> scal; };
static bool make_walk(Walk& W, const Slots& S, const std::vector<SlotList>& targets, uint32_t chunks, const G16Radix& rx) {
    const G16Chunks C = g16_plan_chunks(targets, S.scal, G16_PART_AB, chunks);
    W.L = C.L; W.scal = C.scal; W.offsets = C.offsets;
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

// ---- the whole plan of a committed key: lists C and G2, rows, windows, base order, point counts
static bool same_g1(const g1_aff& a, const g1_aff& b) { return fq_eq(a.x, b.x) && fq_eq(a.y, b.y); }
static bool same_g2(const g2_aff& a, const g2_aff& b) { return fq_eq(a.x.c0, b.x.c0) && fq_eq(a.x.c1, b.x.c1) && fq_eq(a.y.c0, b.y.c0) && fq_eq(a.y.c1, b.y.c1); }
template <class Pt> static size_t finite(const std::vector<Pt>& v) { size_t n = 0; for (auto& e : v) n += !e.inf; return n; }
// what one slot of a list should be: the point, its scalar row and its windows
template <class Aff> struct Want { Aff p; uint32_t row; uint32_t nwin; };
static void check_plan(const Key& K, const std::string& tag) {
    const uint32_t nv = (uint32_t)K.cls.size(), n_inst = K.cs.n_inst, nh = (uint32_t)K.pk.h_query.size();
    // rows as the loader's comment states them: z_k (nv) | h_i (m - 1) | r | s | -rs | one
    const uint32_t ROW_H = nv, ROW_R = nv + nh, ROW_S = ROW_R + 1, ROW_NRS = ROW_R + 2, ROW_ONE = ROW_R + 3;
    size_t bases_g1[2] = {0, 0}, bases_g2[2] = {0, 0};
    for (uint32_t wbits : {13u, 8u}) {
        const G16Radix rx = g16_radix(wbits);
        bool lists_ok = true, rows_ok = true, order_ok = true, sums_ok = true;
        for (int share = 0; share < 2; share++) {
            G16KeyPlan P;
            if (g16_plan_key(P, K.vk, K.pk, K.cs, share != 0)) { lists_ok = rows_ok = order_ok = sums_ok = false; continue; }
            const std::vector<SlotList> t1 = g16_plan_targets(P.cls_g1, rx), t2 = g16_plan_targets(P.cls_g2, rx);
            if (t1.size() != 4 || t2.size() != 1) { lists_ok = rows_ok = order_ok = sums_ok = false; continue; }
            bases_g1[share] = P.bases_g1.size(); bases_g2[share] = P.bases_g2.size();
            // list C: the finite points of l_query, h_query, delta; G2: of b_g2_query, delta, beta -- with the rows and windows of
            // C' = sum aux_k l_k + sum h_i H_i - rs delta and B = beta + sum z_k b_k + s delta
            std::vector<Want<g1_aff>> wc; std::vector<Want<g2_aff>> w2;
            for (uint32_t k = 0; k < K.pk.l_query.size(); k++) if (!K.pk.l_query[k].inf) wc.push_back({K.pk.l_query[k].p, n_inst + k, g16_class_nwin(K.cls[n_inst + k], rx)});
            for (uint32_t i = 0; i < nh; i++) if (!K.pk.h_query[i].inf) wc.push_back({K.pk.h_query[i].p, ROW_H + i, rx.nwin});
            wc.push_back({K.pk.delta_g1.p, ROW_NRS, rx.nwin});
            for (uint32_t k = 0; k < K.pk.b_g2_query.size(); k++) if (!K.pk.b_g2_query[k].inf) w2.push_back({K.pk.b_g2_query[k].p, k, g16_class_nwin(K.cls[k], rx)});
            w2.push_back({K.vk.delta_g2.p, ROW_S, rx.nwin}); w2.push_back({K.vk.beta_g2.p, ROW_ONE, 1});
            lists_ok = lists_ok && t1[3].size() == wc.size() && t2[0].size() == w2.size();
            for (size_t i = 0; lists_ok && i < wc.size(); i++) {
                const uint16_t b = t1[3][i].first;
                lists_ok = b < P.bases_g1.size() && same_g1(P.bases_g1[b], wc[i].p);
                rows_ok = rows_ok && lists_ok && P.row_g1[b] == wc[i].row && t1[3][i].second == wc[i].nwin;
            }
            for (size_t i = 0; lists_ok && i < w2.size(); i++) {
                const uint16_t b = t2[0][i].first;
                lists_ok = b < P.bases_g2.size() && same_g2(P.bases_g2[b], w2[i].p);
                rows_ok = rows_ok && lists_ok && P.row_g2[b] == w2[i].row && t2[0][i].second == w2[i].nwin;
            }
            // A' and B1' end with delta (r / s, every window) and alpha / beta (the row "one", one window); every slot before them, and
            // every slot of S, reads the row of its variable (which variable, and its windows: each_term_once, switch_off_is_parent)
            for (int l : {0, 2}) {
                const SlotList& t = t1[l];
                if (t.size() < 2) { rows_ok = false; continue; }
                const auto &d = t[t.size() - 2], &o = t[t.size() - 1];
                rows_ok = rows_ok && same_g1(P.bases_g1[d.first], K.pk.delta_g1.p) && P.row_g1[d.first] == (l == 0 ? ROW_R : ROW_S) && d.second == rx.nwin;
                rows_ok = rows_ok && same_g1(P.bases_g1[o.first], l == 0 ? K.vk.alpha_g1.p : K.pk.beta_g1.p) && P.row_g1[o.first] == ROW_ONE && o.second == 1;
                for (size_t i = 0; i + 2 < t.size(); i++) rows_ok = rows_ok && P.row_g1[t[i].first] < nv;
            }
            for (auto& sl : t1[1]) rows_ok = rows_ok && P.row_g1[sl.first] < nv;
            // the bases are numbered in list order, so slot s of a layout of all lists is base s (the loader's tables, its host rows and
            // the layouts' slot_base agree without a re-sort), and a part's slots are a contiguous run of bases
            uint16_t next = 0;
            for (auto& t : t1) for (auto& sl : t) order_ok = order_ok && sl.first == next++;
            order_ok = order_ok && next == P.bases_g1.size() && P.row_g1.size() == P.bases_g1.size();
            next = 0; for (auto& sl : t2[0]) order_ok = order_ok && sl.first == next++;
            order_ok = order_ok && next == P.bases_g2.size() && P.row_g2.size() == P.bases_g2.size();
            std::vector<SlotList> all1; for (auto& t : t1) if (!t.empty()) all1.push_back(t);
            const size_t n_ab = t1[0].size() + t1[1].size() + t1[2].size();
            for (uint32_t chunks : {4u, 64u, 229u}) {
                const MsmLayout La = make_layout_even(all1, chunks), L2 = make_layout_even(t2, chunks), Lw = make_layout(all1, 32);
                const MsmLayout Lab = make_layout_even(g16_part_targets(t1, G16_PART_AB), chunks), Lc = make_layout_even(g16_part_targets(t1, G16_PART_C), chunks);
                for (size_t i = 0; i < La.slot_base.size(); i++) order_ok = order_ok && La.slot_base[i] == i && Lw.slot_base[i] == i;
                for (size_t i = 0; i < L2.slot_base.size(); i++) order_ok = order_ok && L2.slot_base[i] == i;
                for (size_t i = 0; i < Lab.slot_base.size(); i++) order_ok = order_ok && Lab.slot_base[i] == i;
                for (size_t i = 0; i < Lc.slot_base.size(); i++) order_ok = order_ok && Lc.slot_base[i] == n_ab + i;
                order_ok = order_ok && La.nslots() == P.bases_g1.size() && Lw.nslots() == La.nslots() && L2.nslots() == P.bases_g2.size() && Lab.nslots() == n_ab && Lc.nslots() == wc.size();
            }
            // win_g1 / win_g2 (mixed additions per proof): the windows of the parent's A and B1 less those of the shared slots, and of C | of G2
            uint64_t want1 = windows_of(parent_slots(K, rx).lists) - (uint64_t)t1[1].size() * rx.nwin, want2 = 0;
            for (auto& w : wc) want1 += w.nwin;
            for (auto& w : w2) want2 += w.nwin;
            sums_ok = sums_ok && g16_windows(t1) == want1 && g16_windows(t2) == want2 && t1[1].size() == (share ? 110u : 0u);
            // the point counts the radix is chosen from: the file's vector lengths, points at infinity included
            if (wbits == 13) {
                const size_t n1 = K.pk.a_query.size() + K.pk.b_g1_query.size() - (share ? 110 : 0) + K.pk.l_query.size() + K.pk.h_query.size() + 5, n2 = K.pk.b_g2_query.size() + 2;
                // ... and the bases that get a table (what key_info's table_bytes is computed from): the finite points, delta three times, alpha, beta
                const size_t f1 = finite(K.pk.a_query) + finite(K.pk.b_g1_query) - (share ? 110 : 0) + finite(K.pk.l_query) + finite(K.pk.h_query) + 5, f2 = finite(K.pk.b_g2_query) + 2;
                report("point_counts_" + tag + (share ? "_shared" : "_switch_off"),
                       P.radix_points_g1 == n1 && P.radix_points_g2 == n2 && P.bases_g1.size() == f1 && P.bases_g2.size() == f2 && f1 <= n1 && f2 <= n2,
                       std::to_string(P.radix_points_g1) + " " + std::to_string(P.radix_points_g2) + " | " + std::to_string(P.bases_g1.size()) + " " + std::to_string(P.bases_g2.size()));
            }
        }
        const std::string r = tag + "_w" + std::to_string(wbits);
        report("lists_c_g2_" + r, lists_ok); report("rows_windows_" + r, rows_ok); report("slot_is_base_" + r, order_ok); report("window_sums_" + r, sums_ok);
    }
    // tests/test_gpu_g16_shared_points.py expects of key_info: with the switch off a key's tables are larger by 110 G1 points' blocks
    // (110 x slot_ent x 64 bytes) and by no G2 block.  Only that difference is pinned by a GPU test; no absolute table size is.
    report("table_points_" + tag, bases_g1[0] == bases_g1[1] + 110 && bases_g2[0] == bases_g2[1] && bases_g2[1] > 0);
}

// ---- the offset corrections: per sum, how many chunks started from the offset point
// counted here from the layout's slots alone: chunk c belongs to the list that holds its first slot
static bool check_offsets(const std::vector<SlotList>& lists, int part, uint32_t chunks) {
    const std::vector<SlotList> targets = g16_part_targets(lists, part);
    std::vector<uint16_t> row; for (auto& t : lists) for (size_t i = 0; i < t.size(); i++) row.push_back((uint16_t)row.size());
    const G16Chunks C = g16_plan_chunks(targets, row, part, chunks);
    std::vector<uint32_t> per_target(targets.size(), 0);
    for (uint32_t c = 0; c < C.L.nchunks(); c++) {
        size_t slot = C.L.chunk_begin[c], t = 0;
        while (t < targets.size() && slot >= targets[t].size()) slot -= targets[t++].size();
        if (t == targets.size()) return false;
        per_target[t]++;
    }
    bool ok = C.scal.size() == C.L.nslots();
    for (size_t i = 0; ok && i < C.scal.size(); i++) ok = C.scal[i] == row[C.L.slot_base[i]];
    if (part != G16_PART_AB) {
        ok = ok && C.offsets.size() == targets.size();
        for (size_t t = 0; ok && t < targets.size(); t++) ok = C.offsets[t] == per_target[t];
        return ok;
    }
    // A sums the chunks of A' and S, B1 those of S and B1'; without S the two lists' own chunks
    const G16AbRanges ab = g16_ab_ranges(C.L);
    const bool three = targets.size() == 3;
    const uint32_t a = per_target[0], sh = three ? per_target[1] : 0, b = per_target[three ? 2 : 1];
    return ok && C.offsets.size() == 2 && C.offsets[0] == a + sh && C.offsets[1] == sh + b &&
           ab.begin[0] == 0 && ab.end[0] == a + sh && ab.begin[1] == a && ab.end[1] == a + sh + b && ab.end[1] == C.L.nchunks();
}
static void check_offsets_of_key(const Key& K, const std::string& tag, std::initializer_list<uint32_t> counts) {
    bool ok = true;
    for (uint32_t wbits : {13u, 8u})
        for (int share = 0; share < 2; share++) {
            G16KeyPlan P;
            if (g16_plan_key(P, K.vk, K.pk, K.cs, share != 0)) { ok = false; continue; }
            const std::vector<SlotList> t1 = g16_plan_targets(P.cls_g1, g16_radix(wbits)), t2 = g16_plan_targets(P.cls_g2, g16_radix(wbits));
            ok = ok && g16_part_targets(t1, G16_PART_AB).size() == (t1[1].empty() ? 2u : 3u) && g16_part_targets(t1, G16_PART_C).size() == 1;
            for (uint32_t chunks : counts) {
                ok = ok && check_offsets(t1, G16_PART_AB, chunks) && check_offsets(t1, G16_PART_C, chunks);
                if (!t2[0].empty()) ok = ok && check_offsets(t2, G16_PART_ALL, chunks);
            }
        }
    report("offset_counts_" + tag, ok);
}

// ---- the proving-key reader's rules, on blobs made from a committed key
static void check_reader(const Key& K) {
    const std::string malformed = "malformed proving key (expected ark-serialize uncompressed ProvingKey<Bn254>)";
    auto refused = [&](const std::vector<uint8_t>& blob, const std::string& want) {
        G16VkBlob vk; G16PkBlob pk; const char* why = read_blob(blob, K.cs, vk, pk);
        return why && want == why;
    };
    { G16VkBlob vk; G16PkBlob pk; report("reader_accepts_committed_key", read_blob(K.blob, K.cs, vk, pk) == nullptr); }
    std::vector<uint8_t> b(K.blob.begin(), K.blob.end() - 10);
    report("reader_truncated", refused(b, malformed));
    b = K.blob; b.push_back(0);
    report("reader_trailing_bytes", refused(b, malformed));
    // a_query one point short: a well-formed key of another shape
    const size_t o_delta = (size_t)g16_vk_blob_bytes(K.vk.abc.size()) + 64, o_a = o_delta + 64, nv = K.pk.a_query.size();
    b.assign(K.blob.begin(), K.blob.begin() + o_a);
    for (int i = 0; i < 8; i++) b.push_back((uint8_t)((uint64_t)(nv - 1) >> (8 * i)));
    b.insert(b.end(), K.blob.begin() + o_a + 8, K.blob.begin() + o_a + 8 + 64 * (nv - 1));
    b.insert(b.end(), K.blob.begin() + o_a + 8 + 64 * nv, K.blob.end());
    report("reader_a_query_length", refused(b, "proving key does not match the circuit shape"));
    b = K.blob; memset(b.data() + o_delta, 0, 64); b[o_delta + 63] = 0x40;
    report("reader_delta_g1_infinity", refused(b, "degenerate proving key"));
}

static void check_committed_key(const char* path, int kind) {
    const std::string tag = kind == 0 ? "equality" : "membership";
    Key K;
    if (!read_key(path, kind, K)) { report("read_key_" + tag, false, path); return; }
    check_plan(K, tag);
    check_offsets_of_key(K, tag, {3u, 7u, 64u, 229u});
    if (kind == 0) check_reader(K);
    for (uint32_t wbits : {13u, 8u}) {
        const G16Radix rx = g16_radix(wbits);
        const Slots S = plan_slots(K, rx, true), off = plan_slots(K, rx, false), P = parent_slots(K, rx);
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
    Key K; K.vk.alpha_g1 = small_point(1001); K.pk.beta_g1 = small_point(1002); K.pk.delta_g1 = small_point(1003);
    for (uint32_t m : a) K.pk.a_query.push_back(small_point(m));
    for (uint32_t m : b) K.pk.b_g1_query.push_back(small_point(m));
    // a circuit of that many variables and no rows: one instance variable, domain size 1 (no h_query); l_query, b_g2_query and the G2
    // points at infinity, so that lists C and G2 hold delta_g1 alone and nothing
    K.cs.inst_nwin = {cls[0]}; K.cs.wit_nwin.assign(cls.begin() + 1, cls.end()); K.cs.n_wit = (uint32_t)cls.size() - 1;
    K.pk.l_query.assign(K.cs.n_wit, G1Pt{true, {}}); K.pk.b_g2_query.assign(cls.size(), G2Pt{true, {}});
    K.vk.beta_g2.inf = K.vk.delta_g2.inf = true;
    fill_parent_fields(K);
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
            const Slots S = plan_slots(K, rx, true), P = parent_slots(K, rx);
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
        K.b1q[1].p = aff_neg(K.b1q[1].p); K.pk.b_g1_query[1].p = K.b1q[1].p;
        const G16AbSlots ab = g16_ab_slots(K.aq, K.b1q, K.cls, true);
        report("negation_not_shared", ab.s == SlotList{{0, F}} && ab.a == SlotList{{1, F}} && ab.b == SlotList{{1, F}});
    }
    // One A / B1 launch on the host: 10 variables, 3 shared (one of each window class), an infinite pair, a finite point against an infinite
    // one both ways, a pair equal at different indices.  Chunk accumulators start from an offset point O and the sums take -(chunks) O,
    // as on the device; entries are rebuilt by double-and-add from the (point, window, |digit|) a step's entry index stands for.
    const Key K = synthetic_key({21, 22, 23, 0, 24, 0, 25, 26, 27, 28}, {21, 32, 23, 0, 0, 35, 22, 26, 37, 38}, {F, F, U, F, F, F, F, 1, U, F});
    check_offsets_of_key(K, "synthetic", {3u, 5u, 16u});
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
        const Slots S = plan_slots(K, rx, true);
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
                for (uint32_t c = ab.begin[t]; c < ab.end[t]; c++) sum = jac_add(sum, partial[c]);
                for (uint32_t k = 0; k < W.offsets[t]; k++) corr = jac_add(corr, O);
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
