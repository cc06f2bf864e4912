// Groth16 key blobs (host only): the ark-serialize uncompressed point reader of the key loader, and the rule that tells the two
// formats zkp_hip_groth16_load_key accepts apart.  ProvingKey<Bn254> starts with its VerifyingKey<Bn254>
//   { alpha_g1 (64 B), beta_g2, gamma_g2, delta_g2 (128 B each), u64 count, count x gamma_abc_g1 (64 B each) }
// so a blob is read as that prefix first: if it ENDS exactly there it is a verifying key, if bytes remain it is a proving key and the
// reader goes on from where the prefix ended.  No length table and no flag.  Compiled for the host by tests/emul/emul_g16_keyblob.cpp too.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "bn254_g.h"

namespace zkp {

struct KeyReader {
    const uint8_t* p; uint64_t left; bool ok = true;
    const uint8_t* take(uint64_t n) { if (left < n) { ok = false; return nullptr; } const uint8_t* q = p; p += n; left -= n; return q; }
    uint64_t u64() { const uint8_t* q = take(8); uint64_t v = 0; if (q) for (int i = 0; i < 8; i++) v |= (uint64_t)q[i] << (8 * i); return v; }
};
// canonical-encoding check on the serialized words
inline bool raw_lt_p(const uint32_t w[8]) { for (int i = 7; i >= 0; i--) { if (w[i] < FqParams::mod(i)) return true; if (w[i] > FqParams::mod(i)) return false; } return false; }
// returns 0 ok (inf set if point at infinity), -1 malformed
inline int parse_g1(KeyReader& R, bool& inf, g1_aff& out) {
    const uint8_t* q = R.take(64); if (!q) return -1;
    uint8_t buf[64]; memcpy(buf, q, 64);
    const uint8_t flags = buf[63] & 0xC0; buf[63] &= 0x3F;
    if (flags == 0xC0) return -1;                        // SWFlags::from_u8 rejects both bits set
    inf = flags & 0x40; if (inf) return 0;
    uint32_t w[16]; memcpy(w, buf, 64);
    if (!raw_lt_p(w) || !raw_lt_p(w + 8)) return -1;
    out.x = fq_from_raw(w); out.y = fq_from_raw(w + 8);
    const fq rhs = fq_add(fq_mul(fq_sq(out.x), out.x), fq_from_u64(3));
    return fq_eq(fq_sq(out.y), rhs) ? 0 : -1;
}
inline int parse_g2(KeyReader& R, bool& inf, g2_aff& out) {
    const uint8_t* q = R.take(128); if (!q) return -1;
    uint8_t buf[128]; memcpy(buf, q, 128);
    const uint8_t flags = buf[127] & 0xC0; buf[127] &= 0x3F;
    if (flags == 0xC0) return -1;
    inf = flags & 0x40; if (inf) return 0;
    uint32_t w[32]; memcpy(w, buf, 128);
    for (int k = 0; k < 4; k++) if (!raw_lt_p(w + 8 * k)) return -1;
    out.x = fq2{fq_from_raw(w), fq_from_raw(w + 8)}; out.y = fq2{fq_from_raw(w + 16), fq_from_raw(w + 24)};
    const fq2 b2 = f_mul(fq2{fq_from_u64(3), fq_zero()}, f_inv(fq2{fq_from_u64(9), fq_from_u64(1)}));
    const fq2 lhs = f_sq(out.y), rhs = f_add(f_mul(f_sq(out.x), out.x), b2);
    return (fq_eq(lhs.c0, rhs.c0) && fq_eq(lhs.c1, rhs.c1)) ? 0 : -1;
}
struct G1Pt { bool inf; g1_aff p; };
struct G2Pt { bool inf; g2_aff p; };
inline int parse_vec_g1(KeyReader& R, std::vector<G1Pt>& v) {
    const uint64_t n = R.u64(); if (!R.ok || n > (1u << 24)) return -1;
    v.resize(n); for (auto& e : v) if (parse_g1(R, e.inf, e.p)) return -1;
    return 0;
}
inline int parse_vec_g2(KeyReader& R, std::vector<G2Pt>& v) {
    const uint64_t n = R.u64(); if (!R.ok || n > (1u << 24)) return -1;
    v.resize(n); for (auto& e : v) if (parse_g2(R, e.inf, e.p)) return -1;
    return 0;
}

// VerifyingKey { alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 }: alone, or as the head of a proving key
struct G16VkBlob { G1Pt alpha_g1{}; G2Pt beta_g2{}, gamma_g2{}, delta_g2{}; std::vector<G1Pt> abc; };
enum { G16_BLOB_MALFORMED = -1, G16_BLOB_PROVING_KEY = 0, G16_BLOB_VERIFYING_KEY = 1 };
// Reads the prefix and classifies the blob; R is left behind gamma_abc_g1 (a proving key's beta_g1 comes next).  MALFORMED: the prefix
// itself is truncated or holds a word that is no field element / a point off the curve.  Points at infinity are valid encodings here:
// what each format makes of them is its loader's business (g16_check_verifying_key for a verifying key).
inline int g16_read_key_prefix(KeyReader& R, G16VkBlob& vk) {
    if (parse_g1(R, vk.alpha_g1.inf, vk.alpha_g1.p) || parse_g2(R, vk.beta_g2.inf, vk.beta_g2.p) || parse_g2(R, vk.gamma_g2.inf, vk.gamma_g2.p) ||
        parse_g2(R, vk.delta_g2.inf, vk.delta_g2.p) || parse_vec_g1(R, vk.abc) || !R.ok) return G16_BLOB_MALFORMED;
    return R.left == 0 ? G16_BLOB_VERIFYING_KEY : G16_BLOB_PROVING_KEY;
}
inline uint64_t g16_vk_blob_bytes(uint64_t n_ic) { return 64 + 3 * 128 + 8 + 64 * n_ic; }
// what a verifying key must satisfy to be usable for the circuit with n_inst instance variables (the constant one included): the message
// of the first rule it breaks, or nullptr
inline const char* g16_check_verifying_key(const G16VkBlob& vk, uint32_t n_inst) {
    if (vk.abc.size() != n_inst) return "verifying key does not match the circuit shape (gamma_abc_g1 count)";
    if (vk.alpha_g1.inf || vk.beta_g2.inf || vk.gamma_g2.inf || vk.delta_g2.inf) return "degenerate verifying key (alpha, beta, gamma or delta at infinity)";
    for (const auto& e : vk.abc) if (e.inf) return "degenerate verifying key (a gamma_abc_g1 point at infinity)";
    return nullptr;
}

// What follows the verifying key in ProvingKey<Bn254>: beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query
struct G16PkBlob { G1Pt beta_g1{}, delta_g1{}; std::vector<G1Pt> a_query, b_g1_query, h_query, l_query; std::vector<G2Pt> b_g2_query; };
// the vector lengths of a circuit's key: nv variables (n_inst instance ones, the constant one included, and n_wit witnesses), domain size m
struct G16KeyShape { uint32_t nv, m, n_wit, n_inst; };
// Reads the rest of a proving key (R as g16_read_key_prefix left it) and checks it against the circuit: nullptr, or the message of the first
// rule it breaks -- the format (nothing may follow l_query), the vector lengths, a key point no proof can do without at infinity
inline const char* g16_read_proving_key(KeyReader& R, const G16VkBlob& vk, const G16KeyShape& s, G16PkBlob& pk) {
    if (parse_g1(R, pk.beta_g1.inf, pk.beta_g1.p) || parse_g1(R, pk.delta_g1.inf, pk.delta_g1.p) || parse_vec_g1(R, pk.a_query) || parse_vec_g1(R, pk.b_g1_query) ||
        parse_vec_g2(R, pk.b_g2_query) || parse_vec_g1(R, pk.h_query) || parse_vec_g1(R, pk.l_query) || !R.ok || R.left != 0)
        return "malformed proving key (expected ark-serialize uncompressed ProvingKey<Bn254>)";
    if (pk.a_query.size() != s.nv || pk.b_g1_query.size() != s.nv || pk.b_g2_query.size() != s.nv || pk.h_query.size() != s.m - 1 || pk.l_query.size() != s.n_wit ||
        vk.abc.size() != s.n_inst)
        return "proving key does not match the circuit shape";
    if (vk.alpha_g1.inf || pk.beta_g1.inf || pk.delta_g1.inf || vk.beta_g2.inf || vk.delta_g2.inf) return "degenerate proving key";
    return nullptr;
}

// ---- the key check's view of a key (g16_keycheck.h).  The finite G2 points in file order, each with the index a report names it by:
// 0 beta_g2, 1 gamma_g2, 2 delta_g2, 3 + i b_g2_query[i] (pk == nullptr: a verifying key, the first three only).  These are the points ark's
// Validate::Yes tests for membership of the prime-order subgroup; G1 has cofactor 1 and needs no such test.
struct G16G2List { std::vector<uint32_t> index; std::vector<g2_aff> pts; };
inline G16G2List g16_key_g2_points(const G16VkBlob& vk, const G16PkBlob* pk) {
    G16G2List L;
    auto add = [&](uint32_t ix, const G2Pt& p) { if (!p.inf) { L.index.push_back(ix); L.pts.push_back(p.p); } };
    add(0, vk.beta_g2); add(1, vk.gamma_g2); add(2, vk.delta_g2);
    if (pk) for (size_t i = 0; i < pk->b_g2_query.size(); i++) add(3u + (uint32_t)i, pk->b_g2_query[i]);
    return L;
}
inline void g16_g2_point_name(char* out, size_t cap, uint32_t index) {
    static const char* head[3] = {"beta_g2", "gamma_g2", "delta_g2"};
    if (index < 3) snprintf(out, cap, "%s", head[index]); else snprintf(out, cap, "b_g2_query[%u]", index - 3);
}
// The twins of a proving key: the indices at which b_g1_query and b_g2_query are both finite, and how many indices have one of the two at
// infinity and the other not (a key in which the two vectors do not hold the same scalars)
struct G16Twins { std::vector<uint32_t> index; uint32_t inf_mismatches = 0; };
inline G16Twins g16_key_twins(const G16PkBlob& pk) {
    G16Twins T;
    const size_t n = pk.b_g1_query.size() < pk.b_g2_query.size() ? pk.b_g1_query.size() : pk.b_g2_query.size();
    for (size_t i = 0; i < n; i++) {
        if (pk.b_g1_query[i].inf != pk.b_g2_query[i].inf) T.inf_mismatches++;
        else if (!pk.b_g1_query[i].inf) T.index.push_back((uint32_t)i);
    }
    return T;
}

}  // namespace zkp
