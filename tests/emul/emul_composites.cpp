// TEST INFRASTRUCTURE: host build of the composite-proof call's steps (composite_steps.h): the framing walk, the digest lane, the pack and
// fold steps.  Loaded by tests/test_emul_composites.py as a shared library; as a program of its own (it has a main) it walks containers
// whose inner proofs lie at every source alignment inside an allocation of exactly the blob's size, which is the form to build with
// -fsanitize=address,undefined: a read outside the blob is then an error, not a value.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../libzkp_amd/csrc/composite_steps.h"
using namespace zkp;

extern "C" {
uint32_t emul_comp_lane_bytes(void) { return (uint32_t)sizeof(CompLane); }
int emul_comp_utf8_ok(const uint8_t* s, uint32_t n) { return cp_utf8_ok(s, n) ? 1 : 0; }
// the walk of container [lo, hi) of a blob readable over [blob_lo, blob_hi): out = ok nproofs nmeta digest_at hashed proof_bytes;
// order_out (1000 entries) receives the hashed metadata entries' offsets.  Returns ok.
int emul_comp_walk(const uint8_t* blob, uint64_t lo, uint64_t hi, uint64_t blob_lo, uint64_t blob_hi, uint64_t* out, uint32_t* order_out) {
    std::vector<uint32_t> order;
    const CompWalk W = comp_walk(blob, lo, hi, blob_lo, blob_hi, order);
    out[0] = W.ok; out[1] = W.nproofs; out[2] = W.nmeta; out[3] = W.digest_at; out[4] = W.hashed; out[5] = W.proof_bytes;
    for (size_t k = 0; k < order.size() && k < CP_MAX_ITEMS; k++) order_out[k] = order[k];
    return W.ok;
}
// What the call makes of n containers, digests only: status[i] = 1 or 2 as zkp_hip_verify_composites writes it under
// ZKP_HIP_COMPOSITES_INTEGRITY_ONLY, digests[32 i ..] = what the lane computed (zeros for a container the walk refused).  The lanes run in
// the host's order (hashed length, descending) over one shared order list, as the kernel's do.
void emul_comp_statuses(uint64_t n, const uint8_t* blob, const uint64_t* off, uint8_t* status, uint8_t* digests) {
    std::vector<CompWalk> walk; std::vector<uint32_t> order;
    for (uint64_t i = 0; i < n; i++) walk.push_back(comp_walk(blob, off[i], off[i + 1], off[0], off[n], order));
    std::vector<uint32_t> by_len;
    for (uint64_t i = 0; i < n; i++) { status[i] = CP_MALFORMED; memset(digests + 32 * i, 0, 32); if (walk[i].ok) by_len.push_back((uint32_t)i); }
    std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b) { return walk[a].hashed > walk[b].hashed; });
    for (uint32_t i : by_len) {
        const CompLane L = comp_lane(walk[i], off[i], walk[i].order0, i);
        uint32_t h[8];
        const bool same = step_comp_digest(blob, blob + off[0], blob + off[n], L, order.data(), h);
        for (int k = 0; k < 8; k++) for (int b = 0; b < 4; b++) digests[32 * i + 4 * k + b] = (uint8_t)(h[k] >> (24 - 8 * b));
        if (same) status[i] = CP_ACCEPTED;
    }
}
// pack: every lane of a 64-wide wave, envelope by envelope
void emul_comp_pack(uint8_t* packed, const uint64_t* poff, const uint8_t* blob, uint64_t bytes, const uint64_t* src, uint64_t envelopes) {
    for (uint64_t e = 0; e < envelopes; e++) for (uint32_t lane = 0; lane < 64; lane++) step_comp_pack(packed, poff, blob, src, blob, blob + bytes, e, lane, 64);
}
void emul_comp_fold(uint8_t* status, const uint8_t* ok, const uint64_t* env0, uint64_t m) {
    for (uint64_t c = 0; c < m; c++) status[c] = step_comp_fold(status[c], ok, env0, c);
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

void put32(std::vector<uint8_t>& v, uint32_t x) { for (int b = 0; b < 4; b++) v.push_back((uint8_t)(x >> (8 * b))); }
struct Meta { std::vector<uint8_t> key, value; };
// a container of format-valid inner proofs of the given lengths (scheme 9) and metadata in the given order, with the digest of the hashed
// stream written out from first principles (sha256_bytes over a flat copy); `hash_order`: the entries' indices in hash order
std::vector<uint8_t> container(const std::vector<uint32_t>& proof_lens, const std::vector<Meta>& meta, const std::vector<uint32_t>& hash_order, uint32_t salt) {
    std::vector<uint8_t> c = {'C', 'O', 'M', 'P'}, flat;
    const char* tag = "COMPOSITE_PROOF:";
    flat.assign(tag, tag + 16);
    put32(c, (uint32_t)proof_lens.size()); put32(c, (uint32_t)meta.size()); put32(flat, (uint32_t)proof_lens.size());
    for (uint32_t len : proof_lens) {
        std::vector<uint8_t> p = {2, 9};
        put32(p, len - 10); put32(p, 0);
        for (uint32_t k = 10; k < len; k++) p.push_back((uint8_t)(k * 37 + salt + len));
        put32(c, len); c.insert(c.end(), p.begin(), p.end()); flat.insert(flat.end(), p.begin(), p.end());
    }
    std::vector<std::vector<uint8_t>> ser;
    for (const Meta& m : meta) {
        std::vector<uint8_t> e;
        put32(e, (uint32_t)m.key.size()); e.insert(e.end(), m.key.begin(), m.key.end());
        put32(e, (uint32_t)m.value.size()); e.insert(e.end(), m.value.begin(), m.value.end());
        c.insert(c.end(), e.begin(), e.end()); ser.push_back(e);
    }
    for (uint32_t k : hash_order) flat.insert(flat.end(), ser[k].begin(), ser[k].end());
    uint8_t d[32];
    sha256_bytes(d, flat.data(), flat.size());
    c.insert(c.end(), d, d + 32);
    return c;
}
}  // namespace

int main() {
    // inner proofs of 10..13 and 60..190 bytes behind 0..7 bytes of another container, values of 0..130 bytes (every residue of the hashed length mod
    // 64), the blob an allocation of exactly its size: the last container ends at the last readable byte
    for (uint32_t before = 0; before < 8; before++) for (uint32_t vl = 0; vl <= 130; vl++) {
        std::vector<Meta> meta = {{{'b'}, std::vector<uint8_t>(vl, (uint8_t)vl)}, {{'a', 'b'}, {1, 2, 3}}, {{'a'}, {}}};
        const std::vector<uint8_t> c = container({10, 11, 12, 13, 60 + vl}, meta, {2, 1, 0}, before + vl);
        std::vector<uint8_t> blob(before, 0xEE);
        blob.insert(blob.end(), c.begin(), c.end());
        std::vector<uint8_t> exact(blob);          // capacity == size: nothing readable behind it
        exact.shrink_to_fit();
        const uint64_t off[3] = {0, before, exact.size()};
        uint8_t status[2], digests[64];
        emul_comp_statuses(2, exact.data(), off, status, digests);
        EXPECT(status[0] == CP_MALFORMED && status[1] == CP_ACCEPTED);
        EXPECT(memcmp(digests + 32, exact.data() + exact.size() - 32, 32) == 0);
        exact[exact.size() - 1] ^= 1;
        emul_comp_statuses(2, exact.data(), off, status, digests);
        EXPECT(status[1] == CP_MALFORMED);
        // the pack step on the same blob: the five proofs, back to back
        exact[exact.size() - 1] ^= 1;
        std::vector<uint64_t> src, poff = {0};
        uint64_t at = before + 12;
        for (int k = 0; k < 5; k++) { const uint64_t len = ve_le(exact.data() + at, 4); src.push_back(at + 4); poff.push_back(poff.back() + len); at += 4 + len; }
        std::vector<uint8_t> packed(poff.back());
        emul_comp_pack(packed.data(), poff.data(), exact.data(), exact.size(), src.data(), 5);
        for (int k = 0; k < 5; k++) EXPECT(memcmp(packed.data() + poff[k], exact.data() + src[k], poff[k + 1] - poff[k]) == 0);
    }
    // String::from_utf8's corner cases
    const struct { std::vector<uint8_t> s; bool ok; } utf8[] = {
        {{}, true}, {{'k'}, true}, {{0xC3, 0xA9}, true}, {{0xE2, 0x82, 0xAC}, true}, {{0xF0, 0x9F, 0x98, 0x80}, true}, {{0xF4, 0x8F, 0xBF, 0xBF}, true},
        {{0xED, 0x9F, 0xBF}, true}, {{0xEE, 0x80, 0x80}, true}, {{0xC0, 0x80}, false}, {{0xC1, 0xBF}, false}, {{0xE0, 0x9F, 0xBF}, false},
        {{0xED, 0xA0, 0x80}, false}, {{0xF0, 0x8F, 0xBF, 0xBF}, false}, {{0xF4, 0x90, 0x80, 0x80}, false}, {{0xF5, 0x80, 0x80, 0x80}, false},
        {{0x80}, false}, {{0xC3}, false}, {{0xE2, 0x82}, false}, {{0xF0, 0x9F, 0x98}, false}, {{'a', 0xE2, 0x82, 'b'}, false}};
    for (const auto& u : utf8) EXPECT(cp_utf8_ok(u.s.data(), (uint32_t)u.s.size()) == u.ok);
    // the fold
    uint8_t status[4] = {CP_ACCEPTED, CP_MALFORMED, CP_ACCEPTED, CP_ACCEPTED};
    const uint8_t ok[5] = {1, 1, 1, 0, 1};
    const uint64_t env0[5] = {0, 2, 2, 2, 5};
    emul_comp_fold(status, ok, env0, 4);
    EXPECT(status[0] == CP_ACCEPTED && status[1] == CP_MALFORMED && status[2] == CP_ACCEPTED && status[3] == CP_REJECTED);
    if (failures) { std::fprintf(stderr, "emul_composites: %d failure(s)\n", failures); return 1; }
    std::printf("emul_composites ok\n");
    return 0;
}
