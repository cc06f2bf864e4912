// TEST INFRASTRUCTURE: host build of the sealing call's plan and steps (composite_seal.h): seal_plan, the frame step with the lanes of a wave
// as a loop, the digest lane.  emul_seal is what libzkp_seal_composites does with the kernels replaced by loops.  Loaded by
// tests/test_emul_composites_seal.py as a shared library; as a program of its own (it has a main) it seals the same families from
// allocations of exactly the blobs' sizes, which is the form to build with -fsanitize=address,undefined: a read outside a blob or a write
// outside the output is then an error, not a value.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "../../libzkp_amd/csrc/composite_seal.h"
using namespace zkp;

extern "C" {
uint32_t emul_seal_piece_bytes(void) { return (uint32_t)sizeof(SealPiece); }
// libzkp_seal_composites on the host.  env_code: null (the envelopes are judged from their lengths and header bytes), or one code per
// envelope as libzkp_seal_batch derives them from the ops' statuses (1 accepted, 2 failed op).  Returns 0, 1 (some container not sealed)
// or -3 (an argument error: out_cap too small -- out_off[n] then holds the size needed and nothing is written --, or a bad `first`).
int emul_seal(uint64_t n, const uint8_t* env_blob, const uint64_t* env_off, uint64_t n_env, const uint8_t* env_code, const uint64_t* first, const uint8_t* meta_blob,
              const uint64_t* meta_off, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* status) {
    if (n == 0) return 0;
    if (n > SEAL_MAX_ITEMS || n_env > SEAL_MAX_ITEMS || first[n] > n_env) return -3;
    for (uint64_t i = 0; i < n; i++) if (first[i] > first[i + 1]) return -3;
    const uint64_t env_lo = n_env ? env_off[0] : 0, env_hi = n_env ? env_off[n_env] : 0;
    std::vector<uint8_t> judged(n_env);
    if (!env_code) {
        for (uint64_t e = 0; e < n_env; e++) judged[e] = seal_env_code(env_blob, env_off[e], env_off[e + 1], env_lo, env_hi);
        env_code = judged.data();
    }
    SealPlan P;
    seal_plan(n, env_off, env_code, first, meta_blob, meta_off, P);
    memcpy(out_off, P.out_off.data(), 8 * (n + 1)); memcpy(status, P.status.data(), n);
    if (P.out_off[n] > out_cap) return -3;
    std::vector<SealPiece> pieces; std::vector<CompLane> lanes;
    seal_pieces(P, env_off, pieces, lanes);
    const uint64_t meta_lo = meta_off ? meta_off[0] : 0, meta_hi = meta_off ? meta_off[n] : 0;
    for (const SealPiece& S : pieces) for (uint32_t lane = 0; lane < 64; lane++)
        step_seal_frame(out, S, env_blob, env_blob + env_lo, env_blob + env_hi, meta_blob, meta_blob + meta_lo, meta_blob + meta_hi, lane, 64);
    for (const CompLane& L : lanes) step_seal_digest(out, out, out + P.out_off[n], L, P.order.data());
    return P.rec.size() != n ? 1 : 0;
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

typedef std::vector<uint8_t> Bytes;
void put32(Bytes& v, uint32_t x) { for (int b = 0; b < 4; b++) v.push_back((uint8_t)(x >> (8 * b))); }
void append(Bytes& v, const Bytes& w) { v.insert(v.end(), w.begin(), w.end()); }
// a format-valid envelope of n >= 10 bytes (scheme 9): no commitment, n - 10 payload bytes
Bytes proof(uint32_t n, uint32_t salt = 0) {
    Bytes p = {2, 9};
    put32(p, n - 10); put32(p, 0);
    for (uint32_t k = 10; k < n; k++) p.push_back((uint8_t)(k * 37 + salt + n));
    return p;
}
struct Meta { std::string key; Bytes value; };
Bytes entry(const Meta& m) { Bytes e; put32(e, (uint32_t)m.key.size()); e.insert(e.end(), m.key.begin(), m.key.end()); put32(e, (uint32_t)m.value.size()); append(e, m.value); return e; }
// the container from first principles: the framing written out, the digest by sha256_bytes over a flat copy of the hashed stream with the
// metadata entries in `hash_order`
Bytes container(const std::vector<Bytes>& proofs, const std::vector<Meta>& meta, const std::vector<uint32_t>& hash_order) {
    Bytes c = {'C', 'O', 'M', 'P'}, flat;
    const char* tag = "COMPOSITE_PROOF:";
    flat.assign(tag, tag + 16);
    put32(c, (uint32_t)proofs.size()); put32(c, (uint32_t)meta.size()); put32(flat, (uint32_t)proofs.size());
    for (const Bytes& p : proofs) { put32(c, (uint32_t)p.size()); append(c, p); append(flat, p); }
    for (const Meta& m : meta) append(c, entry(m));
    for (uint32_t k : hash_order) append(flat, entry(meta[k]));
    uint8_t d[32];
    sha256_bytes(d, flat.data(), flat.size());
    c.insert(c.end(), d, d + 32);
    return c;
}
std::vector<uint32_t> iota(size_t n) { std::vector<uint32_t> v(n); for (size_t k = 0; k < n; k++) v[k] = (uint32_t)k; return v; }

// One call: containers as (proofs, metadata run in wire form), behind `stray` bytes of another envelope so that the sources lie at every
// alignment.  Every blob is an allocation of exactly its size; the output is prefilled with 0xA5 and carries `guard` bytes on both sides.
struct Call {
    std::vector<std::vector<Bytes>> proofs; std::vector<Bytes> metas;
    std::vector<uint8_t> status; std::vector<uint64_t> off; Bytes out; int rc = 0;
    uint64_t lead = 0;
    void run(uint32_t stray, uint64_t lead_bytes, bool with_meta = true, int64_t cap = -1) {
        const uint64_t n = proofs.size();
        Bytes env(stray, 0xEE), meta; std::vector<uint64_t> env_off = {0}, first = {1}, meta_off = {0};
        env_off.push_back(stray);
        for (uint64_t i = 0; i < n; i++) {
            for (const Bytes& p : proofs[i]) { append(env, p); env_off.push_back(env.size()); }
            first.push_back(env_off.size() - 1);
            if (with_meta) { append(meta, metas[i]); meta_off.push_back(meta.size()); }
        }
        uint8_t* e = new uint8_t[env.size() ? env.size() : 1]; if (!env.empty()) memcpy(e, env.data(), env.size());
        uint8_t* m = new uint8_t[meta.size() ? meta.size() : 1]; if (!meta.empty()) memcpy(m, meta.data(), meta.size());
        status.assign(n, 9); off.assign(n + 1, 0); lead = lead_bytes;
        // the size needed: a first call with no room
        rc = emul_seal(n, e, env_off.data(), env_off.size() - 1, nullptr, first.data(), with_meta ? m : nullptr, with_meta ? meta_off.data() : nullptr, nullptr, 0, off.data(), status.data());
        const uint64_t need = off[n];
        EXPECT(need == 0 ? rc >= 0 : rc == -3);
        const uint64_t room = cap < 0 ? need : (uint64_t)cap;
        uint8_t* o = new uint8_t[lead + room + 1];
        memset(o, 0xA5, lead + room + 1);
        rc = emul_seal(n, e, env_off.data(), env_off.size() - 1, nullptr, first.data(), with_meta ? m : nullptr, with_meta ? meta_off.data() : nullptr, o + lead, room, off.data(), status.data());
        out.assign(o, o + lead + room + 1);
        delete[] e; delete[] m; delete[] o;
    }
    Bytes sealed(uint64_t i) const { return Bytes(out.begin() + lead + off[i], out.begin() + lead + off[i + 1]); }
    bool guards_intact() const {
        for (uint64_t k = 0; k < lead; k++) if (out[k] != 0xA5) return false;
        for (uint64_t k = lead + off.back(); k < out.size(); k++) if (out[k] != 0xA5) return false;
        return true;
    }
};
Bytes wire(const std::vector<Meta>& meta) { Bytes w; for (const Meta& m : meta) append(w, entry(m)); return w; }
}  // namespace

int main() {
    // ---- proofs of 10..13 bytes behind 0..7 stray bytes, destinations at 0..3 bytes past a dword: pieces begin at every source and destination alignment
    for (uint32_t stray = 0; stray < 8; stray++) for (uint32_t lead = 0; lead < 4; lead++) {
        Call K;
        std::vector<std::vector<Bytes>> want_p; std::vector<std::vector<Meta>> want_m;
        for (uint32_t a = 10; a <= 13; a++) for (uint32_t b = 10; b <= 13; b++) for (uint32_t c = 10; c <= 13; c += 3) {
            std::vector<Bytes> p = {proof(a, stray), proof(b, 1), proof(c, 2), proof(10, 3), proof(13, 4), proof(11, 5), proof(12, 6)};
            std::vector<Meta> m = {{std::string(stray % 3, 'k'), Bytes(stray, 'v')}};
            K.proofs.push_back(p); K.metas.push_back(wire(m)); want_p.push_back(p); want_m.push_back(m);
        }
        K.run(stray, lead);
        EXPECT(K.rc == 0 && K.guards_intact());
        for (size_t i = 0; i < want_p.size(); i++) { EXPECT(K.status[i] == SEAL_SEALED); EXPECT(K.sealed(i) == container(want_p[i], want_m[i], {0})); }
    }
    // ---- hashed lengths of every residue mod 64, steered by one value of 0..130 bytes; the same from a proof alone, without a metadata array
    {
        Call K, Q;
        for (uint32_t vl = 0; vl <= 130; vl++) {
            K.proofs.push_back({proof(10)}); K.metas.push_back(wire({{"v", Bytes(vl, (uint8_t)vl)}}));
            Q.proofs.push_back({proof(10 + vl, vl)});
        }
        K.run(3, 1); Q.run(5, 2, false);
        EXPECT(K.rc == 0 && Q.rc == 0 && K.guards_intact() && Q.guards_intact());
        for (uint32_t vl = 0; vl <= 130; vl++) {
            EXPECT(K.sealed(vl) == container({proof(10)}, {{"v", Bytes(vl, (uint8_t)vl)}}, {0}));
            EXPECT(Q.sealed(vl) == container({proof(10 + vl, vl)}, {}, {}));
        }
    }
    // ---- every order of three keys, one a prefix of another: the bytes keep the caller's order, the digest takes the sorted one
    {
        const std::vector<Meta> base = {{"ab", {1}}, {"a", {2, 2}}, {"b", {}}};          // hash order: a, ab, b
        const uint32_t perms[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
        Call K;
        for (const auto& pm : perms) { K.proofs.push_back({proof(40), proof(11)}); K.metas.push_back(wire({base[pm[0]], base[pm[1]], base[pm[2]]})); }
        K.run(1, 3);
        EXPECT(K.rc == 0);
        for (int k = 0; k < 6; k++) {
            const std::vector<Meta> m = {base[perms[k][0]], base[perms[k][1]], base[perms[k][2]]};
            std::vector<uint32_t> order(3);
            for (uint32_t j = 0; j < 3; j++) { if (m[j].key == "a") order[0] = j; else if (m[j].key == "ab") order[1] = j; else order[2] = j; }
            EXPECT(K.sealed(k) == container({proof(40), proof(11)}, m, order));
        }
    }
    // ---- the refusals, on both sides of each limit, between sealed neighbours
    {
        Call K;
        auto add = [&](std::vector<Bytes> p, Bytes m) { K.proofs.push_back(p); K.metas.push_back(m); };
        const Bytes good = proof(47, 3);
        Bytes mismatch = proof(20); mismatch.push_back(0);
        Bytes payload = {2, 9}; put32(payload, 900 * 1024 + 1); put32(payload, 0); payload.resize(10 + 900 * 1024 + 1);
        Bytes payload_at = {2, 9}; put32(payload_at, 900 * 1024); put32(payload_at, 0); payload_at.resize(10 + 900 * 1024);
        Bytes commitment = {2, 9}; put32(commitment, 5); put32(commitment, 257); commitment.resize(10 + 262);
        Bytes commitment_at = {2, 9}; put32(commitment_at, 5); put32(commitment_at, 256); commitment_at.resize(10 + 261);
        std::vector<Bytes> p1000, p1001; std::vector<Meta> m1000;
        for (uint32_t k = 0; k < 1001; k++) { if (k < 1000) p1000.push_back(proof(10 + k % 4, k)); p1001.push_back(proof(10, k)); }
        for (uint32_t k = 0; k < 1000; k++) m1000.push_back({"key" + std::to_string(1999 - k), Bytes(k % 5, 7)});
        std::vector<Meta> m1001 = m1000; m1001.push_back({"one more", {}});
        Bytes truncated = wire({{"kk", Bytes(50, 1)}}); truncated.pop_back();
        Bytes left_over = wire({{"kk", {1}}}); left_over.push_back(0);
        const uint8_t want[] = {1, 2, 2, 2, 2, 1, 2, 1, 1, 3, 1, 3, 1, 3, 1, 3, 3, 3, 3, 3, 1};
        add({good}, {});                                             // 0 sealed
        add({}, {});                                                 // 1 an empty list
        add({good, Bytes(9, 2)}, {});                                // 2 an envelope of 9 bytes
        add({mismatch}, {});                                         // 3 a length that is not 10 + payload + commitment
        add({payload}, {});                                          // 4 payload of 900 KiB + 1
        add({payload_at}, {});                                       // 5 ... of 900 KiB
        add({commitment, good}, {});                                 // 6 commitment of 257 bytes
        add({commitment_at}, {});                                    // 7 ... of 256
        add(p1000, {});                                              // 8 1000 proofs
        add(p1001, {});                                              // 9 1001
        add({good}, wire(m1000));                                    // 10 1000 metadata entries
        add({good}, wire(m1001));                                    // 11 1001
        add({good}, wire({{std::string(1024, 'k'), {1}}}));          // 12 a key of 1024 bytes
        add({good}, wire({{std::string(1025, 'k'), {1}}}));          // 13 1025
        add({good}, wire({{"k", Bytes(65536, 9)}}));                 // 14 a value of 65536 bytes
        add({good}, wire({{"k", Bytes(65537, 9)}}));                 // 15 65537
        add({good}, wire({{"\xed\xa0\x80", {1}}}));                  // 16 a surrogate in a key
        add({good}, wire({{"k", {1}}, {"j", {}}, {"k", {2}}}));      // 17 a key that occurs twice
        add({good}, truncated);                                      // 18 a truncated run
        add({good}, left_over);                                      // 19 bytes left over
        add({good, proof(10)}, wire({{"\xc3\xa9", {1}}, {"", {}}})); // 20 sealed: a two-byte character, an empty key
        K.run(2, 1);
        EXPECT(K.rc == 1 && K.guards_intact());
        for (size_t i = 0; i < K.proofs.size(); i++) { EXPECT(K.status[i] == want[i]); if (want[i] != 1) EXPECT(K.off[i] == K.off[i + 1]); }
        EXPECT(K.sealed(0) == container({good}, {}, {}) && K.sealed(5) == container({payload_at}, {}, {}) && K.sealed(7) == container({commitment_at}, {}, {}));
        EXPECT(K.sealed(8) == container(p1000, {}, {}));
        std::vector<uint32_t> rev = iota(1000); for (uint32_t k = 0; k < 1000; k++) rev[k] = 999 - k;          // keys were written descending
        EXPECT(K.sealed(10) == container({good}, m1000, rev));
        EXPECT(K.sealed(12) == container({good}, {{std::string(1024, 'k'), {1}}}, {0}) && K.sealed(14) == container({good}, {{"k", Bytes(65536, 9)}}, {0}));
        EXPECT(K.sealed(20) == container({good, proof(10)}, {{"\xc3\xa9", {1}}, {"", {}}}, {1, 0}));
        // a buffer one byte too small: ZKP_HIP_E_ARGUMENT's place, the size needed in out_off[n], nothing written
        const uint64_t need = K.off.back();
        K.run(2, 1, true, (int64_t)need - 1);
        EXPECT(K.rc == -3 && K.off.back() == need);
        for (uint8_t b : K.out) EXPECT(b == 0xA5);
    }
    // ---- String::from_utf8's corner cases as keys
    {
        const struct { std::string s; bool ok; } utf8[] = {
            {"", true}, {"k", true}, {"caf\xc3\xa9", true}, {"\xe2\x82\xac", true}, {"\xf0\x9f\x98\x80", true}, {"\xf4\x8f\xbf\xbf", true}, {"\xed\x9f\xbf", true}, {"\xee\x80\x80", true},
            {"\xc0\x80", false}, {"\xc1\xbf", false}, {"\xe0\x9f\xbf", false}, {"\xed\xa0\x80", false}, {"\xf0\x8f\xbf\xbf", false}, {"\xf4\x90\x80\x80", false},
            {"\xf5\x80\x80\x80", false}, {"\x80", false}, {"caf\xc3", false}, {"a\xe2\x82", false}, {"\xf0\x9f\x98", false}, {"\xff", false}};
        Call K;
        for (const auto& u : utf8) { K.proofs.push_back({proof(12)}); K.metas.push_back(wire({{"a", {1}}, {u.s, {5, 6}}, {"z", {2}}})); }
        K.run(0, 0);
        size_t i = 0;
        for (const auto& u : utf8) { EXPECT(K.status[i] == (u.ok ? SEAL_SEALED : SEAL_UNREADABLE)); i++; }
        EXPECT(K.sealed(0) == container({proof(12)}, {{"a", {1}}, {"", {5, 6}}, {"z", {2}}}, {1, 0, 2}));
    }
    // ---- exactly 4 MiB, and one byte more
    for (uint32_t more = 0; more < 2; more++) {
        Call K;
        std::vector<Bytes> p;
        for (uint32_t s = 0; s < 4; s++) p.push_back(proof(900000, s));
        p.push_back(proof((4u << 20) - 12 - 5 * 4 - 32 - 4 * 900000 - 500, 4));
        const std::vector<Meta> m = {{"k", Bytes(500 - 9 + more, 0)}};
        K.proofs.push_back(p); K.metas.push_back(wire(m));
        K.run(1, 1);
        EXPECT(K.guards_intact());
        if (more) EXPECT(K.rc == 1 && K.status[0] == SEAL_UNREADABLE && K.off[1] == 0);
        else EXPECT(K.rc == 0 && K.status[0] == SEAL_SEALED && K.off[1] == (4u << 20) && K.sealed(0) == container(p, m, {0}));
    }
    // ---- the batch form's codes: a failed op fails its container and nothing else
    {
        const Bytes a = proof(30), b = proof(31);
        Bytes env = a; append(env, b);
        const uint64_t env_off[4] = {0, 30, 30, 61}, first[4] = {0, 1, 2, 3};
        const uint8_t code[3] = {SEAL_ENV_ACCEPTED, SEAL_ENV_FAILED_OP, SEAL_ENV_ACCEPTED};
        uint8_t status[3]; uint64_t off[4]; Bytes out(200, 0xA5);
        const int rc = emul_seal(3, env.data(), env_off, 3, code, first, nullptr, nullptr, out.data(), out.size(), off, status);
        EXPECT(rc == 1 && status[0] == SEAL_SEALED && status[1] == SEAL_FAILED_OP && status[2] == SEAL_SEALED && off[1] == off[2]);
        EXPECT(Bytes(out.begin(), out.begin() + off[1]) == container({a}, {}, {}) && Bytes(out.begin() + off[2], out.begin() + off[3]) == container({b}, {}, {}));
    }
    if (failures) { std::fprintf(stderr, "emul_composites_seal: %d failure(s)\n", failures); return 1; }
    std::printf("emul_composites_seal ok\n");
    return 0;
}
