// TEST INFRASTRUCTURE: the key-blob reader of zkp_hip_groth16_load_key (libzkp_amd/csrc/g16_keyblob.h) on the CPU -- which of the two
// ark formats a blob is, the points of its verifying-key part, and the shape rules of a verifying key for the circuit it is offered
// for (instance count from the R1CS builders of g16_circuit.h).  Compiled by tests/test_emul_g16_keyblob.py itself; not part of the product.
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/g16_keyblob.h"
#include <cstdio>
using namespace zkp;

static uint32_t circuit_n_inst(int kind) { return (kind == G16_EQUALITY ? build_equality_r1cs() : build_membership_r1cs()).n_inst; }

extern "C" {
uint32_t emul_keyblob_n_inst(int kind) { return circuit_n_inst(kind); }
uint64_t emul_keyblob_vk_bytes(uint64_t n_ic) { return g16_vk_blob_bytes(n_ic); }

// What the loader makes of `blob` offered for circuit `kind`: -1 malformed prefix, 0 proving key (bytes remain behind gamma_abc_g1; the
// rest is not read here), 1 verifying key accepted, 2 verifying key refused -- `why` (cap bytes) then holds the loader's message.
// *n_ic = the count the blob states, *rest = bytes behind the prefix.
int emul_keyblob_classify(int kind, const uint8_t* blob, uint64_t len, uint32_t* n_ic, uint64_t* rest, char* why, uint32_t cap) {
    KeyReader R{blob, len};
    G16VkBlob B;
    if (cap) why[0] = 0;
    const int format = g16_read_key_prefix(R, B);
    if (format == G16_BLOB_MALFORMED) return -1;
    *n_ic = (uint32_t)B.abc.size(); *rest = R.left;
    if (format == G16_BLOB_PROVING_KEY) return 0;
    const char* msg = g16_check_verifying_key(B, circuit_n_inst(kind));
    if (!msg) return 1;
    snprintf(why, cap, "%s", msg);
    return 2;
}

// The parsed points as canonical little-endian words: alpha (16) | beta, gamma, delta (32 each: x.c0 x.c1 y.c0 y.c1) | gamma_abc_g1
// (16 each); inf[k] = 1 for point k at infinity (its words are left zero).  Returns the number of points, -1 if the prefix is malformed
// or `cap_words` is too small.
int emul_keyblob_points(const uint8_t* blob, uint64_t len, uint32_t* words, uint32_t cap_words, uint8_t* inf) {
    KeyReader R{blob, len};
    G16VkBlob B;
    if (g16_read_key_prefix(R, B) == G16_BLOB_MALFORMED) return -1;
    if (cap_words < 16 + 3 * 32 + 16 * B.abc.size()) return -1;
    memset(words, 0, 4ull * cap_words);
    uint32_t* w = words; int k = 0;
    auto put1 = [&](const G1Pt& p) { inf[k++] = p.inf; if (!p.inf) { fq_to_raw(w, p.p.x); fq_to_raw(w + 8, p.p.y); } w += 16; };
    auto put2 = [&](const G2Pt& p) { inf[k++] = p.inf; if (!p.inf) { fq_to_raw(w, p.p.x.c0); fq_to_raw(w + 8, p.p.x.c1); fq_to_raw(w + 16, p.p.y.c0); fq_to_raw(w + 24, p.p.y.c1); } w += 32; };
    put1(B.alpha_g1); put2(B.beta_g2); put2(B.gamma_g2); put2(B.delta_g2);
    for (const auto& e : B.abc) put1(e);
    return k;
}
}
