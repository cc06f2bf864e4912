// Calls the entry points of include/libzkp_hip_seal.h from C++ through the headers alone: fake envelopes are sealed from host buffers, a
// batch of range proofs is staged, proved and sealed where it lies, the same proofs are fetched and sealed from host buffers, and both
// must be the same bytes, which zkp_hip_verify_composites then accepts.  Built by __graft_entry__.build() (host compile + link against
// libzkp_hip.so, no GPU needed), run on the GPU box by tests/test_gpu_composites_seal.py.  Prints "abi_call_seal ok: N symbols" and exits 0
// when every call behaved.
#include "../../include/libzkp_hip_seal.h"
#include "../../include/libzkp_hip_composites.h"
#include <cstdio>
#include <cstring>
#include <set>
#include <string>
#include <vector>

static std::set<std::string> called;
static int failures = 0;
#define CALLED(name) called.insert(#name)
#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s   last_error=%s\n", __FILE__, __LINE__, #cond, zkp_hip_last_error()); failures++; } \
    } while (0)

int main() {
    // an absurd size is an argument error before anything is read or a device is looked for; n = 0 touches nothing
    CHECK(libzkp_seal_composites((1ull << 22) + 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    CHECK(libzkp_seal_composites(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0);
    CHECK(libzkp_seal_batch(nullptr, 0, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == 0);
    CHECK(libzkp_seal_batch(nullptr, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    if (zkp_hip_init(0) != 0) { std::fprintf(stderr, "abi_call_seal: %s\n", zkp_hip_last_error()); return 2; }

    // ---- host buffers: three fake envelopes (scheme 9) in two containers, an empty third one
    {
        std::vector<uint8_t> env; std::vector<uint64_t> env_off = {0};
        for (uint32_t len : {10u, 47u, 13u}) {
            env.push_back(2); env.push_back(9);
            for (int b = 0; b < 4; b++) env.push_back((uint8_t)((len - 10) >> (8 * b)));
            for (int b = 0; b < 4; b++) env.push_back(0);
            for (uint32_t k = 10; k < len; k++) env.push_back((uint8_t)(k + len));
            env_off.push_back(env.size());
        }
        const uint64_t first[4] = {0, 2, 3, 3};
        const uint8_t meta[] = {1, 0, 0, 0, 'k', 2, 0, 0, 0, 'v', 'w'};
        const uint64_t meta_off[4] = {0, 0, 11, 11};
        uint64_t out_off[4] = {9, 9, 9, 9}; uint8_t status[3] = {9, 9, 9};
        CHECK(libzkp_seal_composites(3, env.data(), env_off.data(), 3, first, meta, meta_off, nullptr, 0, out_off, status) == ZKP_HIP_E_ARGUMENT);      // the size needed
        const uint64_t need = out_off[3];
        CHECK(need == (12 + 4 + 10 + 4 + 47 + 32) + (12 + 4 + 13 + 11 + 32));
        std::vector<uint8_t> out(need + 1, 0xA5);
        CHECK(libzkp_seal_composites(3, env.data(), env_off.data(), 3, first, meta, meta_off, out.data(), need, out_off, status) == 1); CALLED(libzkp_seal_composites);
        CHECK(status[0] == LIBZKP_SEAL_SEALED && status[1] == LIBZKP_SEAL_SEALED && status[2] == LIBZKP_SEAL_REFUSED && out_off[2] == out_off[3] && out[need] == 0xA5);
        CHECK(memcmp(out.data(), "COMP\2\0\0\0\0\0\0\0\12\0\0\0", 16) == 0 && memcmp(out.data() + out_off[1], "COMP\1\0\0\0\1\0\0\0\15\0\0\0", 16) == 0);
        uint8_t verdict[2] = {9, 9};
        CHECK(zkp_hip_verify_composites(2, out.data(), out_off, ZKP_HIP_COMPOSITES_INTEGRITY_ONLY, verdict) == 0 && verdict[0] == 1 && verdict[1] == 1);
        double ms = 0; uint64_t containers = 0, sealed = 0, envelopes = 0, bytes = 0;
        CHECK(libzkp_seal_counters(&ms, &containers, &sealed, &envelopes, &bytes, 1) == 0); CALLED(libzkp_seal_counters);
        CHECK(containers == 3 && sealed == 2 && envelopes == 3 && bytes == need && ms > 0);
        CHECK(libzkp_seal_counters(nullptr, &containers, nullptr, nullptr, nullptr, 0) == 0 && containers == 0);
    }
    // ---- a staged batch of five range proofs in containers of 2 and 3, against the host-buffer form on the fetched proofs
    {
        const uint64_t n = 5;
        std::vector<zkp_hip_op> ops(n);
        for (uint64_t i = 0; i < n; i++) { zkp_hip_op o{}; o.kind = ZKP_HIP_OP_RANGE; o.a = 40 + i; o.b = 10; o.c = 1000 + i; ops[i] = o; }
        std::vector<uint8_t> seeds(32 * n); for (size_t i = 0; i < seeds.size(); i++) seeds[i] = (uint8_t)(i * 7 + 1);
        zkp_hip_batch* batch = nullptr;
        CHECK(zkp_hip_batch_stage(n, ops.data(), nullptr, seeds.data(), &batch) == 0 && batch);
        CHECK(zkp_hip_batch_prove_async(batch) == 0);
        const uint64_t first_op[3] = {0, 2, 5};
        const uint8_t meta[] = {2, 0, 0, 0, 'i', 'd', 1, 0, 0, 0, 7};
        const uint64_t meta_off[3] = {0, 11, 11};
        const uint64_t cap = zkp_hip_batch_max_bytes(batch) + 4 * n + 2 * 44 + sizeof meta;
        std::vector<uint8_t> sealed(cap), again(cap), proofs(zkp_hip_batch_max_bytes(batch));
        uint64_t off_a[3], off_b[3], poff[6]; uint8_t st_a[2], st_b[2]; int32_t pst[5];
        CHECK(libzkp_seal_batch(batch, 2, first_op, meta, meta_off, sealed.data(), cap, off_a, st_a) == 0); CALLED(libzkp_seal_batch);
        CHECK(st_a[0] == LIBZKP_SEAL_SEALED && st_a[1] == LIBZKP_SEAL_SEALED);
        CHECK(zkp_hip_batch_fetch(batch, proofs.data(), proofs.size(), poff, pst) == 0);          // the batch is still whole
        CHECK(libzkp_seal_composites(2, proofs.data(), poff, n, first_op, meta, meta_off, again.data(), cap, off_b, st_b) == 0);
        CHECK(memcmp(off_a, off_b, sizeof off_a) == 0 && memcmp(sealed.data(), again.data(), off_a[2]) == 0 && off_a[2] == poff[5] + 4 * n + 2 * 44 + sizeof meta);
        uint8_t verdict[2] = {9, 9};
        CHECK(zkp_hip_verify_composites(2, sealed.data(), off_a, 0, verdict) == 0 && verdict[0] == 1 && verdict[1] == 1);
        zkp_hip_batch_free(batch);
    }
    zkp_hip_shutdown();
    if (failures) { std::fprintf(stderr, "abi_call_seal: %d failure(s)\n", failures); return 1; }
    std::printf("abi_call_seal ok: %zu symbols\n", called.size());
    return 0;
}
