// Calls the entry points of include/libzkp_hip_statements.h from C++ through the headers alone: a mixed batch is proved with
// zkp_hip_process_batch, and its ops and packed output go straight into zkp_stmt_verify, then -- still in device memory -- into
// zkp_stmt_verify_device; two ops are swapped and the two reasons checked.  Built by __graft_entry__.build() (host compile + link against
// libzkp_hip.so, no GPU needed), run on the GPU box by tests/test_gpu_abi_statements.py.  Prints "abi_call_statements ok: N symbols" and
// exits 0 when every call behaved.
#include "../../include/libzkp_hip_statements.h"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <set>
#include <string>
#include <vector>
#include <hip/hip_runtime_api.h>

static std::set<std::string> called;
static int failures = 0;
#define CALLED(name) called.insert(#name)
#define CHECK(cond)                                                                                   \
    do {                                                                                              \
        if (!(cond)) { std::fprintf(stderr, "FAIL %s:%d: %s   last_error=%s\n", __FILE__, __LINE__, #cond, zkp_hip_last_error()); failures++; } \
    } while (0)

static std::vector<uint8_t> slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
    const std::string gold = argc > 1 ? argv[1] : "tests/golden";
    // an absurd size is an argument error before anything is read or a device is looked for; n = 0 touches nothing
    CHECK(zkp_stmt_verify((1ull << 22) + 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    CHECK(zkp_stmt_verify_device((1ull << 22) + 1, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    CHECK(zkp_stmt_verify(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0 && zkp_stmt_verify_device(0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) == 0);
    if (zkp_hip_init(0) != 0) { std::fprintf(stderr, "abi_call_statements: %s\n", zkp_hip_last_error()); return 2; }
    const auto pk_eq = slurp(gold + "/equality_mimc_pk.bin"), pk_mem = slurp(gold + "/membership_mimc_pk.bin");
    CHECK(!pk_eq.empty() && !pk_mem.empty());
    CHECK(zkp_hip_groth16_load_key(0, pk_eq.data(), pk_eq.size()) == 0 && zkp_hip_groth16_load_key(1, pk_mem.data(), pk_mem.size()) == 0);

    // one op of every kind, twice, interleaved; the two ops of a kind state different things
    const uint64_t n = 12;
    std::vector<uint64_t> lists = {10, 20, 30, /* set */ 7, 8, 9, 11, /* consistency */ 1, 5, 5, 9, /* the second set */ 9, 7, 7};
    std::vector<zkp_hip_op> ops(n);
    for (uint64_t i = 0; i < n; i++) {
        zkp_hip_op o{}; o.kind = (uint32_t)(1 + i % 6);
        switch (o.kind) {
            case ZKP_HIP_OP_RANGE: o.a = 40 + i; o.b = 10 + i; o.c = 100; break;
            case ZKP_HIP_OP_EQUALITY: o.a = o.b = 1000 + i; break;
            case ZKP_HIP_OP_THRESHOLD: o.a = 50 + i; o.count = 3; o.list_off = 0; break;
            case ZKP_HIP_OP_MEMBERSHIP: o.a = 9; if (i < 6) { o.count = 4; o.list_off = 3; } else { o.count = 3; o.list_off = 11; } break;
            case ZKP_HIP_OP_IMPROVEMENT: o.a = 5 + i; o.b = 500 + i; break;
            default: o.count = 4; o.list_off = 7; break;
        }
        ops[i] = o;
    }
    std::vector<uint8_t> seeds(32 * n); for (size_t i = 0; i < seeds.size(); i++) seeds[i] = (uint8_t)(i * 11 + 3);
    uint64_t cap = 0;
    CHECK(zkp_hip_process_batch_bytes(n, ops.data(), &cap) == 0 && cap > 0);
    std::vector<uint8_t> out(cap); std::vector<uint64_t> off(n + 1); std::vector<int32_t> status(n);
    CHECK(zkp_hip_process_batch(n, ops.data(), lists.data(), seeds.data(), out.data(), cap, off.data(), status.data()) == 0);
    for (uint64_t i = 0; i < n; i++) CHECK(status[i] == 0);

    // ---- host buffers: the prover's ops and what it wrote go straight in
    std::vector<uint8_t> ok(n, 9), why(n, 9);
    CHECK(zkp_stmt_verify(n, ops.data(), lists.data(), lists.size(), out.data(), off.data(), ok.data(), why.data()) == 0); CALLED(zkp_stmt_verify);
    for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == 1 && why[i] == ZKP_STMT_ACCEPTED);
    CHECK(zkp_stmt_verify(n, ops.data(), lists.data(), lists.size(), out.data(), off.data(), ok.data(), nullptr) == 0);          // why may be NULL
    for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == 1);
    // two ops swapped: the two range ops (other bounds: the statement is not the envelope's), a range and an equality op (another scheme: the envelope)
    std::vector<zkp_hip_op> swapped = ops;
    std::swap(swapped[0], swapped[6]); std::swap(swapped[1], swapped[2]);
    CHECK(zkp_stmt_verify(n, swapped.data(), lists.data(), lists.size(), out.data(), off.data(), ok.data(), why.data()) == 0);
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t want = i == 0 || i == 6 ? ZKP_STMT_STATEMENT : i == 1 || i == 2 ? ZKP_STMT_ENVELOPE : ZKP_STMT_ACCEPTED;
        CHECK(why[i] == want && ok[i] == (want == ZKP_STMT_ACCEPTED));
    }
    // a flipped proof byte under the right statement
    std::vector<uint8_t> bad = out;
    bad[off[4] + 100] ^= 1;
    CHECK(zkp_stmt_verify(n, ops.data(), lists.data(), lists.size(), bad.data(), off.data(), ok.data(), why.data()) == 0);
    for (uint64_t i = 0; i < n; i++) CHECK(why[i] == (i == 4 ? ZKP_STMT_PROOF : ZKP_STMT_ACCEPTED) && ok[i] == (i != 4));
    {
        double ms = 0; uint64_t seen = 0, r_env = 0, r_stmt = 0, r_proof = 0;
        CHECK(zkp_stmt_counters(&ms, &seen, &r_env, &r_stmt, &r_proof, 1) == 0); CALLED(zkp_stmt_counters);
        CHECK(seen == 4 * n && r_env == 2 && r_stmt == 2 && r_proof == 1 && ms > 0);
        CHECK(zkp_stmt_counters(&ms, &seen, nullptr, nullptr, nullptr, 0) == 0 && seen == 0 && ms == 0);
    }

    // ---- device pointers
    {
        uint8_t *d_blob = nullptr, *d_ok = nullptr, *d_why = nullptr; uint64_t *d_off = nullptr, *d_lists = nullptr; zkp_hip_op* d_ops = nullptr;
        CHECK(hipMalloc((void**)&d_blob, off[n]) == hipSuccess); CHECK(hipMalloc((void**)&d_off, 8 * (n + 1)) == hipSuccess);
        CHECK(hipMalloc((void**)&d_ok, n) == hipSuccess); CHECK(hipMalloc((void**)&d_why, n) == hipSuccess);
        CHECK(hipMalloc((void**)&d_lists, 8 * lists.size()) == hipSuccess); CHECK(hipMalloc((void**)&d_ops, sizeof(zkp_hip_op) * n) == hipSuccess);
        (void)hipMemcpy(d_blob, bad.data(), off[n], hipMemcpyHostToDevice); (void)hipMemcpy(d_off, off.data(), 8 * (n + 1), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_lists, lists.data(), 8 * lists.size(), hipMemcpyHostToDevice); (void)hipMemcpy(d_ops, swapped.data(), sizeof(zkp_hip_op) * n, hipMemcpyHostToDevice);
        (void)hipMemset(d_ok, 9, n); (void)hipMemset(d_why, 9, n);
        CHECK(zkp_stmt_verify_device(n, d_ops, d_lists, lists.size(), d_blob, d_off, d_ok, d_why) == 0); CALLED(zkp_stmt_verify_device);
        (void)hipMemcpy(ok.data(), d_ok, n, hipMemcpyDeviceToHost); (void)hipMemcpy(why.data(), d_why, n, hipMemcpyDeviceToHost);
        for (uint64_t i = 0; i < n; i++) {
            const uint8_t want = i == 0 || i == 6 ? ZKP_STMT_STATEMENT : i == 1 || i == 2 ? ZKP_STMT_ENVELOPE : i == 4 ? ZKP_STMT_PROOF : ZKP_STMT_ACCEPTED;
            CHECK(why[i] == want && ok[i] == (want == ZKP_STMT_ACCEPTED));
        }
        (void)hipMemset(d_ok, 9, n);
        CHECK(zkp_stmt_verify_device(n, d_ops, d_lists, lists.size(), d_blob, d_off, d_ok, nullptr) == 0);
        (void)hipMemcpy(ok.data(), d_ok, n, hipMemcpyDeviceToHost);
        for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == !(i == 0 || i == 6 || i == 1 || i == 2 || i == 4));
        (void)hipFree(d_blob); (void)hipFree(d_off); (void)hipFree(d_ok); (void)hipFree(d_why); (void)hipFree(d_lists); (void)hipFree(d_ops);
    }
    zkp_hip_shutdown();
    if (failures) { std::fprintf(stderr, "abi_call_statements: %d failure(s)\n", failures); return 1; }
    std::printf("abi_call_statements ok: %zu symbols\n", called.size());
    return 0;
}
