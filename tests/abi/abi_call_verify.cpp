// Calls the entry points of include/libzkp_hip_verify.h (the mixed verifier) from C++ through the headers alone: a mixed batch is proved
// with zkp_hip_process_batch and its packed output goes straight back into zkp_hip_verify_envelopes, then -- still in device memory -- into
// zkp_hip_verify_envelopes_device.  Built by __graft_entry__.build() (host compile + link against libzkp_hip.so, no GPU needed), run on the
// GPU box by tests/test_gpu_abi_verify.py.  Prints "abi_call_verify ok: N symbols" and exits 0 when every call behaved.
#include "../../include/libzkp_hip_verify.h"
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
    // an absurd size is an argument error before anything is read or a device is looked for
    CHECK(zkp_hip_verify_envelopes((1ull << 22) + 1, nullptr, nullptr, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    CHECK(zkp_hip_verify_envelopes_device((1ull << 22) + 1, nullptr, nullptr, nullptr, nullptr) == ZKP_HIP_E_ARGUMENT);
    CHECK(zkp_hip_verify_envelopes(0, nullptr, nullptr, nullptr, nullptr) == 0 && zkp_hip_verify_envelopes_device(0, nullptr, nullptr, nullptr, nullptr) == 0);
    if (zkp_hip_init(0) != 0) { std::fprintf(stderr, "abi_call_verify: %s\n", zkp_hip_last_error()); return 2; }
    const auto pk_eq = slurp(gold + "/equality_mimc_pk.bin"), pk_mem = slurp(gold + "/membership_mimc_pk.bin");
    CHECK(!pk_eq.empty() && !pk_mem.empty());

    // one op of every kind, twice, interleaved
    const uint64_t n = 12;
    std::vector<uint64_t> lists = {10, 20, 30, /* set */ 7, 8, 9, 11, /* consistency */ 1, 5, 5, 9};
    std::vector<zkp_hip_op> ops(n);
    for (uint64_t i = 0; i < n; i++) {
        zkp_hip_op o{}; o.kind = (uint32_t)(1 + i % 6);
        switch (o.kind) {
            case ZKP_HIP_OP_RANGE: o.a = 40 + i; o.b = 10; o.c = 100; break;
            case ZKP_HIP_OP_EQUALITY: o.a = o.b = 1000 + i; break;
            case ZKP_HIP_OP_THRESHOLD: o.a = 55; o.count = 3; o.list_off = 0; break;
            case ZKP_HIP_OP_MEMBERSHIP: o.a = 9; o.count = 4; o.list_off = 3; break;
            case ZKP_HIP_OP_IMPROVEMENT: o.a = 5 + i; o.b = 500 + i; break;
            default: o.count = 4; o.list_off = 7; break;
        }
        ops[i] = o;
    }
    std::vector<uint8_t> seeds(32 * n); for (size_t i = 0; i < seeds.size(); i++) seeds[i] = (uint8_t)(i * 11 + 3);
    uint64_t cap = 0;
    CHECK(zkp_hip_process_batch_bytes(n, ops.data(), &cap) == 0 && cap > 0);
    std::vector<uint8_t> out(cap); std::vector<uint64_t> off(n + 1); std::vector<int32_t> status(n);

    // no key yet: an equality envelope that reaches its verifier fails the call as zkp_hip_verify_equality_batch does
    {
        std::vector<uint8_t> eq(298, 0); eq[0] = 2; eq[1] = 2; eq[3] = 1; eq[6] = 32;          // payload 256, commitment 32
        const uint64_t o2[2] = {0, 298}; uint8_t ok1 = 9;
        CHECK(zkp_hip_verify_envelopes(1, eq.data(), o2, nullptr, &ok1) == ZKP_HIP_E_ARGUMENT && std::strstr(zkp_hip_last_error(), "no (usable) key loaded"));
        uint32_t len = 298;
        CHECK(zkp_hip_verify_equality_batch(1, eq.data(), 298, &len, &ok1) == ZKP_HIP_E_ARGUMENT && std::strstr(zkp_hip_last_error(), "no (usable) key loaded"));
    }
    CHECK(zkp_hip_groth16_load_key(0, pk_eq.data(), pk_eq.size()) == 0 && zkp_hip_groth16_load_key(1, pk_mem.data(), pk_mem.size()) == 0);
    CHECK(zkp_hip_process_batch(n, ops.data(), lists.data(), seeds.data(), out.data(), cap, off.data(), status.data()) == 0);
    for (uint64_t i = 0; i < n; i++) CHECK(status[i] == 0 && out[off[i]] == 2 && out[off[i] + 1] == ops[i].kind);

    // ---- host buffers: what process_batch wrote goes straight back in
    std::vector<uint8_t> ok(n, 9), expect(n);
    CHECK(zkp_hip_verify_envelopes(n, out.data(), off.data(), nullptr, ok.data()) == 0); CALLED(zkp_hip_verify_envelopes);
    for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == 1);
    for (uint64_t i = 0; i < n; i++) expect[i] = (uint8_t)ops[i].kind;
    expect[0] = 0; expect[1] = 3; expect[2] = 9;                      // any | an equality envelope expected as a threshold one | no scheme at all
    CHECK(zkp_hip_verify_envelopes(n, out.data(), off.data(), expect.data(), ok.data()) == 0);
    for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == (i == 1 || i == 2 ? 0 : 1));
    {
        double ms = 0; uint64_t passes = 0, rows = 0;
        CHECK(zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_VERIFY_MIXED, &ms, &passes, &rows, 1) == 0 && passes == 12 && rows == 2 * n - 2 && ms > 0);
        CHECK(zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_VERIFY_MIXED + 1, &ms, &passes, &rows, 0) == ZKP_HIP_E_ARGUMENT);
    }
    std::vector<uint8_t> bad = out;
    bad[off[4] + 100] ^= 1; bad[off[7] + 60] ^= 1;
    CHECK(zkp_hip_verify_envelopes(n, bad.data(), off.data(), nullptr, ok.data()) == 0);
    for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == (i == 4 || i == 7 ? 0 : 1));
    // a slice of the list: offsets need not start at 0
    CHECK(zkp_hip_verify_envelopes(5, out.data(), off.data() + 3, nullptr, ok.data()) == 0);
    for (uint64_t i = 0; i < 5; i++) CHECK(ok[i] == 1);

    // ---- device pointers
    {
        uint8_t *d_blob = nullptr, *d_ok = nullptr, *d_expect = nullptr; uint64_t* d_off = nullptr;
        CHECK(hipMalloc((void**)&d_blob, off[n]) == hipSuccess); CHECK(hipMalloc((void**)&d_off, 8 * (n + 1)) == hipSuccess);
        CHECK(hipMalloc((void**)&d_ok, n) == hipSuccess); CHECK(hipMalloc((void**)&d_expect, n) == hipSuccess);
        (void)hipMemcpy(d_blob, bad.data(), off[n], hipMemcpyHostToDevice); (void)hipMemcpy(d_off, off.data(), 8 * (n + 1), hipMemcpyHostToDevice);
        (void)hipMemcpy(d_expect, expect.data(), n, hipMemcpyHostToDevice); (void)hipMemset(d_ok, 9, n);
        CHECK(zkp_hip_verify_envelopes_device(n, d_blob, d_off, nullptr, d_ok) == 0); CALLED(zkp_hip_verify_envelopes_device);
        (void)hipMemcpy(ok.data(), d_ok, n, hipMemcpyDeviceToHost);
        for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == (i == 4 || i == 7 ? 0 : 1));
        CHECK(zkp_hip_verify_envelopes_device(n, d_blob, d_off, d_expect, d_ok) == 0);
        (void)hipMemcpy(ok.data(), d_ok, n, hipMemcpyDeviceToHost);
        for (uint64_t i = 0; i < n; i++) CHECK(ok[i] == (i == 1 || i == 2 || i == 4 || i == 7 ? 0 : 1));
        (void)hipFree(d_blob); (void)hipFree(d_off); (void)hipFree(d_ok); (void)hipFree(d_expect);
    }
    zkp_hip_shutdown();
    if (failures) { std::fprintf(stderr, "abi_call_verify: %d failure(s)\n", failures); return 1; }
    std::printf("abi_call_verify ok: %zu symbols\n", called.size());
    return 0;
}
