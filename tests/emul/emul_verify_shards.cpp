// TEST INFRASTRUCTURE: host build of the plan that cuts one verify call over the registered shards (verify_shards.h): weights and their
// prefix sums, slice count, slice boundaries, participating shards.  Loaded by tests/test_emul_verify_shards.py as a shared library; as a
// program of its own (it has a main) it walks a grid of cases and checks the plan's properties, which is the form to build with
// -fsanitize=address,undefined.
#include <cstdio>
#include <vector>
#include "../../libzkp_amd/csrc/verify_shards.h"
using namespace zkp;

extern "C" {
uint32_t emul_vs_max_shards(void) { return VS_MAX_SHARDS; }
// uniform weights: n envelopes of `unit` jobs; bounds has shards + 1 (at most 65) entries; returns the slice count
uint32_t emul_vs_plan_uniform(uint64_t n, uint32_t unit, uint32_t shards, uint64_t min_jobs, uint64_t* bounds) { return vs_plan(n, nullptr, unit, shards, min_jobs, bounds); }
// per-envelope weights (consistency: job counts, zero counted as one); prefix_out (n + 1 entries) receives the sums the plan used
uint32_t emul_vs_plan_weighted(uint64_t n, const uint32_t* weights, uint32_t shards, uint64_t min_jobs, uint64_t* bounds, uint64_t* prefix_out) {
    vs_prefix(n, weights, prefix_out);
    return vs_plan(n, prefix_out, 0, shards, min_jobs, bounds);
}
uint32_t emul_vs_participants(uint32_t caller, uint32_t shards, const uint8_t* holds, uint32_t* out) { return vs_participants(caller, shards, holds, out); }
// the fan-out data of a list call: prefix (n + 1), holds (shards), out = {unit, min_jobs}; has_key is [shards][2] (equality, membership)
void emul_vs_list_fanout(uint64_t n, const uint32_t* weights, int need_eq, int need_mem, uint32_t shards, const uint8_t* has_key, uint64_t bp_min, uint64_t g16_min,
                         uint64_t* prefix, uint8_t* holds, uint64_t* out) {
    uint32_t unit = 99; uint64_t min_jobs = 0;
    vs_list_fanout(n, weights, need_eq != 0, need_mem != 0, shards, has_key, bp_min, g16_min, prefix, holds, &unit, &min_jobs);
    out[0] = unit; out[1] = min_jobs;
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)

// the properties every plan has; weight(i) = prefix[i + 1] - prefix[i] or unit
void check_plan(uint64_t n, const std::vector<uint64_t>* prefix, uint32_t unit, uint32_t shards, uint64_t min_jobs) {
    uint64_t bounds[VS_MAX_SHARDS + 1];
    const uint32_t count = vs_plan(n, prefix ? prefix->data() : nullptr, unit, shards, min_jobs, bounds);
    if (n == 0) { EXPECT(count == 0); return; }
    auto before = [&](uint64_t i) { return prefix ? (*prefix)[i] : (uint64_t)unit * i; };
    const uint64_t total = before(n), m = min_jobs ? min_jobs : 1;
    EXPECT(count >= 1 && count <= shards && count <= VS_MAX_SHARDS && count <= (total / m ? total / m : 1));
    EXPECT(bounds[0] == 0 && bounds[count] == n);
    uint64_t wmax = 0;
    if (prefix) for (uint64_t i = 0; i < n; i++) wmax = before(i + 1) - before(i) > wmax ? before(i + 1) - before(i) : wmax;
    for (uint32_t s = 0; s < count; s++) {
        EXPECT(bounds[s] < bounds[s + 1]);
        const uint64_t w = before(bounds[s + 1]) - before(bounds[s]);
        if (count > 1) EXPECT(w >= m);
        if (!prefix) { const uint64_t len = bounds[s + 1] - bounds[s]; EXPECT(len == n / count || len == (n + count - 1) / count); }
        else { const uint64_t lo = total / count, hi = (total + count - 1) / count; EXPECT(w + wmax > lo && w < hi + wmax); }
    }
    if (total < 2 * m) EXPECT(count == 1);
}
}  // namespace

int main() {
    const uint64_t sizes[] = {0, 1, 2, 3, 12, 13, 64, 65, 1000, 4095, 4096, 8191, 8192, 8193, 16384, 65536, 0xffffffffull};
    const uint32_t shard_counts[] = {1, 2, 3, 8, 64};
    const uint64_t mins[] = {1, 3, 4, 7, 4096, 8193};
    for (uint64_t n : sizes) for (uint32_t S : shard_counts) for (uint64_t mj : mins) for (uint32_t unit : {1u, 2u}) check_plan(n, nullptr, unit, S, mj);
    uint64_t seed = 88172645463325252ull;
    auto next = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (uint64_t n : {1ull, 2ull, 13ull, 100ull, 5000ull, 70000ull}) for (int shape = 0; shape < 4; shape++) {
        std::vector<uint32_t> w(n);
        for (uint64_t i = 0; i < n; i++) w[i] = shape == 0 ? 0u : shape == 1 ? (uint32_t)(next() % 5) : shape == 2 ? (i == n / 2 ? 100000u : 1u) : (uint32_t)(next() % 1000);
        std::vector<uint64_t> prefix(n + 1);
        vs_prefix(n, w.data(), prefix.data());
        for (uint32_t S : shard_counts) for (uint64_t mj : mins) check_plan(n, &prefix, 0, S, mj);
    }
    uint32_t out[VS_MAX_SHARDS];
    const uint8_t holds[4] = {1, 0, 1, 1};
    EXPECT(vs_participants(0, 4, holds, out) == 3 && out[0] == 0 && out[1] == 2 && out[2] == 3);
    EXPECT(vs_participants(2, 4, holds, out) == 3 && out[0] == 2 && out[1] == 3 && out[2] == 0);
    EXPECT(vs_participants(1, 4, holds, out) == 0 && vs_participants(4, 4, holds, out) == 0);
    EXPECT(vs_participants(0, 2, nullptr, out) == 2 && out[0] == 0 && out[1] == 1);
    // the list calls' fan-out data: every combination of needed keys against four shards that hold both, equality only, membership only, none
    const uint8_t has_key[8] = {1, 1, 1, 0, 0, 1, 0, 0};
    const uint32_t lw[5] = {2, 0, 1, 4, 1};
    for (int need = 0; need < 4; need++) for (uint64_t a : {4096ull, 8193ull}) for (uint64_t b : {4096ull, 8193ull}) {
        uint64_t prefix[6], want[6], min_jobs = 0; uint8_t lh[4] = {9, 9, 9, 9}; uint32_t unit = 9;
        vs_list_fanout(5, lw, (need & 1) != 0, (need & 2) != 0, 4, has_key, a, b, prefix, lh, &unit, &min_jobs);
        vs_prefix(5, lw, want);
        for (int i = 0; i < 6; i++) EXPECT(prefix[i] == want[i]);
        EXPECT(prefix[5] == 9 && unit == 0 && min_jobs == (a > b ? a : b));
        for (int s = 0; s < 4; s++) EXPECT(lh[s] == (((need & 1) == 0 || has_key[2 * s]) && ((need & 2) == 0 || has_key[2 * s + 1]) ? 1 : 0));
    }
    if (failures) { std::fprintf(stderr, "emul_verify_shards: %d failure(s)\n", failures); return 1; }
    std::printf("emul_verify_shards ok\n");
    return 0;
}
