// How one zkp_hip_verify_*_batch call is cut over the registered shards: the planning, pure index arithmetic (no HIP calls, every sum in 64
// bits) shared by the host (zkp_hip.hip: verify_call and verify_fan_out, under the seven host-buffer verify entry points) and the host build of tests/emul/emul_verify_shards.cpp.
//
// A call of n envelopes is cut into contiguous slices, in order, one per participating shard; every slice goes through the scheme's own
// host-buffer verifier on its shard -- the same kernels, one set of launches per slice on that shard's stream.  EVERY SLICE DRAWS ITS OWN
// FRESH WEIGHTS AND MAKES ITS OWN BATCH CHECK: soundness is per slice (2^-128 per slice instead of per call), nothing is combined across GPUs.
//
// Weights, in the jobs the verifiers count: a range envelope 2, a threshold / equality / membership / improvement envelope 1 (`unit`, with
// prefix == nullptr), a consistency envelope the job count verify_bp_host reads from its k field, counted as at least 1 so that a zero-job
// envelope still costs something (vs_prefix).
// Slice count: min(shards, total / min_jobs, n), at least 1, lowered further until no slice is empty or lighter than min_jobs (an odd
// min_jobs under weight 2, or one very heavy envelope, can leave a light slice at the first count): min_jobs is the scheme's batch-check
// threshold in force, so every slice still takes the one-check path a whole batch of its size would have taken.  n == 0: no slice.
// Boundary s of `count` slices: the first envelope at which the running weight reaches s * total / count.  Uniform weights: slices of equal
// envelope counts +-1 (boundary = ceil(s * n / count)); otherwise no slice differs from the mean by the largest single weight or more.
#pragma once
#include "zkp_common.h"

namespace zkp {

constexpr uint32_t VS_MAX_SHARDS = 64;          // zkp_hip_init_devices registers at most 64 shards: bounds[] holds at most 65 entries

// ceil(s * total / count) without the product (s <= count <= 64, so s * (total % count) is small)
ZKP_HD inline uint64_t vs_target(uint64_t total, uint32_t count, uint32_t s) {
    const uint64_t q = total / count, r = total % count;
    return q * s + (r * s + count - 1) / count;
}
// prefix[i] = summed weights of the envelopes before i (n + 1 entries), every weight counted as at least 1; returns the total
ZKP_HD inline uint64_t vs_prefix(uint64_t n, const uint32_t* weights, uint64_t* prefix) {
    uint64_t t = 0;
    for (uint64_t i = 0; i < n; i++) { prefix[i] = t; t += weights[i] ? weights[i] : 1u; }
    prefix[n] = t;
    return t;
}
// the first i in [0, n] with prefix[i] >= target (prefix is strictly increasing; target <= prefix[n])
ZKP_HD inline uint64_t vs_first_reaching(uint64_t n, const uint64_t* prefix, uint64_t target) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) { const uint64_t mid = lo + (hi - lo) / 2; if (prefix[mid] >= target) hi = mid; else lo = mid + 1; }
    return lo;
}
ZKP_HD inline uint64_t vs_boundary(uint64_t n, const uint64_t* prefix, uint32_t count, uint32_t s) {
    return prefix ? vs_first_reaching(n, prefix, vs_target(prefix[n], count, s)) : vs_target(n, count, s);
}
ZKP_HD inline uint64_t vs_weight_before(const uint64_t* prefix, uint32_t unit, uint64_t i) { return prefix ? prefix[i] : (uint64_t)unit * i; }
// The plan: slice s holds the envelopes [bounds[s], bounds[s + 1]); returns the number of slices (bounds[0 .. count] written, count <= shards
// <= VS_MAX_SHARDS).  prefix: vs_prefix's n + 1 sums, or nullptr for n envelopes of weight `unit` each (>= 1).
ZKP_HD inline uint32_t vs_plan(uint64_t n, const uint64_t* prefix, uint32_t unit, uint32_t shards, uint64_t min_jobs, uint64_t* bounds) {
    bounds[0] = 0;
    if (n == 0) return 0;
    if (min_jobs == 0) min_jobs = 1;
    if (shards > VS_MAX_SHARDS) shards = VS_MAX_SHARDS;
    const uint64_t total = vs_weight_before(prefix, unit, n);
    uint64_t most = total / min_jobs;
    if (most > shards) most = shards;
    if (most > n) most = n;
    for (uint32_t count = (uint32_t)most; count > 1; count--) {
        bool fits = true;
        for (uint32_t s = 1; s <= count && fits; s++) {
            bounds[s] = vs_boundary(n, prefix, count, s);
            fits = vs_weight_before(prefix, unit, bounds[s]) - vs_weight_before(prefix, unit, bounds[s - 1]) >= min_jobs;      // (min_jobs >= 1: not empty either)
        }
        if (fits) return count;
    }
    bounds[1] = n;
    return 1;
}
// The shards that take part, in registration order starting with the caller's: out[] = the shards s with holds[s] != 0 (holds == nullptr:
// all of them).  Returns how many; 0 when the caller's own shard holds nothing -- the call then stays where it is and fails as it always has.
ZKP_HD inline uint32_t vs_participants(uint32_t caller, uint32_t shards, const uint8_t* holds, uint32_t* out) {
    if (caller >= shards || (holds && !holds[caller])) return 0;
    uint32_t m = 0;
    for (uint32_t k = 0; k < shards; k++) { const uint32_t s = (caller + k) % shards; if (!holds || holds[s]) out[m++] = s; }
    return m;
}
// The fan-out data of a call over a list whose items hold envelopes of any scheme (the mixed verifier's list, the statements call's, a list of
// composite containers), one rule for the three: prefix = vs_prefix of the n weights (n + 1 entries); holds[s] = 1 iff shard s holds a usable
// key of every Groth16 circuit the list needs -- need_eq / need_mem say which, has_key[2 * s + kind] (kind 0: equality, 1: membership) what
// shard s holds; a kind that is not needed is not looked at, so a list without Groth16 work leaves every shard in; unit = 0 (the prefix sums
// carry the weights); min_jobs = the larger of the two batch-check thresholds in force, so every slice still takes the one-check path of
// whichever verifier its envelopes reach.
ZKP_HD inline void vs_list_fanout(uint64_t n, const uint32_t* weights, bool need_eq, bool need_mem, uint32_t shards, const uint8_t* has_key, uint64_t bp_min, uint64_t g16_min,
                                  uint64_t* prefix, uint8_t* holds, uint32_t* unit, uint64_t* min_jobs) {
    vs_prefix(n, weights, prefix);
    for (uint32_t s = 0; s < shards; s++) holds[s] = (!need_eq || has_key[2 * s]) && (!need_mem || has_key[2 * s + 1]) ? 1 : 0;
    *unit = 0;
    *min_jobs = bp_min > g16_min ? bp_min : g16_min;
}

}  // namespace zkp
