// The host-side counters of a shard: one table for every family the library counts, the tally that feeds it and the read that sums it
// over the shards.  Pure host code (no HIP), shared by the host (zkp_hip.hip: Device::counters, read_counters and every call site) and the host
// build of tests/emul/emul_shard_counters.cpp.
//
// A family is `ms` of host wall time plus up to CTR_MAX_FIELDS counts, in the order of the uint64_t* parameters of the export that reads it:
//
//   FAM_G16_VERIFY        zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_G16_VERIFY)        segment checks, envelopes verified one by one
//   FAM_BATCH_SELF_CHECK  zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_BATCH_SELF_CHECK)  ops verified, ops refused
//   FAM_VERIFY_FANOUT     zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_VERIFY_FANOUT)     slices run on this shard, their envelopes
//   FAM_VERIFY_MIXED      zkp_hip_profile_read_kernel(ZKP_HIP_COUNTER_VERIFY_MIXED)      scheme passes, envelopes that got a row
//   FAM_BP_LOCALISE       zkp_hip_bp_localise_counters                                  failed checks, segment checks, jobs verified again
//   FAM_COMPOSITES        zkp_hip_composites_counters                                   composites, malformed, envelopes
//   FAM_SEAL              libzkp_seal_counters                                          containers, sealed, envelopes, bytes
//   FAM_STATEMENTS        zkp_stmt_counters                                             envelopes, refused: envelope / statement / proof
//   FAM_KEY_CHECK         zkpkeycheck_counters                                          loads checked, entries checked, refused
//
// The first four sit at `which - ZKP_HIP_COUNTER_G16_VERIFY` (zkp_hip.hip asserts it).  Two counting rules (DESIGN.md R22 says which site
// follows which): a Tally of rule ALWAYS adds when its scope ends, whichever way; one of rule COMMITTED adds at commit() and never otherwise.
#pragma once
#include <chrono>
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <memory>
#include <mutex>

namespace zkp {

constexpr uint32_t CTR_MAX_FIELDS = 4;
enum CounterFamily : uint32_t { FAM_G16_VERIFY, FAM_BATCH_SELF_CHECK, FAM_VERIFY_FANOUT, FAM_VERIFY_MIXED, FAM_BP_LOCALISE, FAM_COMPOSITES, FAM_SEAL, FAM_STATEMENTS, FAM_KEY_CHECK,
                               FAM_COUNT };
constexpr uint32_t CTR_FIELDS[FAM_COUNT] = {2, 2, 2, 2, 3, 3, 4, 4, 3};
enum : uint32_t {
    CTR_G16_SEGMENT_CHECKS = 0, CTR_G16_ENVELOPES,
    CTR_SELF_CHECK_VERIFIED = 0, CTR_SELF_CHECK_REFUSED,
    CTR_FANOUT_SLICES = 0, CTR_FANOUT_ENVELOPES,
    CTR_MIXED_PASSES = 0, CTR_MIXED_LIVE,
    CTR_BP_FAILED_CHECKS = 0, CTR_BP_SEGMENT_CHECKS, CTR_BP_JOBS_AGAIN,
    CTR_COMP_COMPOSITES = 0, CTR_COMP_MALFORMED, CTR_COMP_ENVELOPES,
    CTR_SEAL_CONTAINERS = 0, CTR_SEAL_SEALED, CTR_SEAL_ENVELOPES, CTR_SEAL_BYTES,
    CTR_STMT_ENVELOPES = 0, CTR_STMT_REFUSED_ENVELOPE, CTR_STMT_REFUSED_STATEMENT, CTR_STMT_REFUSED_PROOF,
    CTR_KEY_LOADS_CHECKED = 0, CTR_KEY_ENTRIES_CHECKED, CTR_KEY_REFUSED,
};

struct ShardCounter { double ms = 0; uint64_t v[CTR_MAX_FIELDS] = {0, 0, 0, 0}; };
// every family of one shard (Device::counters); `= ShardCounters()` zeroes them all
struct ShardCounters {
    ShardCounter family[FAM_COUNT];
    ShardCounter& operator[](uint32_t f) { return family[f]; }
};

inline void counter_add(ShardCounter& c, double ms, const uint64_t* v) {
    c.ms += ms;
    for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) c.v[k] += v[k];
}
// Family `f` summed over n shards; reset: each shard's counter of that family is zeroed as it is read.  locks (may be null): shard k is read
// and reset under *locks[k], one lock at a time.  *ms and the outs (in field order; fewer than the family has is fine) are overwritten with
// the sums, null ones skipped.
inline void counters_read(ShardCounters* const* shards, std::mutex* const* locks, size_t n, uint32_t f, bool reset, double* ms, std::initializer_list<uint64_t*> outs) {
    ShardCounter total;
    for (size_t k = 0; k < n; k++) {
        std::unique_lock<std::mutex> lk;
        if (locks) lk = std::unique_lock<std::mutex>(*locks[k]);
        ShardCounter& c = (*shards[k])[f];
        counter_add(total, c.ms, c.v);
        if (reset) c = ShardCounter();
    }
    if (ms) *ms = total.ms;
    uint32_t field = 0;
    for (uint64_t* out : outs) { if (out && field < CTR_MAX_FIELDS) *out = total.v[field]; field++; }
}

// What one call, slice or check counts into family `f` of `table`: the fields are set through tally[CTR_...] and added together with the
// time since the tally was made -- once.  The thread that owns a tally holds the lock of the shard `table` belongs to.
struct Tally {
    enum Rule { ALWAYS, COMMITTED };
    ShardCounter& into; const Rule rule; bool added = false;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    uint64_t v[CTR_MAX_FIELDS] = {0, 0, 0, 0};
    Tally(ShardCounters& table, uint32_t f, Rule r = ALWAYS) : into(table[f]), rule(r) {}
    Tally(const Tally&) = delete;
    Tally& operator=(const Tally&) = delete;
    uint64_t& operator[](uint32_t field) { return v[field]; }
    void commit() {
        if (added) return;
        added = true;
        counter_add(into, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), v);
    }
    ~Tally() { if (rule == ALWAYS) commit(); }
};
// The Bulletproofs verifiers make theirs once a batch check has not stood: that is the one failed check it counts, whatever follows.
inline std::unique_ptr<Tally> bp_localise_tally(ShardCounters& table) {
    std::unique_ptr<Tally> t(new Tally(table, FAM_BP_LOCALISE));
    (*t)[CTR_BP_FAILED_CHECKS] = 1;
    return t;
}

}  // namespace zkp
