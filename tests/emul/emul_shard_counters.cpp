// TEST INFRASTRUCTURE: host build of the shards' counter table (shard_counters.h): the family table, the read that sums one family over the
// shards, and the tally with its two counting rules.  Loaded by tests/test_emul_shard_counters.py as a shared library; as a program of its
// own (it has a main) it walks the same properties, which is the form to build with -fsanitize=address,undefined.
#include <cstdio>
#include <vector>
#include "../../libzkp_amd/csrc/shard_counters.h"
using namespace zkp;

extern "C" {
uint32_t emul_ctr_families(void) { return FAM_COUNT; }
uint32_t emul_ctr_max_fields(void) { return CTR_MAX_FIELDS; }
uint32_t emul_ctr_fields(uint32_t family) { return family < FAM_COUNT ? CTR_FIELDS[family] : 0; }
// the family ids in the order the test names them: g16_verify, batch_self_check, verify_fanout, verify_mixed, bp_localise, composites, seal, statements, key_check
void emul_ctr_family_ids(uint32_t* out) {
    const uint32_t ids[] = {FAM_G16_VERIFY, FAM_BATCH_SELF_CHECK, FAM_VERIFY_FANOUT, FAM_VERIFY_MIXED, FAM_BP_LOCALISE, FAM_COMPOSITES, FAM_SEAL, FAM_STATEMENTS, FAM_KEY_CHECK};
    for (uint32_t k = 0; k < 9; k++) out[k] = ids[k];
}
// Tables of `shards` shards as flat arrays, [shard][family] for ms and [shard][family][CTR_MAX_FIELDS] for the counts, read in place:
// family `family` summed into *ms and outs[0 .. nouts) (null entries skipped), reset or not, each shard under a lock of its own.
void emul_ctr_read(uint32_t shards, double* ms_table, uint64_t* v_table, uint32_t family, int reset, double* ms, uint64_t** outs, uint32_t nouts) {
    std::vector<ShardCounters> tables(shards);
    std::vector<std::mutex> mu(shards);
    std::vector<ShardCounters*> ptr(shards); std::vector<std::mutex*> locks(shards);
    for (uint32_t s = 0; s < shards; s++) {
        ptr[s] = &tables[s]; locks[s] = &mu[s];
        for (uint32_t f = 0; f < FAM_COUNT; f++) {
            tables[s][f].ms = ms_table[s * FAM_COUNT + f];
            for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) tables[s][f].v[k] = v_table[(s * FAM_COUNT + f) * CTR_MAX_FIELDS + k];
        }
    }
    uint64_t* o[CTR_MAX_FIELDS] = {nullptr, nullptr, nullptr, nullptr};
    for (uint32_t k = 0; k < nouts && k < CTR_MAX_FIELDS; k++) o[k] = outs[k];
    if (nouts == 2) counters_read(ptr.data(), locks.data(), shards, family, reset != 0, ms, {o[0], o[1]});
    else if (nouts == 3) counters_read(ptr.data(), locks.data(), shards, family, reset != 0, ms, {o[0], o[1], o[2]});
    else counters_read(ptr.data(), locks.data(), shards, family, reset != 0, ms, {o[0], o[1], o[2], o[3]});
    for (uint32_t s = 0; s < shards; s++) for (uint32_t f = 0; f < FAM_COUNT; f++) {
        ms_table[s * FAM_COUNT + f] = tables[s][f].ms;
        for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) v_table[(s * FAM_COUNT + f) * CTR_MAX_FIELDS + k] = tables[s][f].v[k];
    }
}
// One tally of `family` with the fields `set` (CTR_MAX_FIELDS entries) in a function that leaves early (`early`: through a return in the
// middle) or at its end; rule: 0 ALWAYS, 1 COMMITTED and committed before the end, 2 COMMITTED and never committed.  The table afterwards:
// v_out [FAM_COUNT][CTR_MAX_FIELDS]; returns 1 when the family's ms is >= 0 and every other family's is exactly 0.
static int tally_body(ShardCounters& table, uint32_t family, int rule, int early, const uint64_t* set) {
    Tally tally(table, family, rule == 0 ? Tally::ALWAYS : Tally::COMMITTED);
    for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) tally[k] = set[k];
    if (early) return -1;          // (what a HIP_TRY that fails does)
    if (rule == 1) tally.commit();
    return 0;
}
int emul_ctr_tally(uint32_t family, int rule, int early, const uint64_t* set, uint64_t* v_out) {
    ShardCounters table;
    (void)tally_body(table, family, rule, early, set);
    int ms_ok = 1;
    for (uint32_t f = 0; f < FAM_COUNT; f++) {
        if (f == family ? !(table[f].ms >= 0) : table[f].ms != 0) ms_ok = 0;
        for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) v_out[f * CTR_MAX_FIELDS + k] = table[f].v[k];
    }
    return ms_ok;
}
// The Bulletproofs verifiers' tally, made after a failed check, with segment checks and jobs counted `times` times each (0: the call returns
// right after making it): the FAM_BP_LOCALISE fields afterwards into v_out (CTR_MAX_FIELDS entries)
void emul_ctr_bp_localise(uint32_t times, uint64_t segment_checks, uint64_t jobs_again, uint64_t* v_out) {
    ShardCounters table;
    {
        std::unique_ptr<Tally> tally = bp_localise_tally(table);
        for (uint32_t t = 0; t < times; t++) { (*tally)[CTR_BP_SEGMENT_CHECKS] += segment_checks; (*tally)[CTR_BP_JOBS_AGAIN] += jobs_again; }
    }
    for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) v_out[k] = table[FAM_BP_LOCALISE].v[k];
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)
}  // namespace

int main() {
    uint32_t total_fields = 0;
    for (uint32_t f = 0; f < FAM_COUNT; f++) { EXPECT(CTR_FIELDS[f] >= 2 && CTR_FIELDS[f] <= CTR_MAX_FIELDS); total_fields += CTR_FIELDS[f]; }
    EXPECT(FAM_COUNT == 9 && total_fields == 25);
    for (uint32_t shards : {1u, 2u, 64u}) for (uint32_t family = 0; family < FAM_COUNT; family++) for (int reset = 0; reset < 2; reset++) {
        std::vector<double> ms((size_t)shards * FAM_COUNT); std::vector<uint64_t> v((size_t)shards * FAM_COUNT * CTR_MAX_FIELDS);
        for (size_t i = 0; i < ms.size(); i++) ms[i] = 0.5 * (double)(i + 1);
        for (size_t i = 0; i < v.size(); i++) v[i] = 1000 * i + 7;
        const std::vector<double> ms0 = ms; const std::vector<uint64_t> v0 = v;
        double got_ms = -1; uint64_t got[CTR_MAX_FIELDS] = {99, 99, 99, 99};
        uint64_t* outs[CTR_MAX_FIELDS] = {&got[0], nullptr, &got[2], &got[3]};          // the second out is null
        emul_ctr_read(shards, ms.data(), v.data(), family, reset, &got_ms, outs, CTR_FIELDS[family]);
        double want_ms = 0; uint64_t want[CTR_MAX_FIELDS] = {0, 0, 0, 0};
        for (uint32_t s = 0; s < shards; s++) { want_ms += ms0[s * FAM_COUNT + family]; for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) want[k] += v0[(s * FAM_COUNT + family) * CTR_MAX_FIELDS + k]; }
        EXPECT(got_ms == want_ms && got[0] == want[0] && got[1] == 99);
        for (uint32_t k = 2; k < CTR_MAX_FIELDS; k++) EXPECT(got[k] == (k < CTR_FIELDS[family] ? want[k] : 99));
        for (uint32_t s = 0; s < shards; s++) for (uint32_t f = 0; f < FAM_COUNT; f++) {
            const bool zeroed = reset && f == family;
            EXPECT(ms[s * FAM_COUNT + f] == (zeroed ? 0 : ms0[s * FAM_COUNT + f]));
            for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) { const size_t i = (s * FAM_COUNT + f) * CTR_MAX_FIELDS + k; EXPECT(v[i] == (zeroed ? 0 : v0[i])); }
        }
    }
    const uint64_t set[CTR_MAX_FIELDS] = {3, 5, 7, 11};
    for (uint32_t family = 0; family < FAM_COUNT; family++) for (int rule = 0; rule < 3; rule++) for (int early = 0; early < 2; early++) {
        uint64_t v[FAM_COUNT * CTR_MAX_FIELDS];
        EXPECT(emul_ctr_tally(family, rule, early, set, v) == 1);
        const bool counted = rule == 0 || (rule == 1 && !early);
        for (uint32_t f = 0; f < FAM_COUNT; f++) for (uint32_t k = 0; k < CTR_MAX_FIELDS; k++) EXPECT(v[f * CTR_MAX_FIELDS + k] == (counted && f == family ? set[k] : 0));
    }
    {
        ShardCounters table;
        { Tally tally(table, FAM_SEAL); tally[CTR_SEAL_BYTES] = 9; tally.commit(); tally.commit(); }          // a second commit and the scope's end add nothing more
        EXPECT(table[FAM_SEAL].v[CTR_SEAL_BYTES] == 9);
    }
    uint64_t bp[CTR_MAX_FIELDS];
    emul_ctr_bp_localise(0, 0, 0, bp); EXPECT(bp[CTR_BP_FAILED_CHECKS] == 1 && bp[CTR_BP_SEGMENT_CHECKS] == 0 && bp[CTR_BP_JOBS_AGAIN] == 0);
    emul_ctr_bp_localise(2, 16, 40, bp); EXPECT(bp[CTR_BP_FAILED_CHECKS] == 1 && bp[CTR_BP_SEGMENT_CHECKS] == 32 && bp[CTR_BP_JOBS_AGAIN] == 80);
    if (failures) { std::fprintf(stderr, "emul_shard_counters: %d failure(s)\n", failures); return 1; }
    std::printf("emul_shard_counters ok\n");
    return 0;
}
