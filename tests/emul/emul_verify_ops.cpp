// TEST INFRASTRUCTURE: host build of the per-lane steps that hold envelopes against the caller's statements (vst_steps.h), run as the kernels
// k_vst_classify / _bind_equality / _bind_membership / _apply run them: the classification lane after lane, the membership step as 64 lanes
// of one wave whose broadcasts read the other lanes' registers, then the mixed verifier's plan and scatter.  Loaded by
// tests/test_emul_verify_ops.py as a shared library; as a program of its own (it has a main) it runs lists whose blob and lists are
// allocations of exactly their size, which is the form to build with -fsanitize=address,undefined.
#define VST_COUNT_OUTSIDE_READS 1
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/vst_steps.h"
using namespace zkp;

static const uint32_t* mimc_words() {
    static std::vector<uint32_t> mc;
    if (mc.empty()) { ensure_mimc_constants(); for (auto& c : g_mimc_host) put_fr(mc, c); }
    return mc.data();
}

extern "C" {
uint32_t emul_vst_op_bytes(void) { return (uint32_t)sizeof(zkp_hip_op); }
// The call on the host: classify -> bind (live equality and membership envelopes only) -> plan -> (verdict of an envelope's row = accept[i],
// supplied by the test) -> apply.  rec_out (may be null): the n records as the host plan reads them, 32 bytes each.  Returns the number of
// list reads outside [0, n_lists) plus broadcasts from a lane at or above the count: 0 for correct steps.
uint64_t emul_vst_verify(uint64_t n, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists, const uint8_t* blob, const uint64_t* off,
                         const uint8_t* accept, uint8_t* ok, uint8_t* why, uint8_t* rec_out) {
    const uint64_t outside0 = vst_outside_reads();
    uint64_t idle_broadcasts = 0;
    std::vector<VenvRecord> rec(n);
    for (uint64_t i = 0; i < n; i++) rec[i] = step_vst_classify(blob, off, ops, n_lists, n, i);
    for (uint64_t i = 0; i < n; i++) {
        if (rec[i].scheme == ZKP_HIP_OP_EQUALITY) {
            if (!step_vst_bind_equality(blob, off, ops, lists, n_lists, mimc_words(), i)) { rec[i].scheme = 0; rec[i].reserved = ZKP_STMT_STATEMENT; }
        } else if (rec[i].scheme == ZKP_HIP_OP_MEMBERSHIP) {
            const zkp_hip_op o = ops[i];
            VstMemLane L[64];
            for (uint32_t lane = 0; lane < 64; lane++) L[lane] = step_vst_mem_load(blob, off, o, lists, n_lists, i, lane);
            bool all = true;
            for (uint32_t lane = 0; lane < 64; lane++)
                all = step_vst_mem_count(L[lane], lane, o.count, [&](uint32_t j) { if (j >= o.count) idle_broadcasts++; return L[j & 63u]; }) && all;
            if (!all) { rec[i].scheme = 0; rec[i].reserved = ZKP_STMT_STATEMENT; }
        }
    }
    if (rec_out) memcpy(rec_out, rec.data(), 32 * n);
    std::vector<uint32_t> op_row(n);
    VenvPlan P;
    if (ve_plan(n, rec.data(), op_row.data(), P)) return ~0ull;
    std::vector<uint8_t> row_ok(P.total_rows ? P.total_rows : 1, 0);
    VenvView V{};
    V.n = n; V.blob = blob; V.off = off; V.rec = rec.data(); V.op_row = op_row.data(); V.row_ok = row_ok.data();
    for (uint64_t i = 0; i < n; i++) if (op_row[i] != SC_NO_ROW) row_ok[op_row[i]] = accept ? accept[i] : 1;
    for (uint64_t i = 0; i < n; i++) { uint8_t w; ok[i] = step_vst_apply(V, i, w); if (why) why[i] = w; }
    return vst_outside_reads() - outside0 + idle_broadcasts;
}
// what a slice of m ops uploads of the lists: span_out = {lo, count}, ops_out = the re-based ops
void emul_vst_slice(uint64_t m, const zkp_hip_op* ops, uint64_t n_lists, zkp_hip_op* ops_out, uint64_t* span_out) {
    const VstListSpan s = vst_slice_ops(m, ops, n_lists, ops_out);
    span_out[0] = s.lo; span_out[1] = s.count;
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)
void put_le(std::vector<uint8_t>& e, uint64_t x, int nbytes) { for (int b = 0; b < nbytes; b++) e.push_back((uint8_t)(x >> (8 * b))); }
std::vector<uint8_t> envelope(uint32_t scheme, const std::vector<uint8_t>& payload) {
    std::vector<uint8_t> e{2, (uint8_t)scheme};
    put_le(e, payload.size(), 4); put_le(e, 32, 4);
    e.insert(e.end(), payload.begin(), payload.end());
    for (int b = 0; b < 32; b++) e.push_back((uint8_t)(b * 7 + scheme));
    return e;
}
}  // namespace

int main() {
    // membership envelopes of every count at every start offset mod 8, the blob and the lists allocations of exactly their size
    for (uint32_t count : {1u, 2u, 63u, 64u}) for (uint32_t lead = 0; lead < 8; lead++) {
        std::vector<uint8_t> payload; put_le(payload, count, 4);
        for (uint32_t k = 0; k < count; k++) put_le(payload, 1000 + (k % 7), 8);
        payload.resize(payload.size() + 256, 0x5a);
        const std::vector<uint8_t> env = envelope(4, payload);
        std::vector<uint8_t> blob(lead, 0xee); blob.insert(blob.end(), env.begin(), env.end());
        const uint64_t off[2] = {lead, blob.size()};
        std::vector<uint64_t> lists(count);
        for (uint32_t k = 0; k < count; k++) lists[k] = 1000 + ((count - 1 - k) % 7);          // the same multiset in reverse order
        for (uint32_t behind : {0u, 1u}) {
            const zkp_hip_op op{ZKP_HIP_OP_MEMBERSHIP, count, 0, 0, 0, behind};
            uint8_t ok = 9, why = 9;
            EXPECT(emul_vst_verify(1, &op, lists.data(), count, blob.data(), off, nullptr, &ok, &why, nullptr) == 0);
            EXPECT(behind ? ok == 0 && why == ZKP_STMT_STATEMENT : ok == 1 && why == ZKP_STMT_ACCEPTED);
        }
        lists[count - 1] ^= 1ull << 40;
        const zkp_hip_op op{ZKP_HIP_OP_MEMBERSHIP, count, 0, 0, 0, 0};
        uint8_t ok = 9, why = 9;
        EXPECT(emul_vst_verify(1, &op, lists.data(), count, blob.data(), off, nullptr, &ok, &why, nullptr) == 0 && ok == 0 && why == ZKP_STMT_STATEMENT);
    }
    // equality: the commitment form reads exactly four list words and the last 32 bytes of the envelope
    {
        const std::vector<uint8_t> env = envelope(2, std::vector<uint8_t>(256, 3));
        const uint64_t off[2] = {0, env.size()};
        std::vector<uint64_t> lists(4);
        memcpy(lists.data(), env.data() + env.size() - 32, 32);
        for (uint32_t count : {4u, 3u}) {
            const zkp_hip_op op{ZKP_HIP_OP_EQUALITY, count, 5, 6, 0, 0};
            uint8_t ok = 9, why = 9;
            EXPECT(emul_vst_verify(1, &op, lists.data(), 4, env.data(), off, nullptr, &ok, &why, nullptr) == 0);
            EXPECT(count == 4 ? ok == 1 && why == ZKP_STMT_ACCEPTED : ok == 0 && why == ZKP_STMT_STATEMENT);
        }
        const zkp_hip_op by_value{ZKP_HIP_OP_EQUALITY, 0, 5, 5, 0, 0};
        uint8_t ok = 9, why = 9;
        EXPECT(emul_vst_verify(1, &by_value, nullptr, 0, env.data(), off, nullptr, &ok, &why, nullptr) == 0 && ok == 0 && why == ZKP_STMT_STATEMENT);
    }
    if (failures) { std::fprintf(stderr, "emul_verify_ops: %d failure(s)\n", failures); return 1; }
    std::printf("emul_verify_ops ok\n");
    return 0;
}
