// TEST INFRASTRUCTURE: host build of the batch self-check's per-lane steps (batch_self_check.h): the lens rows and the row <-> op map,
// the Groth16 binding (equality commitment = MiMC of the staged value, membership set = the staged set) and the scatter of the verdict
// rows back to op order, run lane after lane as the kernels k_self_check_rows / _bind_g16 / _apply run them.
#include "../../libzkp_amd/csrc/g16_circuit.h"
#include "../../libzkp_amd/csrc/batch_self_check.h"
#include <vector>
using namespace zkp;

static const uint32_t* mimc_words() {
    static std::vector<uint32_t> mc;
    if (mc.empty()) { ensure_mimc_constants(); for (auto& c : g_mimc_host) put_fr(mc, c); }
    return mc.data();
}
static void geometry(SelfCheckView& V, const uint64_t* base, const uint64_t* stride, const uint32_t* row0, const uint32_t* rows) {
    for (uint32_t k = 0; k < SC_KINDS; k++) { V.base[k] = base[k]; V.stride[k] = stride[k]; V.row0[k] = row0[k]; V.rows[k] = rows[k]; }
}

extern "C" {
uint32_t emul_sc_no_row(void) { return SC_NO_ROW; }
uint32_t emul_sc_row_align(void) { return SC_ROW_ALIGN; }
// k_self_check_rows over n ops; base / stride / row0 / rows are indexed by op kind (7 entries)
void emul_sc_rows(uint32_t n, const uint64_t* src_off, const uint32_t* len_fixed, const uint32_t* dyn_ix, const uint8_t* dyn_kind, const int32_t* status_fixed,
                  const uint32_t* dyn_len, const int32_t* dyn_status, const uint8_t* op_variant, const uint64_t* base, const uint64_t* stride,
                  const uint32_t* row0, const uint32_t* rows, uint32_t* row_len, uint32_t* row_op, uint32_t* op_row) {
    SelfCheckView V{};
    V.n = n; V.src_off = src_off; V.len_fixed = len_fixed; V.dyn_ix = dyn_ix; V.dyn_kind = dyn_kind; V.status_fixed = status_fixed;
    V.dyn_len = dyn_len; V.dyn_status = dyn_status; V.op_variant = op_variant; geometry(V, base, stride, row0, rows);
    V.row_len = row_len; V.row_op = row_op; V.op_row = op_row;
    for (uint32_t i = 0; i < n; i++) step_self_check_rows(V, i);
}
int emul_sc_equality_bound(const uint8_t* env, uint64_t value) { return sc_equality_bound(env, value, mimc_words()) ? 1 : 0; }
int emul_sc_membership_bound(const uint8_t* env, const uint64_t* set64, uint32_t count) { return sc_membership_bound(env, set64, count) ? 1 : 0; }
// k_self_check_bind_g16 over every equality and membership row
void emul_sc_bind(const uint8_t* arena, const uint64_t* base, const uint64_t* stride, const uint32_t* row0, const uint32_t* rows, const uint32_t* row_len,
                  uint8_t* row_ok, const uint64_t* eq_value, const uint64_t* mem_sets, const uint32_t* mem_len) {
    SelfCheckView V{};
    geometry(V, base, stride, row0, rows);
    V.arena = arena; V.row_len = const_cast<uint32_t*>(row_len); V.row_ok = row_ok; V.eq_value = eq_value; V.mem_sets = mem_sets; V.mem_len = mem_len; V.mimc_c = mimc_words();
    for (uint32_t t = 0; t < rows[2] + rows[4]; t++) step_self_check_bind_g16(V, t);
}
// k_self_check_apply over n ops, then the exclusive prefix sum k_batch_scan takes of the lengths; counters[0] = verified, [1] = refused
void emul_sc_apply(uint32_t n, const uint32_t* op_row, const uint8_t* row_ok, uint32_t* len, int32_t* status, uint64_t* out_off, uint32_t* counters) {
    SelfCheckView V{};
    V.n = n; V.op_row = const_cast<uint32_t*>(op_row); V.row_ok = const_cast<uint8_t*>(row_ok); V.len = len; V.status = status;
    counters[0] = counters[1] = 0;
    for (uint32_t i = 0; i < n; i++) { const uint32_t f = step_self_check_apply(V, i); counters[0] += f & 1u; counters[1] += (f >> 1) & 1u; }
    uint64_t run = 0;
    for (uint32_t i = 0; i < n; i++) { out_off[i] = run; run += len[i]; }
    out_off[n] = run;
}
void emul_sc_flip(uint8_t* arena, const uint64_t* src_off, uint32_t j, uint32_t byte) { step_self_check_flip(arena, src_off, j, byte); }
}
