// TEST INFRASTRUCTURE: host build of the mixed verifier's glue steps (venv_steps.h): the classification of an envelope, the row plan, the
// blob -> row copy, the scatter of the verdicts.  Loaded by tests/test_emul_verify_mixed.py as a shared library; as a program of its own (it
// has a main) it walks every source and destination alignment with a source allocation of exactly the blob's size, which is the form to
// build with -fsanitize=address,undefined: a read outside the blob is then an error, not a value.
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../libzkp_amd/csrc/venv_steps.h"
using namespace zkp;

extern "C" {
uint32_t emul_ve_record_bytes(void) { return (uint32_t)sizeof(VenvRecord); }
// records of n envelopes (32 bytes each), as k_venv_classify writes them
void emul_ve_classify(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* rec_out) {
    for (uint64_t i = 0; i < n; i++) { const VenvRecord r = step_venv_classify(blob, off, expect, n, i); memcpy(rec_out + 32 * i, &r, 32); }
}
uint32_t emul_ve_consistency_jobs(const uint8_t* env, uint64_t len) { return ve_consistency_jobs(env, len); }
uint32_t emul_ve_weight(const uint8_t* blob, const uint64_t* off, uint64_t n, uint64_t i) { return ve_weight(blob, off, n, i); }
// the rule behind it, as a container's inner envelope reaches it: the scheme byte the caller read, the envelope, its length
uint32_t emul_ve_scheme_weight(uint32_t scheme, const uint8_t* env, uint64_t len) { return ve_scheme_weight((uint8_t)scheme, env, len); }
// the plan of n records: out = rows[7] row0[7] stride[7] base[7] total_rows live bytes (31 u64); returns ve_plan's code
uint32_t emul_ve_plan(uint64_t n, const uint8_t* rec, uint32_t* op_row, uint64_t* out) {
    VenvPlan P;
    const uint32_t rc = ve_plan(n, reinterpret_cast<const VenvRecord*>(rec), op_row, P);
    for (uint32_t k = 0; k < SC_KINDS; k++) { out[k] = P.rows[k]; out[7 + k] = P.row0[k]; out[14 + k] = P.stride[k]; out[21 + k] = P.base[k]; }
    if (!rc) { out[28] = P.total_rows; out[29] = P.live; out[30] = P.bytes; }
    return rc;
}
// the plan's refusal for a list that is never materialised: `rows` live envelopes of `len` bytes of one scheme
uint32_t emul_ve_plan_uniform(uint64_t rows, uint32_t scheme, uint32_t len) {
    std::vector<VenvRecord> rec(rows, VenvRecord{scheme, len, 0, 0, 0, 0});
    std::vector<uint32_t> op_row(rows);
    VenvPlan P;
    return ve_plan(rows, rec.data(), op_row.data(), P);
}
// every lane of a `lanes`-wide wave copies its share of src[0 .. len) to dst; [lo, hi) = the readable blob
void emul_ve_copy(uint8_t* dst, const uint8_t* src, uint32_t len, const uint8_t* lo, const uint8_t* hi, uint32_t lanes) {
    for (uint32_t lane = 0; lane < lanes; lane++) step_venv_copy(dst, src, len, lo, hi, lane, lanes);
}
// classification -> plan -> rows -> (verdict of row g = row_ok[g], supplied by the test through `accept`: accept[i] for envelope i) -> ok.
// rows_out must hold the plan's bytes (emul_ve_plan says how many); row_len / row_p0 / row_p1 hold total_rows entries.
uint32_t emul_ve_pipeline(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, const uint8_t* accept,
                          uint8_t* rows_out, uint32_t* row_len, uint64_t* row_p0, uint64_t* row_p1, uint8_t* ok) {
    std::vector<VenvRecord> rec(n);
    for (uint64_t i = 0; i < n; i++) rec[i] = step_venv_classify(blob, off, expect, n, i);
    std::vector<uint32_t> op_row(n);
    VenvPlan P;
    const uint32_t rc = ve_plan(n, rec.data(), op_row.data(), P);
    if (rc) return rc;
    std::vector<uint8_t> row_ok(P.total_rows ? P.total_rows : 1, 0);
    VenvView V{};
    V.n = n; V.blob = blob; V.off = off; V.rec = rec.data(); V.op_row = op_row.data();
    for (uint32_t k = 0; k < SC_KINDS; k++) { V.row0[k] = P.row0[k]; V.stride[k] = P.stride[k]; V.base[k] = P.base[k]; }
    V.rows = rows_out; V.row_len = row_len; V.row_p0 = row_p0; V.row_p1 = row_p1; V.row_ok = row_ok.data();
    for (uint64_t i = 0; i < n; i++) for (uint32_t lane = 0; lane < 64; lane++) step_venv_unpack(V, i, lane, 64);
    for (uint64_t i = 0; i < n; i++) if (op_row[i] != SC_NO_ROW) row_ok[op_row[i]] = accept[i];
    for (uint64_t i = 0; i < n; i++) ok[i] = step_venv_apply(V, i);
    return 0;
}
}

namespace {
int failures = 0;
#define EXPECT(cond) do { if (!(cond)) { failures++; std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); } } while (0)
}  // namespace

int main() {
    // the copy: every source alignment x destination alignment x length, the source an allocation of exactly the blob
    const uint32_t lens[] = {0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65, 70, 298, 762, 814, 1478, 3527};
    for (uint32_t sa = 0; sa < 16; sa++) for (uint32_t da = 0; da < 4; da++) for (uint32_t len : lens) for (uint32_t before : {0u, 5u}) {
        // the blob: `before` bytes of another envelope, the envelope, nothing behind it; its first byte sits at address = sa (mod 16)
        std::vector<uint8_t> store(before + len + 32);
        uint8_t* blob = store.data();
        while (((uintptr_t)(blob + before) & 15u) != sa) blob++;
        std::vector<uint8_t> exact(before + len);          // a second copy with nothing around it, at whatever alignment the allocator gives
        for (uint32_t i = 0; i < before + len; i++) exact[i] = blob[i] = (uint8_t)(i * 131 + 7 * sa + len);
        std::vector<uint8_t> out(len + 48, 0xA5);
        uint8_t* dst = out.data() + 16;
        while (((uintptr_t)dst & 3u) != da) dst++;
        emul_ve_copy(dst, blob + before, len, blob, blob + before + len, 64);
        EXPECT(len == 0 || memcmp(dst, blob + before, len) == 0);
        for (uint8_t* p = out.data(); p < dst; p++) EXPECT(*p == 0xA5);
        for (uint8_t* p = dst + len; p < out.data() + out.size(); p++) EXPECT(*p == 0xA5);
        std::vector<uint8_t> out2(len + 8, 0x5A);
        emul_ve_copy(out2.data() + da, exact.data() + before, len, exact.data(), exact.data() + exact.size(), 64);
        EXPECT(len == 0 || memcmp(out2.data() + da, exact.data() + before, len) == 0);
    }
    // a header at each limit
    auto envelope = [](uint32_t scheme, uint32_t plen, uint32_t clen, uint32_t total) {
        std::vector<uint8_t> e(total, 0);
        if (total >= 10) { e[0] = 2; e[1] = (uint8_t)scheme; for (int b = 0; b < 4; b++) { e[2 + b] = (uint8_t)(plen >> (8 * b)); e[6 + b] = (uint8_t)(clen >> (8 * b)); } }
        return e;
    };
    auto scheme_of = [](const std::vector<uint8_t>& e, uint8_t expect) {
        const uint64_t off[2] = {0, e.size()};
        return step_venv_classify(e.data(), off, expect == 0xff ? nullptr : &expect, 1, 0).scheme;
    };
    EXPECT(scheme_of(envelope(2, 256, 32, 298), 0xff) == 2 && scheme_of(envelope(2, 256, 32, 298), 0) == 2 && scheme_of(envelope(2, 256, 32, 298), 2) == 2);
    EXPECT(scheme_of(envelope(2, 256, 32, 298), 1) == 0 && scheme_of(envelope(2, 256, 32, 298), 9) == 0);
    EXPECT(scheme_of(envelope(2, 256, 31, 297), 0xff) == 0 && scheme_of(envelope(2, 256, 32, 299), 0xff) == 0 && scheme_of(envelope(2, 0, 0, 9), 0xff) == 0);
    EXPECT(scheme_of(envelope(6, 900 * 1024, 32, 10 + 900 * 1024 + 32), 0xff) == 6 && scheme_of(envelope(6, 900 * 1024 + 1, 32, 10 + 900 * 1024 + 33), 0xff) == 0);
    EXPECT(scheme_of(envelope(6, 100, 256, 366), 0xff) == 6 && scheme_of(envelope(6, 100, 257, 367), 0xff) == 0);
    EXPECT(scheme_of(envelope(0, 256, 32, 298), 0xff) == 0 && scheme_of(envelope(7, 256, 32, 298), 0xff) == 0);
    EXPECT(emul_ve_plan_uniform((1u << 20) + 1, 1, 4096) == 1 && emul_ve_plan_uniform(1u << 20, 1, 4096) == 0 && emul_ve_plan_uniform(1u << 22, 2, 298) == 0);
    if (failures) { std::fprintf(stderr, "emul_verify_mixed: %d failure(s)\n", failures); return 1; }
    std::printf("emul_verify_mixed ok\n");
    return 0;
}
