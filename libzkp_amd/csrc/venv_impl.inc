// The mixed verifier (include/libzkp_hip_verify.h), host side and glue kernels of libzkp_hip (included by zkp_hip.hip).  Steps: venv_steps.h.
// The verifiers themselves are the cores of the per-scheme calls (verify_bp_device, verify_g16_core, verify_stark_device), called unchanged,
// one after the other on the shard's stream by verify_scheme_passes below, which the batch self-check (batch_impl.inc) runs too.
static_assert(VE_RANGE_PROOF_BYTES == RP_BYTES, "venv_steps.h: the range proof inside a consistency envelope");
static_assert(SC_KINDS == ZKP_HIP_OP_CONSISTENCY + 1, "scheme bytes index the row plan");

__global__ void __launch_bounds__(256) k_venv_classify(const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint64_t n, VenvRecord* rec) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) rec[i] = step_venv_classify(blob, off, expect, n, i);
}
constexpr uint32_t VENV_UNPACK_TB = 256;          // four waves, one envelope each
__global__ void __launch_bounds__(VENV_UNPACK_TB) k_venv_unpack(VenvView V) {
    const uint64_t i = (uint64_t)blockIdx.x * (VENV_UNPACK_TB / 64) + threadIdx.x / 64;
    if (i < V.n) step_venv_unpack(V, i, threadIdx.x & 63u, 64);
}
__global__ void __launch_bounds__(256) k_venv_apply(VenvView V, uint8_t* ok) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < V.n) ok[i] = step_venv_apply(V, i);
}

namespace {

// One scheme's rows for verify_scheme_passes: n envelopes at `stride` bytes in `rows`, lens[i] bytes used, verdicts into ok (all device
// pointers); p0 / p1: the scheme's parameter columns (range: mins, maxs; threshold: thresholds; improvement: old values); jobs: a consistency
// envelope's job counts (host, n entries).
struct SchemePass { uint64_t n = 0; const uint8_t* rows = nullptr; uint64_t stride = 0; const uint32_t* lens = nullptr; const uint64_t *p0 = nullptr, *p1 = nullptr;
                    uint8_t* ok = nullptr; const uint32_t* jobs = nullptr; };
// Each scheme's verifier core over its rows (K is indexed by ZKP_HIP_OP_*), one after the other on the bound shard's stream: range, threshold,
// consistency, equality, membership, improvement; a kind without rows is skipped.  *passes (may be null) is raised by the number run.  The two
// Groth16 kinds share one host copy of the batch check's verdicts and run under a Quiesce: their scratch comes from the caller's `mem`.
// after_g16() runs behind them when either had rows (the self-check binds their public inputs there).
template <class F> int verify_scheme_passes(const SchemePass (&K)[SC_KINDS], DevScope& mem, uint64_t* passes, F after_g16) {
    int rc;
    uint64_t ran = 0;
    for (int s : {ZKP_HIP_OP_RANGE, ZKP_HIP_OP_THRESHOLD, ZKP_HIP_OP_CONSISTENCY}) {
        const SchemePass& k = K[s];
        if (!k.n) continue;
        ran++;
        if ((rc = verify_bp_device(s, k.n, k.rows, k.stride, k.lens, k.p0, k.p1, k.ok, k.jobs, nullptr))) return rc;
    }
    const SchemePass &eq = K[ZKP_HIP_OP_EQUALITY], &me = K[ZKP_HIP_OP_MEMBERSHIP], &im = K[ZKP_HIP_OP_IMPROVEMENT];
    if (eq.n || me.n) {
        Quiesce quiesce;
        std::vector<uint8_t> h_ok(eq.n > me.n ? eq.n : me.n);      // the batch check's verdicts, read by its localisation pass
        if (eq.n) { ran++; if ((rc = verify_g16_core(G16_EQUALITY, eq.n, eq.rows, eq.stride, eq.lens, eq.ok, h_ok.data(), mem))) return rc; }
        if (me.n) { ran++; if ((rc = verify_g16_core(G16_MEMBERSHIP, me.n, me.rows, me.stride, me.lens, me.ok, h_ok.data(), mem))) return rc; }
        quiesce.armed = false;
        if ((rc = after_g16())) return rc;
    }
    if (im.n) { ran++; if ((rc = verify_stark_device(im.n, im.rows, im.stride, im.lens, im.p0, im.ok))) return rc; }
    if (passes) *passes += ran;
    return 0;
}

// Everything behind the records, on the bound shard, shared by every call that classifies envelopes into VenvRecords (this file's, and
// vst_impl.inc's against statements): the records back (`rec` receives them), the plan, the rows, the cores, then apply(V) -- the launch that
// takes the row verdicts back to the caller's order, into d_ok (device, n bytes) -- and the wait that ends the call; ok_host (may be null)
// receives the verdicts before it.  *passes / *live: scheme passes run / envelopes that got a row.
template <class Apply>
int verify_records_core(uint64_t n, const uint8_t* d_blob, const uint64_t* d_off, const VenvRecord* d_rec, std::vector<VenvRecord>& rec, uint8_t* d_ok, uint8_t* ok_host,
                        uint64_t* passes_out, uint64_t* live_out, Apply apply) {
    hipStream_t st = dev().stream;
    DevScope mem;
    rec.resize(n);
    HIP_TRY(hipMemcpyAsync(rec.data(), d_rec, sizeof(VenvRecord) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::vector<uint32_t> op_row(n);
    VenvPlan P;
    const uint32_t too_large = ve_plan(n, rec.data(), op_row.data(), P);
    if (too_large) return fail(ZKP_HIP_E_ARGUMENT, "the envelopes of one scheme would take more than 4 GiB as rows (split the call)");
    // nothing is enqueued unless every key the list needs is there
    for (int kind : {G16_EQUALITY, G16_MEMBERSHIP})
        if (P.rows[kind == G16_EQUALITY ? ZKP_HIP_OP_EQUALITY : ZKP_HIP_OP_MEMBERSHIP] && !g16s().key[kind].vk_ready)
            return fail(ZKP_HIP_E_ARGUMENT, "no (usable) key loaded for this circuit (zkp_hip_groth16_load_key)");
    const uint32_t R = P.total_rows ? P.total_rows : 1;
    VenvView V{};
    V.n = n; V.blob = d_blob; V.off = d_off; V.rec = d_rec;
    uint32_t* d_op_row = nullptr;
    HIP_TRY(mem.alloc(&d_op_row, 4 * n)); HIP_TRY(mem.alloc(&V.rows, P.bytes)); HIP_TRY(mem.alloc(&V.row_len, 4ull * R));
    HIP_TRY(mem.alloc(&V.row_p0, 8ull * R)); HIP_TRY(mem.alloc(&V.row_p1, 8ull * R)); HIP_TRY(mem.alloc(&V.row_ok, R));
    V.op_row = d_op_row;
    for (uint32_t k = 0; k < SC_KINDS; k++) { V.row0[k] = P.row0[k]; V.stride[k] = P.stride[k]; V.base[k] = P.base[k]; }
    HIP_TRY(hipMemcpyAsync(d_op_row, op_row.data(), 4 * n, hipMemcpyHostToDevice, st));
    uint64_t passes = 0;
    if (P.live) {
        HIP_TRY(hipMemsetAsync(V.rows, 0, P.bytes, st));          // what a row holds behind its envelope, and the rows' alignment gaps
        HIP_TRY(hipMemsetAsync(V.row_len, 0, 4ull * R, st));
        HIP_TRY(hipMemsetAsync(V.row_ok, 0, R, st));
        k_venv_unpack<<<(uint32_t)((n + VENV_UNPACK_TB / 64 - 1) / (VENV_UNPACK_TB / 64)), VENV_UNPACK_TB, 0, st>>>(V);
        HIP_TRY(hipGetLastError());
        std::vector<uint32_t> jobs; jobs.reserve(P.rows[ZKP_HIP_OP_CONSISTENCY]);          // in row order = envelope order
        if (P.rows[ZKP_HIP_OP_CONSISTENCY]) for (uint64_t i = 0; i < n; i++) if (rec[i].scheme == ZKP_HIP_OP_CONSISTENCY) jobs.push_back(rec[i].jobs);
        SchemePass K[SC_KINDS];          // (a core ignores the columns its scheme has no use for)
        for (uint32_t k = 0; k < SC_KINDS; k++)
            K[k] = {P.rows[k], V.rows + P.base[k], P.stride[k], V.row_len + P.row0[k], V.row_p0 + P.row0[k], V.row_p1 + P.row0[k], V.row_ok + P.row0[k], jobs.data()};
        const int rc = verify_scheme_passes(K, mem, &passes, [] { return 0; });
        if (rc) return rc;
    }
    const int arc = apply(V);
    if (arc) return arc;
    if (ok_host) HIP_TRY(hipMemcpyAsync(ok_host, d_ok, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *passes_out = passes; *live_out = P.live;
    return 0;
}

// The call on device pointers, on the bound shard: classification, then verify_records_core with k_venv_apply; the verdicts into d_ok
// (device, n bytes); ok_host (may be null) also receives them before the wait that ends the call.
int verify_envelopes_core(uint64_t n, const uint8_t* d_blob, const uint64_t* d_off, const uint8_t* d_expect, uint8_t* d_ok, uint8_t* ok_host) {
    Tally tally(dev().counters, FAM_VERIFY_MIXED, Tally::COMMITTED);          // a call that fails is not counted
    hipStream_t st = dev().stream;
    DevScope mem;
    VenvRecord* d_rec = nullptr;
    HIP_TRY(mem.alloc(&d_rec, sizeof(VenvRecord) * n));
    const uint32_t lane_blocks = (uint32_t)((n + 255) / 256);
    k_venv_classify<<<lane_blocks, 256, 0, st>>>(d_blob, d_off, d_expect, n, d_rec);
    HIP_TRY(hipGetLastError());
    std::vector<VenvRecord> rec;
    uint64_t passes = 0, live = 0;
    const int rc = verify_records_core(n, d_blob, d_off, d_rec, rec, d_ok, ok_host, &passes, &live, [&](const VenvView& V) {
        k_venv_apply<<<lane_blocks, 256, 0, st>>>(V, d_ok);
        HIP_TRY(hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    tally[CTR_MIXED_PASSES] = passes; tally[CTR_MIXED_LIVE] = live;
    tally.commit();
    return 0;
}

// The host-buffer form on the bound shard, for the m envelopes whose offsets start at `off` (m + 1 entries): the span's upload (SpanUpload)
// and `expect`; then the core.
int verify_envelopes_host(uint64_t m, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok) {
    SpanUpload up; bool empty;
    int rc = up.open(m, blob, off, &empty);
    if (rc) return rc;
    if (empty) { memset(ok, 0, m); return 0; }
    uint8_t* d_expect = nullptr;
    if (expect) { HIP_TRY(up.mem.alloc(&d_expect, m)); HIP_TRY(hipMemcpyAsync(d_expect, expect, m, hipMemcpyHostToDevice, dev().stream)); }
    return verify_envelopes_core(m, up.d_blob, up.d_off, d_expect, up.d_ok, ok);
}

// The fan-out data of a host-buffer call over a list of envelopes of any scheme (verify_call), for this file's call, vst_impl.inc's and
// composite_impl.inc's: the rule is vs_list_fanout (verify_shards.h).  weights: one per item of the list; need[kind]: the list holds work for
// the Groth16 circuit `kind`, so a shard takes part only with a usable key of it -- asked here, of every candidate, and nowhere else.
// Minimum slice: the larger of the two batch-check thresholds in force.
int list_fanout(const std::vector<uint32_t>& weights, const bool (&need)[2], const std::vector<Device*>& shards, VerifyFanout& F) {
    static_assert(G16_EQUALITY == 0 && G16_MEMBERSHIP == 1, "need[] and the key table are indexed by circuit kind");
    std::vector<uint8_t> has_key(2 * shards.size(), 0);
    for (size_t s = 0; s < shards.size(); s++) {
        bool has = true;          // (a shard that lacks the first needed key is not asked for the second: it takes no part either way)
        for (int kind : {G16_EQUALITY, G16_MEMBERSHIP}) if (need[kind]) has_key[2 * s + kind] = has = has && g16_shard_holds_vk(shards[s], kind);
    }
    F.prefix.resize(weights.size() + 1); F.holds.resize(shards.size());
    vs_list_fanout(weights.size(), weights.data(), need[G16_EQUALITY], need[G16_MEMBERSHIP], (uint32_t)shards.size(), has_key.data(), bp_min_slice(), g16_min_slice(),
                   F.prefix.data(), F.holds.data(), &F.unit, &F.min_jobs);
    return 0;
}
// The mixed verifier's: weights from ve_weight; a key is needed when its scheme byte occurs in an envelope that lies inside the blob.
int verify_envelopes_plan(uint64_t n, const uint8_t* blob, const uint64_t* off, const std::vector<Device*>& shards, VerifyFanout& F) {
    std::vector<uint32_t> weights(n);
    bool need[2] = {false, false};
    for (uint64_t i = 0; i < n; i++) {
        weights[i] = ve_weight(blob, off, n, i);
        if (off[i + 1] >= off[i] && off[i] >= off[0] && off[i + 1] <= off[n] && off[i + 1] - off[i] >= 2) {
            const uint8_t s = blob[off[i] + 1];
            if (s == ZKP_HIP_OP_EQUALITY) need[G16_EQUALITY] = true;
            if (s == ZKP_HIP_OP_MEMBERSHIP) need[G16_MEMBERSHIP] = true;
        }
    }
    return list_fanout(weights, need, shards, F);
}

}  // namespace

extern "C" {

int zkp_hip_verify_envelopes(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!off || !ok) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (null_blob_of_span(blob, off, n)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    return verify_call(n, [&](const std::vector<Device*>& shards, VerifyFanout& F) { return verify_envelopes_plan(n, blob, off, shards, F); },
                       [&](uint64_t lo, uint64_t m) { return verify_envelopes_host(m, blob, off + lo, expect ? expect + lo : nullptr, ok + lo); });
} ZKP_API_CATCH_INT

int zkp_hip_verify_envelopes_device(uint64_t n, const uint8_t* d_blob, const uint64_t* d_off, const uint8_t* d_expect, uint8_t* d_ok) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!d_blob || !d_off || !d_ok) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    Bind bind;
    if ((rc = bind.open())) return rc;
    return verify_envelopes_core(n, d_blob, d_off, d_expect, d_ok, nullptr);
} ZKP_API_CATCH_INT

}  // extern "C"
