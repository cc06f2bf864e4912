// The mixed verifier (include/libzkp_hip_verify.h), host side and glue kernels of libzkp_hip (included by zkp_hip.hip).  Steps: venv_steps.h.
// The verifiers themselves are the cores of the per-scheme calls (verify_bp_device, verify_g16_core, verify_stark_device), called unchanged,
// one after the other on the shard's stream in self_check_shard's order.
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

// The call on device pointers, on the bound shard: classification, the records back, the plan, the rows, the cores, the verdicts into d_ok
// (device, n bytes); ok_host (may be null) also receives them before the wait that ends the call.
int verify_envelopes_core(uint64_t n, const uint8_t* d_blob, const uint64_t* d_off, const uint8_t* d_expect, uint8_t* d_ok, uint8_t* ok_host) {
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t st = dev().stream;
    DevScope mem;
    struct Quiesce { bool armed = false; ~Quiesce() { if (armed) (void)hipDeviceSynchronize(); } } quiesce;      // as verify_g16_host: the chains' side streams
    VenvRecord* d_rec = nullptr;
    HIP_TRY(mem.alloc(&d_rec, sizeof(VenvRecord) * n));
    const uint32_t lane_blocks = (uint32_t)((n + 255) / 256);
    k_venv_classify<<<lane_blocks, 256, 0, st>>>(d_blob, d_off, d_expect, n, d_rec);
    HIP_TRY(hipGetLastError());
    std::vector<VenvRecord> rec(n);
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
        int rc;
        auto rows_of = [&](uint32_t k) { return (const uint8_t*)(V.rows + P.base[k]); };
        auto lens = [&](uint32_t k) { return (const uint32_t*)(V.row_len + P.row0[k]); };
        auto p0 = [&](uint32_t k) { return (const uint64_t*)(V.row_p0 + P.row0[k]); };
        auto oks = [&](uint32_t k) { return V.row_ok + P.row0[k]; };
        const uint32_t RG = ZKP_HIP_OP_RANGE, TH = ZKP_HIP_OP_THRESHOLD, CO = ZKP_HIP_OP_CONSISTENCY, EQ = ZKP_HIP_OP_EQUALITY, ME = ZKP_HIP_OP_MEMBERSHIP, IM = ZKP_HIP_OP_IMPROVEMENT;
        if (P.rows[RG]) { passes++; if ((rc = verify_bp_device(1, P.rows[RG], rows_of(RG), P.stride[RG], lens(RG), p0(RG), V.row_p1 + P.row0[RG], oks(RG), nullptr, nullptr))) return rc; }
        if (P.rows[TH]) { passes++; if ((rc = verify_bp_device(3, P.rows[TH], rows_of(TH), P.stride[TH], lens(TH), p0(TH), nullptr, oks(TH), nullptr, nullptr))) return rc; }
        if (P.rows[CO]) {
            std::vector<uint32_t> jobs; jobs.reserve(P.rows[CO]);          // in row order = envelope order
            for (uint64_t i = 0; i < n; i++) if (rec[i].scheme == CO) jobs.push_back(rec[i].jobs);
            passes++;
            if ((rc = verify_bp_device(6, P.rows[CO], rows_of(CO), P.stride[CO], lens(CO), nullptr, nullptr, oks(CO), jobs.data(), nullptr))) return rc;
        }
        if (P.rows[EQ] || P.rows[ME]) {
            quiesce.armed = true;
            std::vector<uint8_t> h_ok(P.rows[EQ] > P.rows[ME] ? P.rows[EQ] : P.rows[ME]);      // the batch check's verdicts, read by its localisation pass
            if (P.rows[EQ]) { passes++; if ((rc = verify_g16_core(G16_EQUALITY, P.rows[EQ], rows_of(EQ), P.stride[EQ], lens(EQ), oks(EQ), h_ok.data(), mem, hipSuccess))) return rc; }
            if (P.rows[ME]) { passes++; if ((rc = verify_g16_core(G16_MEMBERSHIP, P.rows[ME], rows_of(ME), P.stride[ME], lens(ME), oks(ME), h_ok.data(), mem, hipSuccess))) return rc; }
            quiesce.armed = false;
        }
        if (P.rows[IM]) { passes++; if ((rc = verify_stark_device(P.rows[IM], rows_of(IM), P.stride[IM], lens(IM), p0(IM), oks(IM)))) return rc; }
    }
    k_venv_apply<<<lane_blocks, 256, 0, st>>>(V, d_ok);
    HIP_TRY(hipGetLastError());
    if (ok_host) HIP_TRY(hipMemcpyAsync(ok_host, d_ok, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    Device::VerifyMixedStats& C = dev().verify_mixed;
    C.passes += passes; C.rows += P.live;
    C.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

// The host-buffer form on the bound shard, for the m envelopes whose offsets start at `off` (m + 1 entries): one upload of the bytes they
// span, their offsets re-based to that span, and `expect`; then the core.
int verify_envelopes_host(uint64_t m, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok) {
    if (off[m] < off[0]) { memset(ok, 0, m); return 0; }          // no envelope lies inside an empty span
    const uint64_t first = off[0], bytes = off[m] - first;
    // (an offset below `first` wraps to a value beyond `bytes`, so the classification rejects its envelope as outside the span)
    std::vector<uint64_t> rel(m + 1);
    for (uint64_t i = 0; i <= m; i++) rel[i] = off[i] - first;
    hipStream_t st = dev().stream;
    DevScope mem;
    uint8_t *d_blob = nullptr, *d_expect = nullptr, *d_ok = nullptr; uint64_t* d_off = nullptr;
    HIP_TRY(mem.alloc(&d_blob, bytes)); HIP_TRY(mem.alloc(&d_off, 8 * (m + 1))); HIP_TRY(mem.alloc(&d_ok, m));
    if (expect) HIP_TRY(mem.alloc(&d_expect, m));
    if (bytes) HIP_TRY(hipMemcpyAsync(d_blob, blob + first, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_off, rel.data(), 8 * (m + 1), hipMemcpyHostToDevice, st));
    if (expect) HIP_TRY(hipMemcpyAsync(d_expect, expect, m, hipMemcpyHostToDevice, st));
    return verify_envelopes_core(m, d_blob, d_off, d_expect, d_ok, ok);
}

// The host-buffer form over every registered shard when the plan of verify_shards.h says so (*fanned): contiguous slices through
// verify_envelopes_host.  Weights: ve_weight.  Minimum slice: the larger of the two batch-check thresholds in force.  Shards that lack a
// usable key of a Groth16 circuit whose scheme byte occurs in the list take no part.
int verify_envelopes_fanned(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok, bool* fanned) {
    *fanned = false;
    const std::vector<Device*> shards = verify_fanout_candidates();
    if (shards.empty()) return 0;
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
    std::vector<uint64_t> prefix(n + 1);
    vs_prefix(n, weights.data(), prefix.data());
    std::vector<uint8_t> holds(shards.size());
    for (size_t k = 0; k < shards.size(); k++) {
        std::lock_guard<std::mutex> lk(shards[k]->mu);
        bool has = true;
        for (int kind : {G16_EQUALITY, G16_MEMBERSHIP}) if (need[kind]) has = has && shards[k]->g16 && shards[k]->g16->key[kind].vk_ready;
        holds[k] = has;
    }
    const int bp_min = env_int("ZKP_HIP_BATCH_VERIFY_MIN", (int)RLC_MIN_JOBS), g16_min = g16_rlc_min();
    const uint64_t a = bp_min > 0 ? (uint64_t)bp_min : RLC_MIN_JOBS, b = g16_min > 0 ? (uint64_t)g16_min : 8193u;
    return verify_fan_out(shards, holds.data(), n, prefix.data(), 0u, a > b ? a : b,
                          [&](uint64_t lo, uint64_t m) { return verify_envelopes_host(m, blob, off + lo, expect ? expect + lo : nullptr, ok + lo); }, fanned);
}

}  // namespace

extern "C" {

int zkp_hip_verify_envelopes(uint64_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* expect, uint8_t* ok) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!off || !ok) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (!blob && off[n] > off[0]) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    bool fanned = false;
    rc = verify_envelopes_fanned(n, blob, off, expect, ok, &fanned);
    if (rc || fanned) return rc;
    Bind bind;
    if ((rc = bind.open())) return rc;
    return verify_envelopes_host(n, blob, off, expect, ok);
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
