// Envelopes against the caller's statements (include/libzkp_hip_statements.h), host side and kernels of libzkp_hip (included by zkp_hip.hip).
// Steps: vst_steps.h.  Stream order of one call or slice: k_vst_classify, the two bind kernels over the live envelopes of their scheme, then
// the mixed verifier's spine from the record copy on (venv_impl.inc: verify_records_core), closed by k_vst_apply in place of k_venv_apply.

// One lane per envelope.  A live equality / membership envelope is appended to its scheme's index list (cnt[0] / cnt[1] entries; any order:
// every entry is bound on its own).  The lists hold as many entries as the call has ops of that kind, and a live envelope has its op's kind.
__global__ void __launch_bounds__(256) k_vst_classify(const uint8_t* blob, const uint64_t* off, const zkp_hip_op* ops, uint64_t n_lists, uint64_t n, VenvRecord* rec,
                                                      uint32_t* eq_idx, uint32_t* mem_idx, uint32_t* cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const VenvRecord r = step_vst_classify(blob, off, ops, n_lists, n, i);
    rec[i] = r;
    if (r.scheme == ZKP_HIP_OP_EQUALITY) eq_idx[atomicAdd(&cnt[0], 1u)] = (uint32_t)i;
    else if (r.scheme == ZKP_HIP_OP_MEMBERSHIP) mem_idx[atomicAdd(&cnt[1], 1u)] = (uint32_t)i;
}
// One lane per live equality envelope, one wave per workgroup (a lane runs the 110 rounds of the MiMC chain on its own: many short
// workgroups spread a small list over the CUs); the grid strides over the list.
constexpr uint32_t VST_EQ_TB = 64;
__global__ void __launch_bounds__(VST_EQ_TB) k_vst_bind_equality(const uint8_t* blob, const uint64_t* off, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists,
                                                                 const uint32_t* mimc_c, const uint32_t* eq_idx, const uint32_t* cnt, VenvRecord* rec) {
    const uint32_t live = cnt[0];
    for (uint32_t t = blockIdx.x * VST_EQ_TB + threadIdx.x; t < live; t += gridDim.x * VST_EQ_TB) {
        const uint64_t i = eq_idx[t];
        if (!step_vst_bind_equality(blob, off, ops, lists, n_lists, mimc_c, i)) { rec[i].scheme = 0; rec[i].reserved = ZKP_STMT_STATEMENT; }
    }
}
// One wave per live membership envelope, four waves per workgroup; the waves stride over the list.  Lane k holds embedded element k and
// statement element k in registers; lane j's pair reaches every lane through v_readlane with j in a scalar register.
constexpr uint32_t VST_MEM_TB = 256;
__device__ __forceinline__ uint64_t vst_readlane_u64(uint64_t x, uint32_t lane) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, (int)lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), (int)lane);
    return ((uint64_t)hi << 32) | lo;
}
__global__ void __launch_bounds__(VST_MEM_TB) k_vst_bind_membership(const uint8_t* blob, const uint64_t* off, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists,
                                                                    const uint32_t* mem_idx, const uint32_t* cnt, VenvRecord* rec) {
    const uint32_t lane = threadIdx.x & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t live = cnt[1], waves = gridDim.x * (VST_MEM_TB / 64);
    for (uint32_t t = blockIdx.x * (VST_MEM_TB / 64) + wave; t < live; t += waves) {
        const uint64_t i = mem_idx[t];
        const zkp_hip_op o = ops[i];
        const uint32_t count = (uint32_t)__builtin_amdgcn_readfirstlane((int)o.count);
        const VstMemLane mine = step_vst_mem_load(blob, off, o, lists, n_lists, i, lane);
        const bool vote = step_vst_mem_count(mine, lane, count, [&](uint32_t j) { return VstMemLane{vst_readlane_u64(mine.emb, j), vst_readlane_u64(mine.stmt, j)}; });
        if (!__all(vote) && lane == 0) { rec[i].scheme = 0; rec[i].reserved = ZKP_STMT_STATEMENT; }
    }
}
__global__ void __launch_bounds__(256) k_vst_apply(VenvView V, uint8_t* ok, uint8_t* why) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V.n) return;
    uint8_t w;
    ok[i] = step_vst_apply(V, i, w);
    if (why) why[i] = w;
}

namespace {

// The call on device pointers, on the bound shard.  max_eq / max_mem: how many of the n ops are equality / membership ops at the most (the
// host-buffer form counts them, the device form knows only n): the capacity of the index lists and the bound of the bind kernels' grids.  A
// bind kernel is not launched when its bound is 0.  ok_host (may be null) receives the verdicts, why_host (may be null) the reasons.
int verify_statements_core(uint64_t n, const zkp_hip_op* d_ops, const uint64_t* d_lists, uint64_t n_lists, const uint8_t* d_blob, const uint64_t* d_off,
                           uint8_t* d_ok, uint8_t* ok_host, uint8_t* d_why, uint8_t* why_host, uint64_t max_eq, uint64_t max_mem) {
    Tally tally(dev().counters, FAM_STATEMENTS);          // added when the call or slice returns, whichever way
    tally[CTR_STMT_ENVELOPES] = n;
    hipStream_t st = dev().stream;
    int rc;
    if (max_eq && (rc = ensure_mimc_dev())) return rc;
    DevScope mem;
    VenvRecord* d_rec = nullptr; uint32_t *d_eq_idx = nullptr, *d_mem_idx = nullptr, *d_cnt = nullptr;
    HIP_TRY(mem.alloc(&d_rec, sizeof(VenvRecord) * n)); HIP_TRY(mem.alloc(&d_eq_idx, 4 * max_eq)); HIP_TRY(mem.alloc(&d_mem_idx, 4 * max_mem)); HIP_TRY(mem.alloc(&d_cnt, 8));
    if (why_host && !d_why) HIP_TRY(mem.alloc(&d_why, n));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, 8, st));
    const uint32_t lane_blocks = (uint32_t)((n + 255) / 256);
    k_vst_classify<<<lane_blocks, 256, 0, st>>>(d_blob, d_off, d_ops, n_lists, n, d_rec, d_eq_idx, d_mem_idx, d_cnt);
    HIP_TRY(hipGetLastError());
    const uint64_t resident = 8ull * (uint64_t)dev().num_cu;          // workgroups beyond what the GPU holds at once only queue: the grids stride
    if (max_eq) {
        const uint64_t blocks = std::min<uint64_t>((max_eq + VST_EQ_TB - 1) / VST_EQ_TB, resident);
        k_vst_bind_equality<<<(uint32_t)blocks, VST_EQ_TB, 0, st>>>(d_blob, d_off, d_ops, d_lists, n_lists, g16s().mimc_dev, d_eq_idx, d_cnt, d_rec);
        HIP_TRY(hipGetLastError());
    }
    if (max_mem) {
        const uint64_t blocks = std::min<uint64_t>((max_mem + VST_MEM_TB / 64 - 1) / (VST_MEM_TB / 64), resident);
        k_vst_bind_membership<<<(uint32_t)blocks, VST_MEM_TB, 0, st>>>(d_blob, d_off, d_ops, d_lists, n_lists, d_mem_idx, d_cnt, d_rec);
        HIP_TRY(hipGetLastError());
    }
    std::vector<VenvRecord> rec;
    uint64_t passes = 0, live = 0;
    rc = verify_records_core(n, d_blob, d_off, d_rec, rec, d_ok, ok_host, &passes, &live, [&](const VenvView& V) {
        k_vst_apply<<<lane_blocks, 256, 0, st>>>(V, d_ok, d_why);
        HIP_TRY(hipGetLastError());
        if (why_host) HIP_TRY(hipMemcpyAsync(why_host, d_why, n, hipMemcpyDeviceToHost, st));
        return 0;
    });
    for (const VenvRecord& r : rec) {
        if (r.scheme) continue;
        tally[r.reserved == ZKP_STMT_STATEMENT ? CTR_STMT_REFUSED_STATEMENT : CTR_STMT_REFUSED_ENVELOPE]++;
    }
    if (rc) return rc;
    if (ok_host) for (uint64_t i = 0; i < n; i++) if (rec[i].scheme && !ok_host[i]) tally[CTR_STMT_REFUSED_PROOF]++;
    return 0;
}

// The host-buffer form on the bound shard, for the m ops at `ops` and the m envelopes whose offsets start at `off` (m + 1 entries): the
// envelopes' span (SpanUpload), the ops re-based to the span of lists they name, and that span; then the core.
int verify_statements_host(uint64_t m, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists, const uint8_t* blob, const uint64_t* off, uint8_t* ok, uint8_t* why) {
    SpanUpload up; bool empty;
    int rc = up.open(m, blob, off, &empty);
    if (rc) return rc;
    if (empty) {
        memset(ok, 0, m);
        if (why) memset(why, ZKP_STMT_ENVELOPE, m);
        Tally tally(dev().counters, FAM_STATEMENTS); tally[CTR_STMT_ENVELOPES] = m; tally[CTR_STMT_REFUSED_ENVELOPE] = m;
        return 0;
    }
    std::vector<zkp_hip_op> sliced(m);
    const VstListSpan span = vst_slice_ops(m, ops, n_lists, sliced.data());
    uint64_t max_eq = 0, max_mem = 0;
    for (const zkp_hip_op& o : sliced) { max_eq += op_kind(o) == ZKP_HIP_OP_EQUALITY; max_mem += op_kind(o) == ZKP_HIP_OP_MEMBERSHIP; }
    hipStream_t st = dev().stream;
    uint64_t* d_lists = nullptr; zkp_hip_op* d_ops = nullptr;
    HIP_TRY(up.mem.alloc(&d_ops, sizeof(zkp_hip_op) * m)); HIP_TRY(up.mem.alloc(&d_lists, 8 * span.count));
    HIP_TRY(hipMemcpyAsync(d_ops, sliced.data(), sizeof(zkp_hip_op) * m, hipMemcpyHostToDevice, st));
    if (span.count) HIP_TRY(hipMemcpyAsync(d_lists, lists + span.lo, 8 * span.count, hipMemcpyHostToDevice, st));
    return verify_statements_core(m, d_ops, d_lists, span.count, up.d_blob, up.d_off, up.d_ok, ok, nullptr, why, max_eq, max_mem);
}

// The fan-out data of the host-buffer form (verify_call): the mixed verifier's weights (ve_weight) through list_fanout (venv_impl.inc), but for
// the keys: a shard takes part when it holds a usable key of every Groth16 circuit of which the list has ops.
int verify_statements_plan(uint64_t n, const zkp_hip_op* ops, const uint8_t* blob, const uint64_t* off, const std::vector<Device*>& shards, VerifyFanout& F) {
    std::vector<uint32_t> weights(n);
    bool need[2] = {false, false};
    for (uint64_t i = 0; i < n; i++) {
        weights[i] = ve_weight(blob, off, n, i);
        if (op_kind(ops[i]) == ZKP_HIP_OP_EQUALITY) need[G16_EQUALITY] = true;
        if (op_kind(ops[i]) == ZKP_HIP_OP_MEMBERSHIP) need[G16_MEMBERSHIP] = true;
    }
    return list_fanout(weights, need, shards, F);
}

}  // namespace

extern "C" {

int zkp_stmt_verify(uint64_t n, const zkp_hip_op* ops, const uint64_t* lists, uint64_t n_lists, const uint8_t* blob, const uint64_t* off, uint8_t* ok, uint8_t* why) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!ops || !off || !ok || (!lists && n_lists)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (null_blob_of_span(blob, off, n)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    return verify_call(n, [&](const std::vector<Device*>& shards, VerifyFanout& F) { return verify_statements_plan(n, ops, blob, off, shards, F); },
                       [&](uint64_t lo, uint64_t m) { return verify_statements_host(m, ops + lo, lists, n_lists, blob, off + lo, ok + lo, why ? why + lo : nullptr); });
} ZKP_API_CATCH_INT

int zkp_stmt_verify_device(uint64_t n, const zkp_hip_op* d_ops, const uint64_t* d_lists, uint64_t n_lists, const uint8_t* d_blob, const uint64_t* d_off,
                           uint8_t* d_ok, uint8_t* d_why) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!d_ops || !d_blob || !d_off || !d_ok || (!d_lists && n_lists)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    Bind bind;
    if ((rc = bind.open())) return rc;
    return verify_statements_core(n, d_ops, d_lists, n_lists, d_blob, d_off, d_ok, nullptr, d_why, nullptr, n, n);
} ZKP_API_CATCH_INT

int zkp_stmt_counters(double* ms, uint64_t* envelopes, uint64_t* refused_envelope, uint64_t* refused_statement, uint64_t* refused_proof, int reset) try {
    return read_counters(FAM_STATEMENTS, ms, {envelopes, refused_envelope, refused_statement, refused_proof}, reset);
} ZKP_API_CATCH_INT

}  // extern "C"
