// Sealing a list of composite proofs in one call (include/libzkp_hip_seal.h), host side and kernels of libzkp_hip (included by zkp_hip.hip
// behind batch_impl.inc: the batch form reads a proved batch's packed proofs where they lie).  Plan, steps and the division of work:
// composite_seal.h.

constexpr uint32_t SEAL_FRAME_TB = 256;         // four waves, one piece each
__global__ void __launch_bounds__(SEAL_FRAME_TB) k_comp_frame(uint8_t* out, const SealPiece* pieces, uint64_t npieces, const uint8_t* env, uint64_t env_bytes,
                                                              const uint8_t* meta, uint64_t meta_bytes) {
    const uint64_t p = (uint64_t)blockIdx.x * (SEAL_FRAME_TB / 64) + threadIdx.x / 64;
    if (p >= npieces) return;
    const SealPiece S = pieces[p];
    step_seal_frame(out, S, env, env, env + env_bytes, meta, meta, meta + meta_bytes, threadIdx.x & 63u, 64);
}
// One lane per sealed container, 64 consecutive lanes of the host's order (hashed length, descending) per wave, one wave per workgroup, as
// k_comp_digest has them; runs behind k_comp_frame on the same stream.
__global__ void __launch_bounds__(64) k_comp_seal(uint8_t* out, uint64_t bytes, const CompLane* lanes, const uint32_t* order, uint32_t m) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= m) return;
    const CompLane L = lanes[j];
    step_seal_digest(out, out, out + bytes, L, order);
}

namespace {

// The arguments both forms share, checked before anything is sized from them
int seal_check_args(uint64_t n, uint64_t n_env, const uint64_t* first, const uint8_t* meta_blob, const uint64_t* meta_off, const uint8_t* out, uint64_t out_cap,
                    const uint64_t* out_off, const uint8_t* status) {
    if (n > SEAL_MAX_ITEMS || n_env > SEAL_MAX_ITEMS) return fail(ZKP_HIP_E_ARGUMENT, "too many containers or envelopes: at most 4194304 of each per call (split the call)");
    if (!first || !out_off || !status || (!out && out_cap)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (first[n] > n_env) return fail(ZKP_HIP_E_ARGUMENT, "first[] leaves the envelope list");
    for (uint64_t i = 0; i < n; i++) if (first[i] > first[i + 1]) return fail(ZKP_HIP_E_ARGUMENT, "first[] must not decrease");
    if (meta_off) {
        for (uint64_t i = 0; i < n; i++) if (meta_off[i] > meta_off[i + 1]) return fail(ZKP_HIP_E_ARGUMENT, "meta_off[] must not decrease");
        if (null_blob_of_span(meta_blob, meta_off, n)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    }
    return 0;
}

// The plan of a call -> the caller's out_off and status; the required size against out_cap.  Nothing has been written to `out` yet.
int seal_publish(const SealPlan& P, uint64_t n, uint64_t out_cap, uint64_t* out_off, uint8_t* status) {
    memcpy(out_off, P.out_off.data(), 8 * (n + 1));
    memcpy(status, P.status.data(), n);
    if (P.out_off[n] > out_cap) return fail(ZKP_HIP_E_ARGUMENT, "output buffer too small (out_off[n] holds the required size)");
    return 0;
}

// The device half on the bound shard: frame, seal, one download.  d_env: the envelope bytes [env_lo, env_hi) of env_off's offsets where they lie
// on the device, or null: h_env[env_lo .. env_hi) is uploaded.  Returns 0, or 1 when some container was not sealed.
int seal_run(const SealPlan& P, uint64_t n, const uint64_t* env_off, const uint8_t* h_env, const uint8_t* d_env, uint64_t env_lo, uint64_t env_hi,
             const uint8_t* meta_blob, const uint64_t* meta_off, uint8_t* out) {
    Tally tally(dev().counters, FAM_SEAL);          // added when the call returns, whichever way
    tally[CTR_SEAL_CONTAINERS] = n; tally[CTR_SEAL_SEALED] = P.rec.size(); tally[CTR_SEAL_ENVELOPES] = P.envelopes; tally[CTR_SEAL_BYTES] = P.out_off[n];
    const int any = P.rec.size() != n ? 1 : 0;
    if (P.rec.empty()) return any;
    hipStream_t st = dev().stream;
    std::vector<SealPiece> pieces; std::vector<CompLane> lanes;
    seal_pieces(P, env_off, pieces, lanes);
    const uint64_t total = P.out_off[n], env_bytes = env_hi - env_lo;
    const uint64_t meta_lo = meta_off ? meta_off[0] : 0, meta_bytes = meta_off ? meta_off[n] - meta_off[0] : 0;
    for (SealPiece& S : pieces) S.src -= S.kind == SEAL_PIECE_META ? meta_lo : env_lo;          // sources relative to what is on the device
    DevScope mem;
    uint8_t *d_up = nullptr, *d_meta = nullptr, *d_out = nullptr; SealPiece* d_pieces = nullptr; CompLane* d_lanes = nullptr; uint32_t* d_order = nullptr;
    HIP_TRY(mem.alloc(&d_out, total)); HIP_TRY(mem.alloc(&d_pieces, sizeof(SealPiece) * pieces.size())); HIP_TRY(mem.alloc(&d_lanes, sizeof(CompLane) * lanes.size()));
    HIP_TRY(mem.alloc(&d_order, 4 * P.order.size())); HIP_TRY(mem.alloc(&d_meta, meta_bytes));
    if (!d_env) {
        HIP_TRY(mem.alloc(&d_up, env_bytes));
        if (env_bytes) HIP_TRY(hipMemcpyAsync(d_up, h_env + env_lo, env_bytes, hipMemcpyHostToDevice, st));
        d_env = d_up;
    }
    if (meta_bytes) HIP_TRY(hipMemcpyAsync(d_meta, meta_blob + meta_lo, meta_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_pieces, pieces.data(), sizeof(SealPiece) * pieces.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lanes, lanes.data(), sizeof(CompLane) * lanes.size(), hipMemcpyHostToDevice, st));
    if (!P.order.empty()) HIP_TRY(hipMemcpyAsync(d_order, P.order.data(), 4 * P.order.size(), hipMemcpyHostToDevice, st));
    const uint32_t per = SEAL_FRAME_TB / 64, L = (uint32_t)lanes.size();
    k_comp_frame<<<(uint32_t)((pieces.size() + per - 1) / per), SEAL_FRAME_TB, 0, st>>>(d_out, d_pieces, pieces.size(), d_env, env_bytes, d_meta, meta_bytes);
    HIP_TRY(hipGetLastError());
    k_comp_seal<<<(L + 63) / 64, 64, 0, st>>>(d_out, total, d_lanes, d_order, L);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, total, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the vectors above are read by the uploads until here)
    return any;
}

// The host-buffer form behind its argument checks, on the calling thread's shard.  env_code: null (judged here, from the envelopes' lengths and
// header bytes), or what the caller knows of its own envelopes.
int seal_host(uint64_t n, const uint8_t* env_blob, const uint64_t* env_off, uint64_t n_env, const uint8_t* env_code, const uint64_t* first, const uint8_t* meta_blob,
              const uint64_t* meta_off, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* status) {
    std::vector<uint8_t> judged;
    const uint64_t env_lo = n_env ? env_off[0] : 0, env_hi = n_env ? env_off[n_env] : 0;
    if (!env_code) {
        judged.resize(n_env);
        for (uint64_t e = 0; e < n_env; e++) judged[e] = seal_env_code(env_blob, env_off[e], env_off[e + 1], env_lo, env_hi);
        env_code = judged.data();
    }
    SealPlan P;
    seal_plan(n, env_off, env_code, first, meta_blob, meta_off, P);
    int rc = seal_publish(P, n, out_cap, out_off, status);
    if (rc) return rc;
    Bind bind;
    if ((rc = bind.open())) return rc;
    return seal_run(P, n, env_off, env_blob, nullptr, env_lo, env_hi >= env_lo ? env_hi : env_lo, meta_blob, meta_off, out);
}

}  // namespace

extern "C" {

int libzkp_seal_composites(uint64_t n, const uint8_t* env_blob, const uint64_t* env_off, uint64_t n_env, const uint64_t* first, const uint8_t* meta_blob,
                           const uint64_t* meta_off, uint8_t* out, uint64_t out_cap, uint64_t* out_off, uint8_t* status) try {
    if (n == 0) return 0;
    int rc = seal_check_args(n, n_env, first, meta_blob, meta_off, out, out_cap, out_off, status);
    if (rc) return rc;
    if (n_env && (!env_off || null_blob_of_span(env_blob, env_off, n_env))) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    return seal_host(n, env_blob, env_off, n_env, nullptr, first, meta_blob, meta_off, out, out_cap, out_off, status);
} ZKP_API_CATCH_INT

int libzkp_seal_batch(zkp_hip_batch* batch, uint64_t n, const uint64_t* first_op, const uint8_t* meta_blob, const uint64_t* meta_off, uint8_t* out, uint64_t out_cap,
                      uint64_t* out_off, uint8_t* status) try {
    if (n == 0) return 0;
    if (!batch) return fail(ZKP_HIP_E_ARGUMENT, "null batch");
    zkp_hip_batch& B = *batch;
    int rc = seal_check_args(n, B.n, first_op, meta_blob, meta_off, out, out_cap, out_off, status);
    if (rc) return rc;
    if ((rc = zkp_hip_batch_wait(batch))) return rc;
    if (B.shards.size() != 1) {
        // one container's ops lie on several GPUs (plan_shards cuts per variant): one fetch into a scratch buffer, then the host-buffer path
        std::vector<uint8_t> proofs(B.max_total ? B.max_total : 1), code(B.n);
        std::vector<uint64_t> off(B.n + 1); std::vector<int32_t> st(B.n);
        if ((rc = batch_fetch(B, proofs.data(), proofs.size(), off.data(), st.data())) < 0) return rc;
        for (uint64_t e = 0; e < B.n; e++) code[e] = st[e] == 0 ? SEAL_ENV_ACCEPTED : SEAL_ENV_FAILED_OP;
        return seal_host(n, proofs.data(), off.data(), B.n, code.data(), first_op, meta_blob, meta_off, out, out_cap, out_off, status);
    }
    // one shard: the packed proofs are framed and hashed where they lie (ShardPlan::d_out, in op order: gidx is 0 .. n - 1)
    return for_each_shard(B, [&](ShardPlan& S) -> int {
        int rcs = fetch_meta_shard(S);
        if (rcs < 0) return rcs;
        std::vector<uint8_t> code(S.n);
        for (uint32_t e = 0; e < S.n; e++) code[e] = S.h_status[e] == 0 ? SEAL_ENV_ACCEPTED : SEAL_ENV_FAILED_OP;
        SealPlan P;
        seal_plan(n, S.h_off.data(), code.data(), first_op, meta_blob, meta_off, P);
        if ((rcs = seal_publish(P, n, out_cap, out_off, status))) return rcs;
        return seal_run(P, n, S.h_off.data(), nullptr, S.d_out, 0, S.total, meta_blob, meta_off, out);
    });
} ZKP_API_CATCH_INT

int libzkp_seal_counters(double* ms, uint64_t* containers, uint64_t* sealed, uint64_t* envelopes, uint64_t* bytes, int reset) try {
    return read_counters(FAM_SEAL, ms, {containers, sealed, envelopes, bytes}, reset);
} ZKP_API_CATCH_INT

}  // extern "C"
