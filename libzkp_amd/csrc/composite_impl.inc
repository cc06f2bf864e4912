// One verify call for a list of composite proofs (include/libzkp_hip_composites.h), host side and kernels of libzkp_hip (included by
// zkp_hip.hip).  Steps and the division of work: composite_steps.h.  The cryptographic side is the mixed verifier's core, called unchanged
// on the packed inner envelopes of every container that stands (venv_impl.inc: verify_envelopes_core).

// One lane per container, 64 consecutive lanes of the host's order (hashed length, descending) per wave, one wave per workgroup: the lanes
// of a wave finish together, and a wave of short containers does not wait for a long one.
__global__ void __launch_bounds__(64) k_comp_digest(const uint8_t* blob, uint64_t bytes, const CompLane* lanes, const uint32_t* order, uint32_t m, uint8_t* verdict) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j >= m) return;
    const CompLane L = lanes[j];
    verdict[j] = step_comp_digest(blob, blob, blob + bytes, L, order, nullptr) ? 1 : 0;
}
constexpr uint32_t COMP_PACK_TB = 256;          // four waves, one envelope each
__global__ void __launch_bounds__(COMP_PACK_TB) k_comp_pack(uint8_t* packed, const uint64_t* poff, const uint8_t* blob, uint64_t bytes, const uint64_t* src, uint64_t envelopes) {
    const uint64_t e = (uint64_t)blockIdx.x * (COMP_PACK_TB / 64) + threadIdx.x / 64;
    if (e < envelopes) step_comp_pack(packed, poff, blob, src, blob, blob + bytes, e, threadIdx.x & 63u, 64);
}
__global__ void __launch_bounds__(256) k_comp_fold(uint8_t* status, const uint8_t* ok, const uint64_t* env0, uint64_t m) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (c < m) status[c] = step_comp_fold(status[c], ok, env0, c);
}

namespace {

constexpr uint64_t COMP_MAX_ENVELOPES = 1ull << 22;

// One call: the caller's buffers and what the walk over all of its containers left (made once, before any device work: the envelope
// bound, the fan-out weights and every slice read it)
struct CompCall {
    uint64_t n; const uint8_t* blob; const uint64_t* off; uint32_t flags; uint8_t* status;
    std::vector<CompWalk> walk; std::vector<uint32_t> order;
    uint64_t envelopes = 0;
};

// The containers [lo, lo + m) of the call on the bound shard: digests first, then the inner envelopes of the containers that stand through
// the mixed verifier's core, then the fold.
int composites_slice(const CompCall& K, uint64_t lo, uint64_t m) {
    Tally tally(dev().counters, FAM_COMPOSITES);          // added when the slice returns, whichever way
    tally[CTR_COMP_COMPOSITES] = m;
    hipStream_t st = dev().stream;
    uint8_t* status = K.status + lo;
    std::vector<uint32_t> good; good.reserve(m);          // slice indices of the well-formed containers
    uint64_t span_lo = ~0ull, span_hi = 0;
    for (uint64_t i = 0; i < m; i++) {
        status[i] = CP_MALFORMED;
        if (!K.walk[lo + i].ok) continue;
        good.push_back((uint32_t)i);
        span_lo = std::min(span_lo, K.off[lo + i]); span_hi = std::max(span_hi, K.off[lo + i + 1]);
    }
    tally[CTR_COMP_MALFORMED] = m - good.size();
    if (good.empty()) return 0;
    // lanes: longest stream first
    std::vector<uint32_t> by_len(good);
    std::stable_sort(by_len.begin(), by_len.end(), [&](uint32_t a, uint32_t b) { return K.walk[lo + a].hashed > K.walk[lo + b].hashed; });
    const uint64_t order_lo = K.walk[lo].order0, order_hi = lo + m < K.n ? K.walk[lo + m].order0 : K.order.size();
    const uint32_t L = (uint32_t)by_len.size();
    std::vector<CompLane> lanes(L);
    for (uint32_t j = 0; j < L; j++) {
        const uint64_t i = lo + by_len[j];
        lanes[j] = comp_lane(K.walk[i], K.off[i] - span_lo, K.walk[i].order0 - order_lo, by_len[j]);
    }
    const uint64_t bytes = span_hi - span_lo;
    DevScope mem;
    uint8_t *d_blob = nullptr, *d_verdict = nullptr; CompLane* d_lanes = nullptr; uint32_t* d_order = nullptr;
    HIP_TRY(mem.alloc(&d_blob, bytes)); HIP_TRY(mem.alloc(&d_lanes, sizeof(CompLane) * L)); HIP_TRY(mem.alloc(&d_order, 4 * (order_hi - order_lo))); HIP_TRY(mem.alloc(&d_verdict, L));
    HIP_TRY(hipMemcpyAsync(d_blob, K.blob + span_lo, bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_lanes, lanes.data(), sizeof(CompLane) * L, hipMemcpyHostToDevice, st));
    if (order_hi > order_lo) HIP_TRY(hipMemcpyAsync(d_order, K.order.data() + order_lo, 4 * (order_hi - order_lo), hipMemcpyHostToDevice, st));
    // ZKP_HIP_COMPOSITES_DIGEST_LOG=<file> (read on every call): the digest kernel between two events, one line per slice
    const char* log_path = getenv("ZKP_HIP_COMPOSITES_DIGEST_LOG");
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (log_path && *log_path) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventRecord(e0, st)); }
    k_comp_digest<<<(L + 63) / 64, 64, 0, st>>>(d_blob, bytes, d_lanes, d_order, L, d_verdict);
    HIP_TRY(hipGetLastError());
    if (e0) HIP_TRY(hipEventRecord(e1, st));
    std::vector<uint8_t> verdict(L);
    HIP_TRY(hipMemcpyAsync(verdict.data(), d_verdict, L, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (e0) {
        float ms = 0; uint64_t hashed = 0;
        HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
        for (uint32_t j = 0; j < L; j++) hashed += lanes[j].hashed;
        if (FILE* f = fopen(log_path, "a")) { fprintf(f, "{\"containers\": %u, \"hashed_bytes\": %llu, \"digest_kernel_ms\": %.6f}\n", L, (unsigned long long)hashed, (double)ms); fclose(f); }
    }
    uint64_t standing = 0, envelopes = 0, packed_bytes = 0;
    for (uint32_t j = 0; j < L; j++) {
        if (!verdict[j]) continue;
        status[by_len[j]] = CP_ACCEPTED; standing++;
        envelopes += K.walk[lo + by_len[j]].nproofs; packed_bytes += K.walk[lo + by_len[j]].proof_bytes;
    }
    tally[CTR_COMP_MALFORMED] = m - standing;
    if ((K.flags & ZKP_HIP_COMPOSITES_INTEGRITY_ONLY) || envelopes == 0) return 0;
    // the inner envelopes of the containers that stand, in container order: where each lies, where it goes
    std::vector<uint64_t> src(envelopes), poff(envelopes + 1), env0(m + 1);
    uint64_t e = 0, at_packed = 0;
    for (uint64_t i = 0; i < m; i++) {
        env0[i] = e;
        if (status[i] != CP_ACCEPTED) continue;
        comp_each_envelope(K.blob, K.off[lo + i], K.walk[lo + i].nproofs, [&](uint64_t at, uint64_t len) { src[e] = at - span_lo; poff[e] = at_packed; e++; at_packed += len; });
    }
    env0[m] = e; poff[e] = at_packed;
    tally[CTR_COMP_ENVELOPES] = envelopes;
    uint8_t *d_packed = nullptr, *d_ok = nullptr, *d_status = nullptr; uint64_t *d_src = nullptr, *d_poff = nullptr, *d_env0 = nullptr;
    HIP_TRY(mem.alloc(&d_packed, packed_bytes)); HIP_TRY(mem.alloc(&d_ok, envelopes)); HIP_TRY(mem.alloc(&d_status, m));
    HIP_TRY(mem.alloc(&d_src, 8 * envelopes)); HIP_TRY(mem.alloc(&d_poff, 8 * (envelopes + 1))); HIP_TRY(mem.alloc(&d_env0, 8 * (m + 1)));
    HIP_TRY(hipMemcpyAsync(d_src, src.data(), 8 * envelopes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_poff, poff.data(), 8 * (envelopes + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_env0, env0.data(), 8 * (m + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_status, status, m, hipMemcpyHostToDevice, st));
    k_comp_pack<<<(uint32_t)((envelopes + COMP_PACK_TB / 64 - 1) / (COMP_PACK_TB / 64)), COMP_PACK_TB, 0, st>>>(d_packed, d_poff, d_blob, bytes, d_src, envelopes);
    HIP_TRY(hipGetLastError());
    const int rc = verify_envelopes_core(envelopes, d_packed, d_poff, nullptr, d_ok, nullptr);
    if (rc) return rc;
    k_comp_fold<<<(uint32_t)((m + 255) / 256), 256, 0, st>>>(d_status, d_ok, d_env0, m);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(status, d_status, m, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// The fan-out data (verify_call) through list_fanout (venv_impl.inc).  A container weighs what its envelopes weigh (ve_scheme_weight), at least 1;
// a key is needed when its scheme byte occurs in a well-formed container.
int composites_plan(const CompCall& K, const std::vector<Device*>& shards, VerifyFanout& F) {
    std::vector<uint32_t> weights(K.n, 1);
    bool need[2] = {false, false};
    if (!(K.flags & ZKP_HIP_COMPOSITES_INTEGRITY_ONLY)) for (uint64_t i = 0; i < K.n; i++) {
        if (!K.walk[i].ok) continue;
        uint64_t w = 0;
        comp_each_envelope(K.blob, K.off[i], K.walk[i].nproofs, [&](uint64_t at, uint64_t len) {
            const uint8_t s = K.blob[at + 1];
            w += ve_scheme_weight(s, K.blob + at, len);
            if (s == ZKP_HIP_OP_EQUALITY) need[G16_EQUALITY] = true;
            if (s == ZKP_HIP_OP_MEMBERSHIP) need[G16_MEMBERSHIP] = true;
        });
        weights[i] = (uint32_t)std::min<uint64_t>(w, 0xffffffffu);
    }
    return list_fanout(weights, need, shards, F);
}

}  // namespace

extern "C" {

int zkp_hip_verify_composites(uint64_t n, const uint8_t* blob, const uint64_t* off, uint32_t flags, uint8_t* status) try {
    if (n == 0) return 0;
    int rc = check_batch_size(n);
    if (rc) return rc;
    if (!off || !status) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (null_blob_of_span(blob, off, n)) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (flags & ~ZKP_HIP_COMPOSITES_INTEGRITY_ONLY) return fail(ZKP_HIP_E_ARGUMENT, "unknown flag");
    CompCall K{n, blob, off, flags, status, {}, {}};
    K.walk.reserve(n);
    for (uint64_t i = 0; i < n; i++) {
        K.walk.push_back(comp_walk(blob, off[i], off[i + 1], off[0], off[n], K.order));
        if (K.walk.back().ok) K.envelopes += K.walk.back().nproofs;
    }
    if (K.envelopes > COMP_MAX_ENVELOPES) return fail(ZKP_HIP_E_ARGUMENT, "too many inner envelopes: at most 4194304 per call (split the call)");
    return verify_call(n, [&](const std::vector<Device*>& shards, VerifyFanout& F) { return composites_plan(K, shards, F); },
                       [&](uint64_t lo, uint64_t m) { return composites_slice(K, lo, m); });
} ZKP_API_CATCH_INT

int zkp_hip_composites_counters(double* ms, uint64_t* composites, uint64_t* malformed, uint64_t* envelopes, int reset) try {
    return read_counters(FAM_COMPOSITES, ms, {composites, malformed, envelopes}, reset);
} ZKP_API_CATCH_INT

}  // extern "C"
