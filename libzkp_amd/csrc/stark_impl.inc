// Improvement proofs (STARK) host side of libzkp_hip (included by zkp_hip.hip): the constants, the provers, the verifier's core on device
// pointers (verify_stark_device), one slice of a host-buffer call (verify_stark_host) and its entry point on verify_call.  Kernel: stark_kernels.hip.
namespace {

struct StarkState { StarkConst* consts = nullptr; };       // per shard (Device::stark)
#define g_stark_const (dev().stark->consts)
int ensure_stark_constants() {
    if (!dev().stark) dev().stark = new StarkState();
    if (g_stark_const) return 0;
    StarkConst* h = new StarkConst();
    stark_build_constants(*h);                       // domain tables: a few hundred field operations, once per process
    StarkConst* d = nullptr;
    hipError_t e = hipMalloc(&d, sizeof(StarkConst));
    if (e == hipSuccess) e = hipMemcpy(d, h, sizeof(StarkConst), hipMemcpyHostToDevice);
    delete h;
    if (e != hipSuccess) { if (d) (void)hipFree(d); return fail(ZKP_HIP_E_RUNTIME, hipGetErrorString(e)); }
    g_stark_const = d;
    return 0;
}

// The verifier on device pointers: n envelopes at `stride` bytes in d_in, d_len[i] bytes used, verdicts into d_ok (device), enqueued on the
// shard's stream (the host-buffer entry point uploads and calls this; the batch self-check calls it on the arena's rows)
int verify_stark_device(uint64_t n, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, const uint64_t* d_old, uint8_t* d_ok) {
    int rc = ensure_stark_constants();
    if (rc) return rc;
    stark_launch_verify(d_in, stride, d_len, d_old, (uint32_t)n, g_stark_const, d_ok, dev().stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

// one slice of a host-buffer call on the bound shard: upload, the core above, verdicts back
int verify_stark_host(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* old_values, uint8_t* ok) {
    int rc = ensure_stark_constants();
    if (rc) return rc;
    EnvelopeUpload up;
    if ((rc = up.open(n, proofs, stride, lens, old_values)) || (rc = verify_stark_device(n, up.d_in, stride, up.d_len, up.d_p0, up.d_ok))) return rc;
    HIP_TRY(hipMemcpyAsync(ok, up.d_ok, n, hipMemcpyDeviceToHost, dev().stream));
    HIP_TRY(hipStreamSynchronize(dev().stream));
    return 0;
}
// The minimum slice of a fanned-out call.  The STARK verifier has no batch check; what it needs is what fills a GPU -- the envelopes (one per
// lane, 64 per workgroup) of the k_stark_verify workgroups the caller's GPU holds at once, asked once per shard under a short Bind of its own
// that is gone before anything is posted: a slice that does not fill a GPU cannot finish sooner on two.  An occupancy query that fails keeps
// the call on the caller's shard (no slice is large enough).  Not asked when ZKP_HIP_VERIFY_SHARD_MIN replaces the minimum anyway.
int stark_min_slice(uint64_t* min_jobs) {
    *min_jobs = 0;
    if (env_int("ZKP_HIP_VERIFY_SHARD_MIN", 0) > 0) return 0;
    Bind bind; int rc = bind.open();
    if (rc) return rc;
    if (!dev().stark_verify_resident) dev().stark_verify_resident = (uint64_t)stark_verify_blocks_per_cu() * (uint64_t)dev().num_cu * 64u;
    *min_jobs = dev().stark_verify_resident ? dev().stark_verify_resident : ~0ull;
    return 0;
}

void stark_release_all() {
    if (!dev().stark) return;
    if (dev().stark->consts) (void)hipFree(dev().stark->consts);
    delete dev().stark; dev().stark = nullptr;
}

}  // namespace

extern "C" {

uint32_t zkp_hip_improvement_max_bytes(void) { return STARK_MAX_ENVELOPE; }      // (a constant: nothing to guard)

int zkp_hip_prove_improvement_batch_device(uint64_t n, const uint64_t* d_old, const uint64_t* d_new, uint8_t* d_out, uint64_t stride,
                                           uint32_t* d_out_len, void* stream) try {
    if (n == 0) return 0;
    Bind bind; int rc = host_args(n, {d_old, d_new, d_out, d_out_len}, nullptr, stride, STARK_MAX_ENVELOPE, "stride must be at least zkp_hip_improvement_max_bytes()");
    if (rc || (rc = bind.open()) || (rc = ensure_stark_constants())) return rc;
    hipStream_t st = stream ? (hipStream_t)stream : dev().stream;
    stark_launch_prove(d_old, d_new, (uint32_t)n, g_stark_const, d_out, stride, d_out_len, st);
    HIP_TRY(hipGetLastError());
    if (!stream) HIP_TRY(hipStreamSynchronize(st));
    return 0;
} ZKP_API_CATCH_INT

int zkp_hip_prove_improvement_batch(uint64_t n, const uint64_t* old_values, const uint64_t* new_values, uint8_t* out, uint64_t stride,
                                    uint32_t* out_len, int32_t* status) try {
    if (n == 0) return 0;
    Bind bind; int rc = host_args(n, {old_values, new_values, out, out_len, status}, nullptr, stride, STARK_MAX_ENVELOPE,
                                  "stride must be at least zkp_hip_improvement_max_bytes()");
    if (rc || (rc = bind.open()) || (rc = ensure_stark_constants())) return rc;
    hipStream_t st = dev().stream;
    uint64_t *d_old = nullptr, *d_new = nullptr; uint8_t* d_out = nullptr; uint32_t* d_len = nullptr;
    DevScope mem;
    HIP_TRY(mem.alloc(&d_old, 8 * n)); HIP_TRY(mem.alloc(&d_new, 8 * n)); HIP_TRY(mem.alloc(&d_out, stride * n)); HIP_TRY(mem.alloc(&d_len, 4 * n));
    HIP_TRY(hipMemcpyAsync(d_old, old_values, 8 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_new, new_values, 8 * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_out, 0, stride * n, st));
    stark_launch_prove(d_old, d_new, (uint32_t)n, g_stark_const, d_out, stride, d_len, st);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, stride * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(out_len, d_len, 4 * n, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ZKP_HIP_E_RUNTIME, hipGetErrorString(e));
    int any = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!improvement_ok(old_values[i], new_values[i])) { status[i] = ZKP_HIP_INVALID_INPUT; out_len[i] = 0; any = 1; }
        else if (out_len[i] == 0) { status[i] = ZKP_HIP_PROOF_GENERATION_FAILED; any = 1; }
        else status[i] = ZKP_HIP_OK;
    }
    return any;
} ZKP_API_CATCH_INT

int zkp_hip_verify_improvement_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* old_values, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, old_values, ok}, stride);
    if (rc) return rc;
    return verify_call(n, [&](const std::vector<Device*>&, VerifyFanout& F) { return stark_min_slice(&F.min_jobs); },
                       [&](uint64_t lo, uint64_t m) { return verify_stark_host(m, proofs + stride * lo, stride, lens + lo, old_values + lo, ok + lo); });
} ZKP_API_CATCH_INT

}  // extern "C"
