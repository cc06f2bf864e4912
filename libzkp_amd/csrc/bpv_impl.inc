// Range, threshold and consistency verification, host side of libzkp_hip (included by zkp_hip.hip): the core on device pointers
// (verify_bp_device) with what follows a batch check that does not stand (localise_bp), both on the workspace plan of bpv_plan.h and on one
// per-job pass (per_job_pass) and one fixed-base sum (fixed_base_sum); one slice of a host-buffer call (verify_bp_host), the three entry
// points on verify_call and the localisation counters.  Kernels: bpv_kernels.hip + the prover's MSM / partial-sum / encode kernels.
#include "bpv_plan.h"
namespace {

struct VfyState { GrowBuf buf, loc; LayoutSet set; bool ready = false; };      // per shard (Device::vfy); buf: the batch block, loc: localise_bp's two shapes (bpv_plan.h), created by the first batch check that does not stand
VfyState& vfys() { if (!dev().vfy) dev().vfy = new VfyState(); return *dev().vfy; }

// The per-job pass over the C.M jobs of a view bound to the job arrays J at `base` (D: the layout J was planned for; digits and vscal zeroed,
// J.chunk_table at J.tcb): every job's folded equation as one multiscalar sum -- the generator terms through the fixed-base MSM, the proof
// points one lane each -- and its ristretto encoding into the block's enc rows, 32 zero bytes iff the job verifies
int per_job_pass(const VfyView& C, const DevLayout& D, uint8_t* base, const BpvJobArrays& J, hipStream_t st) {
    bpv_launch_transcript(C, st);
    bpv_launch_scalars(C, st);
    if (int rc = launch_msm(D, C.M, C.digits, C.partial, st)) return rc;
    bpv_launch_varbase(C, st);
    ReduceView R = reduce_view(D, C.M, C.partial, nullptr); R.target_chunk_begin = (const uint16_t*)(base + J.tcb); R.enc = (uint32_t*)(base + J.enc);      // (its own table: J.chunk_table)
    uint32_t* sums = (uint32_t*)(base + J.sums);
    launch_sum_ed(R, sums, st);
    k_encode<<<dim3((C.M + TW - 1) / TW, 1), TW, 0, st>>>(R, sums);
    return 0;
}
// sums[r] = the generators' sum under row r of `rows` rows of fixed-base digits: the MSM's chunk partials, summed over D's own chunk table
// (targets_verify is one target: {0, nchunks}, as the prover's launch_reduce reads it)
int fixed_base_sum(const DevLayout& D, uint32_t rows, const uint32_t* digits, uint32_t* partial, uint32_t* sums, hipStream_t st) {
    if (D.ntargets != 1) return fail(ZKP_HIP_E_RUNTIME, "Bulletproofs verification: the generator layout has more than one target");
    if (int rc = launch_msm(D, rows, digits, partial, st)) return rc;
    launch_sum_ed(reduce_view(D, rows, partial, nullptr), sums, st);
    return 0;
}

// After a batch check of V's M jobs (n envelopes) that did not stand (W: the weighted view, Q: the check's point terms): one check per
// segment says where the bad jobs can be (bp_localise.h), only the suspect segments' jobs get the per-job pass, on compact arrays, and their
// encodings land in enc among zeros.  *done = false: nothing was decided here and the caller verifies the whole batch (localisation
// switched off, suspects in half of the batch, or -- against all odds -- no suspect at all).  job_base: the host's copy, or null.
int localise_bp(VfyState& S, const VfyView& V, const VfyView& W, const RlcView& Q, uint32_t n, uint32_t jobs_per, const uint32_t* job_base, uint32_t* enc,
                Tally& tally, bool* done) {
    *done = false;
    if (env_int("ZKP_HIP_BP_LOCALISE", 1) == 0) return 0;
    int rc;
    hipStream_t st = dev().stream;
    const uint32_t M = V.M;
    const int forced = env_int("ZKP_HIP_BP_LOCALISE_SEGMENT", 0);
    const BpSegments g = bp_loc_segments(n, forced > 0 ? (uint32_t)forced : 0u);
    const uint32_t count = g.count;
    // ---- the segment checks
    const DevLayout& Ds = pick_layout(S.set, count);
    const BpvSegmentPlan Ps = bpv_plan_segments(count, Ds.nchunks);
    uint8_t*& lb = S.loc.p;                                         // the block in use: another one after a growth
    if ((rc = S.loc.reserve(Ps.total))) return rc;
    BpLocView L{}; L.g = g; L.n = n; L.jobs_per = jobs_per; L.job_base = job_base ? V.job_base : nullptr; L.suspect = lb + Ps.suspect; L.off = nullptr;
    bpv_launch_seg_fixed_sum(W, L, (uint32_t*)(lb + Ps.dig), st);
    if ((rc = fixed_base_sum(Ds, count, (uint32_t*)(lb + Ps.dig), (uint32_t*)(lb + Ps.part), (uint32_t*)(lb + Ps.gen), st))) return rc;
    bpv_launch_seg_points(Q, L, M, (uint32_t*)(lb + Ps.win), (const uint32_t*)(lb + Ps.gen), lb + Ps.suspect, st);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> suspect(count);
    HIP_TRY(hipMemcpyAsync(suspect.data(), lb + Ps.suspect, count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tally[CTR_BP_SEGMENT_CHECKS] += count;
    std::vector<uint32_t> offs((size_t)count + 1);
    const uint32_t Mc = bp_loc_offsets(g, n, jobs_per, job_base, suspect.data(), offs.data());
    if (Mc == 0 || bp_loc_whole_batch(Mc, M)) return 0;
    // ---- the per-job pass over the suspects' jobs, compacted
    const DevLayout& Dc = pick_layout(S.set, Mc);
    const BpvCompactPlan Pc = bpv_plan_compact(count, Mc, Dc.nchunks);
    if ((rc = S.loc.reserve(Pc.total))) return rc;                 // (maybe a new block, and the second shape in either case: the suspect bytes go up again)
    HIP_TRY(hipMemcpyAsync(lb + Pc.suspect, suspect.data(), count, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lb + Pc.off, offs.data(), 4 * offs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lb + Pc.J.tcb, Pc.J.chunk_table, sizeof Pc.J.chunk_table, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(lb + Pc.J.zero0, 0, Pc.J.zero1 - Pc.J.zero0, st));
    L.suspect = lb + Pc.suspect; L.off = (const uint32_t*)(lb + Pc.off);
    VfyView C = V; C.M = Mc; C.rho = nullptr; C.fterm = nullptr;
    bpv_bind_jobs(C, lb, Pc.J);
    bpv_launch_gather(V, L, C, st);
    if ((rc = per_job_pass(C, Dc, lb, Pc.J, st))) return rc;
    HIP_TRY(hipMemsetAsync(enc, 0, (size_t)32 * M, st));
    bpv_launch_scatter(L, (const uint32_t*)(lb + Pc.J.enc), Mc, enc, M, st);
    HIP_TRY(hipGetLastError());
    tally[CTR_BP_JOBS_AGAIN] += Mc;
    *done = true;
    return 0;
}

// The verifier on device pointers: n envelopes at `stride` bytes in d_proofs, d_lens[i] bytes used, verdicts into d_ok (device); waits for them.
// scheme: ZKP_HIP_OP_RANGE (bounds = d_mins, d_maxs; two jobs per envelope), ZKP_HIP_OP_THRESHOLD (bounds = thresholds, d_maxs unused; one job)
// or ZKP_HIP_OP_CONSISTENCY (no bounds; job_counts[i] jobs for envelope i, a host array from the caller -- the host entry point counts k - 1
// from each envelope's own k field, the batch self-check knows its ops' list lengths; the device step rejects an envelope whose k disagrees).
// The batch check (k_rlc_*), what follows one that does not stand (localise_bp, or the per-job pass over everything) and their switches
// are in here, so every caller gets the same verdicts.
// ok_host (may be null): the verdicts are also copied there before the one wait that ends the call.
int verify_bp_device(int scheme, uint64_t n, const uint8_t* d_proofs, uint64_t stride, const uint32_t* d_lens, const uint64_t* d_mins, const uint64_t* d_maxs, uint8_t* d_ok,
                     const uint32_t* job_counts, uint8_t* ok_host) {
    int rc;
    if ((rc = ensure_bp())) return rc;
    VfyState& S = vfys();
    if (!S.ready) {
        if ((rc = upload_set(S.set, targets_verify((uint8_t)dev().edg.nwin)))) return rc;      // round 4: the prover's tables in HBM (edg.h)
        S.ready = true;
    }
    const bool consistency = scheme == ZKP_HIP_OP_CONSISTENCY;
    const uint32_t jobs_per = scheme == ZKP_HIP_OP_RANGE ? 2u : 1u;
    std::vector<uint32_t> job_base;
    if (consistency) {
        job_base.resize(n + 1); job_base[0] = 0;
        for (uint64_t i = 0; i < n; i++) job_base[i + 1] = job_base[i] + job_counts[i];
    }
    const uint32_t M = consistency ? job_base[n] : (uint32_t)(jobs_per * n), Mw = M ? M : 1;
    const DevLayout &D = pick_layout(S.set, Mw), &D1 = pick_layout(S.set, 1);
    hipStream_t st = dev().stream;
    // batch check (random linear combination, bp_verify.h RlcView): used when the batch is large enough to pay for it
    const bool batch_mode = M >= (uint32_t)env_int("ZKP_HIP_BATCH_VERIFY_MIN", (int)RLC_MIN_JOBS) && !getenv("ZKP_HIP_NO_BATCH_VERIFY");
    const BpvBatchPlan P = bpv_plan_batch(n, Mw, D.nchunks, batch_mode, D1.nchunks);
    if ((rc = S.buf.reserve(P.total))) return rc;
    uint8_t* base = S.buf.p;
    if (consistency) HIP_TRY(hipMemcpyAsync(base + P.job_base, job_base.data(), 4 * (n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(base + P.J.zero0, 0, P.J.zero1 - P.J.zero0, st));
    HIP_TRY(hipMemcpyAsync(base + P.J.tcb, P.J.chunk_table, sizeof P.J.chunk_table, hipMemcpyHostToDevice, st));
    VfyView V{}; V.M = M; V.in = d_proofs; V.table = dev().d_edg_table; V.wbits = dev().edg.wbits; V.job_base = (const uint32_t*)(base + P.job_base); V.env_bad = (int32_t*)(base + P.env_bad);
    bpv_bind_jobs(V, base, P.J);
    if (scheme == ZKP_HIP_OP_RANGE) bpv_launch_parse(V, (uint32_t)n, stride, d_lens, d_mins, d_maxs, st);
    else if (scheme == ZKP_HIP_OP_THRESHOLD) bpv_launch_parse_threshold(V, (uint32_t)n, stride, d_lens, d_mins, st);
    else bpv_launch_parse_consistency(V, (uint32_t)n, stride, d_lens, st);
    uint32_t* enc = (uint32_t*)(base + P.J.enc);
    bool accepted_as_a_batch = false, located = false;      // located: the check did not stand and localise_bp has put the suspects' encodings into enc
    std::unique_ptr<Tally> tally;                            // zkp_hip_bp_localise_counters: made once the batch check has not stood, added when the call returns, whichever way
    if (M) bpv_launch_decode(V, st);
    if (M && batch_mode) {
        // One check for the whole batch: sum_j rho_j (job j's combination) == 0 with fresh 128-bit weights from the OS, as
        // upstream's batch verification does.  It passes iff every job that survived parsing / decoding verifies (up to 2^-128);
        // if it fails, segment checks (localise_bp) say where the bad envelopes can be and the per-job path says which they are.
        std::vector<uint8_t> rnd; if ((rc = fresh_seeds(rnd, (M + 1) / 2))) return rc;               // 16 bytes per job
        std::vector<uint32_t> rho((size_t)8 * M);
        for (uint32_t j = 0; j < M; j++) {
            sc raw = sc_zero(); memcpy(raw.v, rnd.data() + 16ull * j, 16);
            if ((raw.v[0] | raw.v[1] | raw.v[2] | raw.v[3]) == 0) raw.v[0] = 1;
            const sc m = sc_from_raw256(raw);
            for (int k = 0; k < 8; k++) rho[(size_t)k * M + j] = m.v[k];
        }
        HIP_TRY(hipMemcpyAsync(base + P.rho, rho.data(), rho.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(base + P.fterm, 0, P.rzero1 - P.fterm, st));
        VfyView W = V; W.rho = (const uint32_t*)(base + P.rho); W.fterm = (uint32_t*)(base + P.fterm);
        bpv_launch_transcript(W, st);
        bpv_launch_scalars(W, st);
        uint32_t* dig1 = (uint32_t*)(base + P.dig1); uint32_t* sums1 = (uint32_t*)(base + P.sum1);
        bpv_launch_rlc_fixed_sum(W, dig1, st);
        if ((rc = fixed_base_sum(D1, 1, dig1, (uint32_t*)(base + P.part1), sums1, st))) return rc;
        RlcView Q{}; Q.N = VP_NUM * M; Q.niels = (uint32_t*)(base + P.niels); Q.dig = (int16_t*)(base + P.dig); Q.count = (uint32_t*)(base + P.count);
        Q.start = (uint32_t*)(base + P.start); Q.cursor = (uint32_t*)(base + P.cursor); Q.sorted = (uint32_t*)(base + P.sorted);
        Q.bucket = (uint32_t*)(base + P.bucket); Q.seg = (uint32_t*)(base + P.seg); Q.fixed_sum = sums1; Q.result = (uint32_t*)(base + P.result);
        bpv_launch_rlc_points(W, Q, st);
        bpv_launch_rlc_sort(Q, st);
        bpv_launch_rlc_reduce(Q, st);
        HIP_TRY(hipGetLastError());
        uint32_t res[9] = {0};
        HIP_TRY(hipMemcpyAsync(res, base + P.result, sizeof res, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        accepted_as_a_batch = res[8] == 1;
        if (!accepted_as_a_batch && getenv("ZKP_HIP_BP_BATCH_VERIFY_ONLY"))                           // diagnostic: the verdict of this check, no per-job pass
            return fail(ZKP_HIP_E_RUNTIME, "Bulletproofs verification: the batch check did not stand and ZKP_HIP_BP_BATCH_VERIFY_ONLY is set");
        if (accepted_as_a_batch) HIP_TRY(hipMemsetAsync(enc, 0, (size_t)32 * Mw, st));                // every surviving job's sum is the identity
        else {
            tally = bp_localise_tally(dev().counters);
            if ((rc = localise_bp(S, V, W, Q, (uint32_t)n, jobs_per, consistency ? job_base.data() : nullptr, enc, *tally, &located))) return rc;
            if (!located) {
                (*tally)[CTR_BP_JOBS_AGAIN] += M;
                HIP_TRY(hipMemsetAsync(base + P.J.zero0, 0, P.J.zero1 - P.J.zero0, st));          // weighted scalars out, per-job path below
            }
        }
    }
    if (M && !accepted_as_a_batch && !located && (rc = per_job_pass(V, D, base, P.J, st))) return rc;
    if (consistency) bpv_launch_final_ranges(V, enc, (uint32_t)n, d_ok, st);
    else bpv_launch_final(V, enc, (uint32_t)n, d_ok, jobs_per, st);
    HIP_TRY(hipGetLastError());
    if (ok_host) HIP_TRY(hipMemcpyAsync(ok_host, d_ok, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// jobs of each consistency envelope, read from its own k field (k - 1 range proofs; 0 for an envelope the device step will reject): the rule
// is ve_consistency_jobs (venv_steps.h), shared with the mixed verifier's classification kernel
std::vector<uint32_t> consistency_job_counts(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens) {
    std::vector<uint32_t> job_counts(n);
    for (uint64_t i = 0; i < n; i++) job_counts[i] = lens[i] <= stride ? ve_consistency_jobs(proofs + stride * i, lens[i]) : 0u;
    return job_counts;
}
// the batch-check threshold in force (ZKP_HIP_BATCH_VERIFY_MIN, read on every call) as the minimum slice of a fanned-out call
uint64_t bp_min_slice() { const int v = env_int("ZKP_HIP_BATCH_VERIFY_MIN", (int)RLC_MIN_JOBS); return v > 0 ? (uint64_t)v : RLC_MIN_JOBS; }

// one slice of a host-buffer call on the bound shard: the consistency job counts from the envelopes' own k fields, the upload, the core above
int verify_bp_host(int scheme, uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* mins, const uint64_t* maxs, uint8_t* ok) {
    std::vector<uint32_t> job_counts;
    if (scheme == ZKP_HIP_OP_CONSISTENCY) job_counts = consistency_job_counts(n, proofs, stride, lens);
    EnvelopeUpload up;
    int rc = up.open(n, proofs, stride, lens, mins, maxs);
    if (rc) return rc;
    return verify_bp_device(scheme, n, up.d_in, stride, up.d_len, up.d_p0, up.d_p1, up.d_ok, job_counts.data(), ok);
}
// The three host-buffer entry points after their argument checks.  Spread over the shards (verify_call), every slice draws its own weights
// and makes its own batch check.  Weights: two jobs per range envelope, one per threshold envelope, a consistency envelope's own job count.
int verify_bp_call(int scheme, uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* mins, const uint64_t* maxs, uint8_t* ok) {
    return verify_call(n,
        [&](const std::vector<Device*>&, VerifyFanout& F) {
            if (scheme == ZKP_HIP_OP_CONSISTENCY) { F.prefix.resize(n + 1); vs_prefix(n, consistency_job_counts(n, proofs, stride, lens).data(), F.prefix.data()); }
            F.unit = scheme == ZKP_HIP_OP_RANGE ? 2u : 1u; F.min_jobs = bp_min_slice();
            return 0;
        },
        [&](uint64_t lo, uint64_t m) { return verify_bp_host(scheme, m, proofs + stride * lo, stride, lens + lo, mins ? mins + lo : nullptr, maxs ? maxs + lo : nullptr, ok + lo); });
}

void bpv_release_all() {
    if (!dev().vfy) return;
    dev().vfy->buf.release(); dev().vfy->loc.release();
    free_set(dev().vfy->set);
    delete dev().vfy; dev().vfy = nullptr;
}

}  // namespace

extern "C" {

int zkp_hip_verify_range_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* mins, const uint64_t* maxs, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, mins, maxs, ok}, stride);
    return rc ? rc : verify_bp_call(ZKP_HIP_OP_RANGE, n, proofs, stride, lens, mins, maxs, ok);
} ZKP_API_CATCH_INT

int zkp_hip_verify_threshold_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, const uint64_t* thresholds, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, thresholds, ok}, stride);
    return rc ? rc : verify_bp_call(ZKP_HIP_OP_THRESHOLD, n, proofs, stride, lens, thresholds, nullptr, ok);
} ZKP_API_CATCH_INT

int zkp_hip_verify_consistency_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, ok}, stride);
    return rc ? rc : verify_bp_call(ZKP_HIP_OP_CONSISTENCY, n, proofs, stride, lens, nullptr, nullptr, ok);
} ZKP_API_CATCH_INT

// accumulated over all shards; needs no device
int zkp_hip_bp_localise_counters(double* ms, uint64_t* failed_checks, uint64_t* segment_checks, uint64_t* jobs_again, int reset) try {
    return read_counters(FAM_BP_LOCALISE, ms, {failed_checks, segment_checks, jobs_again}, reset);
} ZKP_API_CATCH_INT

}  // extern "C"
