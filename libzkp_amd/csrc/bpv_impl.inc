// Range, threshold and consistency verification, host side of libzkp_hip (included by zkp_hip.hip): the core on device pointers
// (verify_bp_device), one slice of a host-buffer call (verify_bp_host) and the three entry points on verify_call.  Kernels: bpv_kernels.hip +
// the prover's MSM / partial-sum / encode kernels.
namespace {

struct VfyState { void* buf = nullptr; size_t cap = 0; LayoutSet set; bool ready = false; void* loc_buf = nullptr; size_t loc_cap = 0; };      // per shard (Device::vfy); loc_buf: localise_bp's, created by the first batch check that does not stand
VfyState& vfys() { if (!dev().vfy) dev().vfy = new VfyState(); return *dev().vfy; }

// What a call did after a batch check that did not stand (zkp_hip_bp_localise_counters): added to the shard's counters when the call
// returns, whichever way
struct BpLocaliseTally {
    Device& d; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    uint64_t segment_checks = 0, jobs_again = 0;
    explicit BpLocaliseTally(Device& dv) : d(dv) {}
    ~BpLocaliseTally() {
        Device::BpLocaliseCounter& C = d.bp_localise;
        C.failed_checks++; C.segment_checks += segment_checks; C.jobs_again += jobs_again;
        C.ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
};

// After a batch check of V's M jobs (n envelopes) that did not stand (W: the weighted view, Q: the check's point terms): one check per
// segment says where the bad jobs can be (bp_localise.h), only the suspect segments' jobs get the per-job pass, on compact arrays, and their
// encodings land in enc among zeros.  *done = false: nothing was decided here and the caller verifies the whole batch (localisation
// switched off, suspects in half of the batch, or -- against all odds -- no suspect at all).  job_base: the host's copy, or null.
int localise_bp(VfyState& S, const VfyView& V, const VfyView& W, const RlcView& Q, uint32_t n, uint32_t jobs_per, const uint32_t* job_base, uint32_t* enc,
                BpLocaliseTally& tally, bool* done) {
    *done = false;
    if (env_int("ZKP_HIP_BP_LOCALISE", 1) == 0) return 0;
    int rc;
    hipStream_t st = dev().stream;
    const uint32_t M = V.M;
    const int forced = env_int("ZKP_HIP_BP_LOCALISE_SEGMENT", 0);
    const BpSegments g = bp_loc_segments(n, forced > 0 ? (uint32_t)forced : 0u);
    const uint32_t count = g.count;
    size_t off = 0;
    auto sz = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    auto ensure = [&]() {           // (the buffer only grows; what it held is not needed across a growth)
        if (off <= S.loc_cap) return 0;
        if (S.loc_buf) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(S.loc_buf)); S.loc_buf = nullptr; S.loc_cap = 0; }
        HIP_TRY(hipMalloc(&S.loc_buf, off)); S.loc_cap = off;
        return 0;
    };
    // ---- the segment checks
    const DevLayout& Ds = pick_layout(S.set, count);
    const size_t s_dig = sz((size_t)NBASE * DIGW * 4 * count), s_part = sz((size_t)Ds.nchunks * GE_W * 4 * count), s_gen = sz((size_t)GE_W * 4 * count),
                 s_win = sz((size_t)count * RLC_NWIN * GE_W * 4), s_sus = sz(count), s_tcb = sz(16);
    if ((rc = ensure())) return rc;
    uint8_t* lb = (uint8_t*)S.loc_buf;
    BpLocView L{}; L.g = g; L.n = n; L.jobs_per = jobs_per; L.job_base = job_base ? V.job_base : nullptr; L.suspect = lb + s_sus; L.off = nullptr;
    const uint16_t tcbs[2] = {0, (uint16_t)Ds.nchunks};
    HIP_TRY(hipMemcpyAsync(lb + s_tcb, tcbs, sizeof tcbs, hipMemcpyHostToDevice, st));
    bpv_launch_seg_fixed_sum(W, L, (uint32_t*)(lb + s_dig), st);
    if ((rc = launch_msm(Ds, count, (uint32_t*)(lb + s_dig), (uint32_t*)(lb + s_part), st))) return rc;
    ReduceView Rs; Rs.rows = count; Rs.ntargets = 1; Rs.partial = (uint32_t*)(lb + s_part); Rs.target_chunk_begin = (const uint16_t*)(lb + s_tcb);
    Rs.enc = nullptr; Rs.out_off = nullptr; Rs.out = nullptr; Rs.corr = nullptr;
    launch_sum_ed(Rs, (uint32_t*)(lb + s_gen), st);
    bpv_launch_seg_points(Q, L, M, (uint32_t*)(lb + s_win), (const uint32_t*)(lb + s_gen), lb + s_sus, st);
    HIP_TRY(hipGetLastError());
    std::vector<uint8_t> suspect(count);
    HIP_TRY(hipMemcpyAsync(suspect.data(), lb + s_sus, count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tally.segment_checks += count;
    std::vector<uint32_t> offs((size_t)count + 1);
    const uint32_t Mc = bp_loc_offsets(g, n, jobs_per, job_base, suspect.data(), offs.data());
    if (Mc == 0 || bp_loc_whole_batch(Mc, M)) return 0;
    // ---- the per-job pass over the suspects' jobs, compacted
    const DevLayout& Dc = pick_layout(S.set, Mc);
    off = 0;
    const size_t c_sus = sz(count), c_off = sz(4ull * (count + 1)), c_tcb = sz(16),
                 c_poff = sz(8ull * Mc), c_voff = sz(8ull * Mc), c_kind = sz(Mc), c_lgn = sz(Mc), c_bad = sz(4ull * Mc),
                 c_pts = sz((size_t)VP_NUM * GE_W * 4 * Mc), c_scal = sz((size_t)VS_NUM * 32 * Mc),
                 c_zero0 = off, c_dig = sz((size_t)NBASE * DIGW * 4 * Mc), c_vs = sz((size_t)VP_NUM * 32 * Mc), c_zero1 = off,
                 c_part = sz((size_t)(Dc.nchunks + VP_NUM) * GE_W * 4 * Mc), c_sums = sz((size_t)GE_W * 4 * Mc), c_enc = sz((size_t)32 * Mc);
    if ((rc = ensure())) return rc;
    lb = (uint8_t*)S.loc_buf;
    HIP_TRY(hipMemcpyAsync(lb + c_sus, suspect.data(), count, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(lb + c_off, offs.data(), 4 * offs.size(), hipMemcpyHostToDevice, st));
    const uint16_t tcbc[2] = {0, (uint16_t)(Dc.nchunks + VP_NUM)};
    HIP_TRY(hipMemcpyAsync(lb + c_tcb, tcbc, sizeof tcbc, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(lb + c_zero0, 0, c_zero1 - c_zero0, st));
    L.suspect = lb + c_sus; L.off = (const uint32_t*)(lb + c_off);
    VfyView C = V;
    C.M = Mc; C.proof_off = (uint64_t*)(lb + c_poff); C.venc_off = (uint64_t*)(lb + c_voff); C.kind = lb + c_kind; C.lgn = lb + c_lgn; C.bad = (int32_t*)(lb + c_bad);
    C.pts = (uint32_t*)(lb + c_pts); C.scal = (uint32_t*)(lb + c_scal); C.digits = (uint32_t*)(lb + c_dig); C.vscal = (uint32_t*)(lb + c_vs);
    C.partial = (uint32_t*)(lb + c_part); C.var_chunk0 = Dc.nchunks; C.rho = nullptr; C.fterm = nullptr;
    bpv_launch_gather(V, L, C, st);
    bpv_launch_transcript(C, st);
    bpv_launch_scalars(C, st);
    if ((rc = launch_msm(Dc, Mc, C.digits, C.partial, st))) return rc;
    bpv_launch_varbase(C, st);
    ReduceView R; R.rows = Mc; R.ntargets = 1; R.partial = C.partial; R.target_chunk_begin = (const uint16_t*)(lb + c_tcb);
    R.enc = (uint32_t*)(lb + c_enc); R.out_off = nullptr; R.out = nullptr; R.corr = nullptr;
    uint32_t* sums = (uint32_t*)(lb + c_sums);
    launch_sum_ed(R, sums, st);
    k_encode<<<dim3((Mc + TW - 1) / TW, 1), TW, 0, st>>>(R, sums);
    HIP_TRY(hipMemsetAsync(enc, 0, (size_t)32 * M, st));
    bpv_launch_scatter(L, R.enc, Mc, enc, M, st);
    HIP_TRY(hipGetLastError());
    tally.jobs_again += Mc;
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
    const DevLayout& D = pick_layout(S.set, Mw);
    hipStream_t st = dev().stream;
    // workspace
    size_t off = 0;
    auto sz = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    const size_t o_jb = sz(4 * (n + 1)), o_eb = sz(4 * n),
                 o_poff = sz(8ull * Mw), o_voff = sz(8ull * Mw), o_kind = sz(Mw), o_lgn = sz(Mw), o_bad = sz(4ull * Mw),
                 o_pts = sz((size_t)VP_NUM * GE_W * 4 * Mw), o_scal = sz((size_t)VS_NUM * 32 * Mw),
                 o_zero0 = off,                                                                   // ---- zero-initialised from here
                 o_dig = sz((size_t)NBASE * DIGW * 4 * Mw), o_vs = sz((size_t)VP_NUM * 32 * Mw),
                 o_zero1 = off,
                 o_part = sz((size_t)(D.nchunks + VP_NUM) * GE_W * 4 * Mw), o_sums = sz((size_t)GE_W * 4 * Mw), o_enc = sz((size_t)32 * Mw), o_tcb = sz(16);
    // batch check (random linear combination, bp_verify.h RlcView): used when the batch is large enough to pay for it
    const bool batch_mode = M >= (uint32_t)env_int("ZKP_HIP_BATCH_VERIFY_MIN", (int)RLC_MIN_JOBS) && !getenv("ZKP_HIP_NO_BATCH_VERIFY");
    const uint32_t N = VP_NUM * Mw;
    const DevLayout& D1 = pick_layout(S.set, 1);
    size_t o_rho = 0, o_ft = 0, o_cnt = 0, o_rz1 = 0, o_nl = 0, o_vd = 0, o_stt = 0, o_cur = 0, o_srt = 0, o_bkt = 0, o_seg = 0, o_d1 = 0, o_p1 = 0, o_s1 = 0, o_res = 0, o_tcb1 = 0;
    if (batch_mode) {
        o_rho = sz(32ull * Mw);
        o_ft = sz((size_t)NBASE * 32 * Mw); o_cnt = sz((size_t)RLC_NWIN * (RLC_NBUCKET + 1) * 4); o_rz1 = off;      // [o_ft, o_rz1) zero-initialised
        o_nl = sz((size_t)N * RLC_NIELS_W * 4); o_vd = sz((size_t)RLC_NWIN * N * 2); o_stt = sz((size_t)RLC_NWIN * (RLC_NBUCKET + 2) * 4);
        o_cur = sz((size_t)RLC_NWIN * (RLC_NBUCKET + 1) * 4); o_srt = sz((size_t)RLC_NWIN * N * 4);
        o_bkt = sz((size_t)RLC_NWIN * RLC_NBUCKET * GE_W * 4); o_seg = sz((size_t)RLC_NWIN * RLC_NSEG * GE_W * 4);
        o_d1 = sz((size_t)NBASE * DIGW * 4); o_p1 = sz((size_t)D1.nchunks * GE_W * 4); o_s1 = sz((size_t)GE_W * 4); o_res = sz(64); o_tcb1 = sz(16);
    }
    if (off > S.cap) {
        if (S.buf) { HIP_TRY(hipDeviceSynchronize()); HIP_TRY(hipFree(S.buf)); S.buf = nullptr; S.cap = 0; }
        HIP_TRY(hipMalloc(&S.buf, off)); S.cap = off;
    }
    uint8_t* base = (uint8_t*)S.buf;
    if (consistency) HIP_TRY(hipMemcpyAsync(base + o_jb, job_base.data(), 4 * (n + 1), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(base + o_zero0, 0, o_zero1 - o_zero0, st));
    const uint16_t tcb[2] = {0, (uint16_t)(D.nchunks + VP_NUM)};       // one target: the fixed chunks and the 17 proof-point products
    HIP_TRY(hipMemcpyAsync(base + o_tcb, tcb, sizeof tcb, hipMemcpyHostToDevice, st));
    VfyView V{};
    V.M = M; V.in = d_proofs; V.proof_off = (uint64_t*)(base + o_poff); V.venc_off = (uint64_t*)(base + o_voff); V.kind = base + o_kind; V.lgn = base + o_lgn;
    V.bad = (int32_t*)(base + o_bad); V.pts = (uint32_t*)(base + o_pts); V.scal = (uint32_t*)(base + o_scal); V.digits = (uint32_t*)(base + o_dig);
    V.vscal = (uint32_t*)(base + o_vs); V.partial = (uint32_t*)(base + o_part); V.var_chunk0 = D.nchunks; V.table = dev().d_edg_table; V.wbits = dev().edg.wbits;
    V.job_base = (const uint32_t*)(base + o_jb); V.env_bad = (int32_t*)(base + o_eb);
    if (scheme == ZKP_HIP_OP_RANGE) bpv_launch_parse(V, (uint32_t)n, stride, d_lens, d_mins, d_maxs, st);
    else if (scheme == ZKP_HIP_OP_THRESHOLD) bpv_launch_parse_threshold(V, (uint32_t)n, stride, d_lens, d_mins, st);
    else bpv_launch_parse_consistency(V, (uint32_t)n, stride, d_lens, st);
    uint32_t* enc = (uint32_t*)(base + o_enc);
    bool accepted_as_a_batch = false, located = false;      // located: the check did not stand and localise_bp has put the suspects' encodings into enc
    std::unique_ptr<BpLocaliseTally> tally;                  // set once the batch check has not stood
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
        HIP_TRY(hipMemcpyAsync(base + o_rho, rho.data(), rho.size() * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(base + o_ft, 0, o_rz1 - o_ft, st));
        const uint16_t tcb1[2] = {0, (uint16_t)D1.nchunks};
        HIP_TRY(hipMemcpyAsync(base + o_tcb1, tcb1, sizeof tcb1, hipMemcpyHostToDevice, st));
        VfyView W = V; W.rho = (const uint32_t*)(base + o_rho); W.fterm = (uint32_t*)(base + o_ft);
        bpv_launch_transcript(W, st);
        bpv_launch_scalars(W, st);
        uint32_t* dig1 = (uint32_t*)(base + o_d1); uint32_t* part1 = (uint32_t*)(base + o_p1); uint32_t* sums1 = (uint32_t*)(base + o_s1);
        bpv_launch_rlc_fixed_sum(W, dig1, st);
        if ((rc = launch_msm(D1, 1, dig1, part1, st))) return rc;
        ReduceView R1; R1.rows = 1; R1.ntargets = 1; R1.partial = part1; R1.target_chunk_begin = (const uint16_t*)(base + o_tcb1);
        R1.enc = nullptr; R1.out_off = nullptr; R1.out = nullptr; R1.corr = nullptr;
        launch_sum_ed(R1, sums1, st);
        RlcView Q{};
        Q.N = VP_NUM * M; Q.niels = (uint32_t*)(base + o_nl); Q.dig = (int16_t*)(base + o_vd); Q.count = (uint32_t*)(base + o_cnt);
        Q.start = (uint32_t*)(base + o_stt); Q.cursor = (uint32_t*)(base + o_cur); Q.sorted = (uint32_t*)(base + o_srt);
        Q.bucket = (uint32_t*)(base + o_bkt); Q.seg = (uint32_t*)(base + o_seg); Q.fixed_sum = sums1; Q.result = (uint32_t*)(base + o_res);
        bpv_launch_rlc_points(W, Q, st);
        bpv_launch_rlc_sort(Q, st);
        bpv_launch_rlc_reduce(Q, st);
        HIP_TRY(hipGetLastError());
        uint32_t res[9] = {0};
        HIP_TRY(hipMemcpyAsync(res, base + o_res, sizeof res, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        accepted_as_a_batch = res[8] == 1;
        if (!accepted_as_a_batch && getenv("ZKP_HIP_BP_BATCH_VERIFY_ONLY"))                           // diagnostic: the verdict of this check, no per-job pass
            return fail(ZKP_HIP_E_RUNTIME, "Bulletproofs verification: the batch check did not stand and ZKP_HIP_BP_BATCH_VERIFY_ONLY is set");
        if (accepted_as_a_batch) HIP_TRY(hipMemsetAsync(enc, 0, (size_t)32 * Mw, st));                // every surviving job's sum is the identity
        else {
            tally.reset(new BpLocaliseTally(dev()));
            if ((rc = localise_bp(S, V, W, Q, (uint32_t)n, jobs_per, consistency ? job_base.data() : nullptr, enc, *tally, &located))) return rc;
            if (!located) {
                tally->jobs_again += M;
                HIP_TRY(hipMemsetAsync(base + o_zero0, 0, o_zero1 - o_zero0, st));                  // weighted scalars out, per-job path below
            }
        }
    }
    if (M && !accepted_as_a_batch && !located) {
        bpv_launch_transcript(V, st);
        bpv_launch_scalars(V, st);
        if ((rc = launch_msm(D, M, V.digits, V.partial, st))) return rc;
        bpv_launch_varbase(V, st);
        ReduceView R; R.rows = M; R.ntargets = 1; R.partial = V.partial; R.target_chunk_begin = (const uint16_t*)(base + o_tcb);
        R.enc = enc; R.out_off = nullptr; R.out = nullptr; R.corr = nullptr;
        uint32_t* sums = (uint32_t*)(base + o_sums);
        launch_sum_ed(R, sums, st);
        k_encode<<<dim3((M + TW - 1) / TW, 1), TW, 0, st>>>(R, sums);
    }
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
    if (dev().vfy->buf) (void)hipFree(dev().vfy->buf);
    if (dev().vfy->loc_buf) (void)hipFree(dev().vfy->loc_buf);
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

// accumulated over all shards (BpLocaliseTally); needs no device
int zkp_hip_bp_localise_counters(double* ms, uint64_t* failed_checks, uint64_t* segment_checks, uint64_t* jobs_again, int reset) try {
    std::vector<Device*> shards;
    { Registry& R = registry(); std::lock_guard<std::mutex> lk(R.mu); shards = R.shards; }
    Device::BpLocaliseCounter T;
    for (Device* d : shards) {
        std::lock_guard<std::mutex> dl(d->mu);
        Device::BpLocaliseCounter& C = d->bp_localise;
        T.ms += C.ms; T.failed_checks += C.failed_checks; T.segment_checks += C.segment_checks; T.jobs_again += C.jobs_again;
        if (reset) C = Device::BpLocaliseCounter();
    }
    if (ms) *ms = T.ms;
    if (failed_checks) *failed_checks = T.failed_checks;
    if (segment_checks) *segment_checks = T.segment_checks;
    if (jobs_again) *jobs_again = T.jobs_again;
    return 0;
} ZKP_API_CATCH_INT

}  // extern "C"
