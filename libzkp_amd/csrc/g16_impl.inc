// Groth16 / BN254 host side of libzkp_hip (included by zkp_hip.hip): R1CS of libzkp's two circuits, ark-serialize
// proving-key loader, fixed-base table construction, the batched prove pipeline, and the verifier: its core on device pointers
// (verify_g16_core), one slice of a host-buffer call (verify_g16_host) and the two entry points on verify_call.  Kernels: g16_kernels.hip,
// g16_verify_kernels.hip, fq2vm_kernels.hip.

// ================================================================================================ host
namespace {

// ---- device-resident key + circuit
struct G16Key {
    bool loaded = false;                                // a PROVING key is loaded (circuit, MSM tables, layouts); a verifier-only key has vk_ready alone
    uint32_t n_inst = 0, n_wit = 0, nv = 0, n_rows = 0, m = 0, logm = 0;
    G16Circuit C{};
    std::vector<void*> allocs;
    uint32_t *table_g1 = nullptr, *table_g2 = nullptr;
    G16Radix rx = g16_radix(G16_WBITS_DEFAULT);        // radix of this key's tables, chosen when the key was loaded
    int shared_tables = -1;                             // index into the process-wide table registry (shards of one GPU share a key's tables)
    uint64_t table_bytes = 0;                           // HBM held by this key's two MSM tables (shared by the shards of one GPU)
    // chunkings of the two key-point MSMs, built on demand per chunk count (the grid is matched to the batch size at run time)
    struct Chunking { DevLayout lay; const uint32_t* corr = nullptr; const uint16_t* scal = nullptr; };   // scal: digit row of each slot of this layout
    std::vector<SlotList> targets_g1, targets_g2;              // G1: A' | S (the slots A and B1 share, g16_share.h; may be empty) | B1' | C
    std::vector<uint16_t> hscal_g1, hscal_g2;  // digit row per key point (host copy; the layouts carry their own device copy)
    std::map<uint64_t, Chunking> lays_g1, lays_g2;            // key = part << 32 | chunk count
    uint64_t win_g1 = 0, win_g2 = 0;          // windows (= mixed additions) per proof
    const uint32_t *init_g1 = nullptr, *init_g2 = nullptr;
    G16Vk vk{}; bool vk_ready = false;        // the verifying key (loaded alone, or the one that leads the proving key file): all the verification entry points read
    uint64_t vk_table_bytes = 0;              // HBM held by vk.ic_table
    uint8_t digest[32] = {}; bool have_digest = false;      // SHA-256 of the key bytes a successful load read (zkpkeycheck_key: is this the loaded key?)
    bool verifier_only() const { return vk_ready && !loaded; }
    const uint32_t *vm_kconst = nullptr, *vm_lines = nullptr;      // the Fq2 machine's Miller value of (beta, -alpha) and line table of gamma, delta (fq2vm.h)
};
// per-shard Groth16 state (Device::g16): both circuits' keys, the MiMC constants, one workspace + side stream per circuit
// so that equality and membership batches of one mixed batch run concurrently on their own streams
struct G16Run {
    GrowBuf buf; hipStream_t side = nullptr, side2 = nullptr; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // recorded behind the final assembly of the last run on this workspace: the next run (possibly on another stream -- a per-variant
    // call while an asynchronous batch is in flight) waits for it before it overwrites z / digits / partials
    hipEvent_t last = nullptr; bool used = false;
};
struct G16State {
    G16Key key[2];
    uint32_t* mimc_dev = nullptr;
    G16Run run[2][2];          // [circuit][lane]: two batches may be in flight on a shard (batch_impl.inc)
    bool attr_set = false;
    G16VmTables vm;            // micro-operation tables of the verifier's Fq2 machine (uploaded on first use)
};
G16State& g16s() {
    if (!dev().g16) dev().g16 = new G16State();
    return *dev().g16;
}

template <class Tv> int dev_upload(G16Key& K, Tv** dst, const std::vector<typename std::remove_const<Tv>::type>& src) {
    typename std::remove_const<Tv>::type* p = nullptr;
    HIP_TRY(hipMalloc(&p, src.size() * sizeof(src[0]) + 16));
    if (!src.empty()) HIP_TRY(hipMemcpy(p, src.data(), src.size() * sizeof(src[0]), hipMemcpyHostToDevice));
    K.allocs.push_back(p); *dst = p;
    return 0;
}

int upload_circuit(G16Key& K, const HostR1CS& cs) {
    const HostCircuitTables T = build_circuit_tables(cs);
    K.n_inst = T.n_inst; K.n_wit = T.n_wit; K.nv = T.nv; K.n_rows = T.n_rows; K.m = T.m; K.logm = T.logm;
    G16Circuit& C = K.C;
    C.n_rows = T.n_rows; C.m = T.m; C.logm = T.logm;
    int rc;
    if ((rc = dev_upload(K, &C.a_ptr, T.ptr[0])) || (rc = dev_upload(K, &C.a_col, T.col[0])) || (rc = dev_upload(K, &C.a_coef, T.coef[0]))) return rc;
    if ((rc = dev_upload(K, &C.b_ptr, T.ptr[1])) || (rc = dev_upload(K, &C.b_col, T.col[1])) || (rc = dev_upload(K, &C.b_coef, T.coef[1]))) return rc;
    if ((rc = dev_upload(K, &C.c_ptr, T.ptr[2])) || (rc = dev_upload(K, &C.c_col, T.col[2])) || (rc = dev_upload(K, &C.c_coef, T.coef[2]))) return rc;
    if ((rc = dev_upload(K, &C.tw, T.tw)) || (rc = dev_upload(K, &C.tw_inv, T.tw_inv)) || (rc = dev_upload(K, &C.coset, T.coset)) ||
        (rc = dev_upload(K, &C.coset_inv, T.coset_inv)) || (rc = dev_upload(K, &C.zinv, T.zinv))) return rc;
    return 0;
}


// ---- offset points for the unchecked mixed additions: O1 = [c] G1, O2 = [c] G2 with c = SHA-256("libzkp-amd msm offset")
g2_aff host_g2_generator() {
    static const char* dec[4] = {"10857046999023057135944570762232829481370756359578518086990519993285655852781",
                                 "11559732032986387107991004021392285783925812861821192530917403151452391805634",
                                 "8495653923123431417604973247489272438418190587263600148770280649306958101930",
                                 "4082367875863433681332203403145435568316851327593401208105741076214120093531"};
    fq c[4];
    for (int k = 0; k < 4; k++) {
        fq acc = fq_zero(); const fq ten = fq_from_u64(10);
        for (const char* q = dec[k]; *q; q++) acc = fq_add(fq_mul(acc, ten), fq_from_u64((uint64_t)(*q - '0')));
        c[k] = acc;
    }
    return g2_aff{fq2{c[0], c[1]}, fq2{c[2], c[3]}};
}
g1_aff host_g1_generator() { return g1_aff{fq_from_u64(1), fq_from_u64(2)}; }
struct MsmOffsets { g1_jac o1; g2_jac o2; };
const MsmOffsets& msm_offsets() {               // host-side constants, computed once per process
    static const MsmOffsets off = [] {
        uint8_t h[32]; const char* tag = "libzkp-amd msm offset"; sha256_host(h, (const uint8_t*)tag, strlen(tag));
        uint32_t k[8]; memcpy(k, h, 32); k[7] &= 0x0fffffffu;
        return MsmOffsets{jac_mul_raw(jac_from_aff(host_g1_generator()), k), jac_mul_raw(jac_from_aff(host_g2_generator()), k)};
    }();
    return off;
}
template <class J> void append_words(std::vector<uint32_t>& v, const J& p) { const uint32_t* w = reinterpret_cast<const uint32_t*>(&p); for (size_t i = 0; i < sizeof(J) / 4; i++) v.push_back(w[i]); }
template <class J> J host_neg_multiple(const J& o, uint32_t k) {     // -(k * O), k small
    J acc = o; for (uint32_t i = 1; i < k; i++) acc = jac_add(acc, o);
    return jac_neg(acc);
}
// the words of O (k = 0: the accumulator every chunk starts from) or of -(k O) (what the sum of k chunks is corrected by)
void append_offset(std::vector<uint32_t>& v, bool g2, uint32_t k) {
    const MsmOffsets& o = msm_offsets();
    if (!g2) append_words(v, k ? host_neg_multiple(o.o1, k) : o.o1); else append_words(v, k ? host_neg_multiple(o.o2, k) : o.o2);
}
int upload_offset_point(G16Key& K, bool g2, const uint32_t** d_init) { std::vector<uint32_t> init; append_offset(init, g2, 0); return dev_upload(K, d_init, init); }
// Chunking of one key-point MSM for a batch of `rows` proofs.  One workgroup (G1: 1024 lanes, G2: 512) fills a CU, so the
// grid runs in strict rounds of `resident` equal workgroups: take the window-granular chunk count that minimises
// rounds x (windows per workgroup + per-workgroup overhead) + the partial-sum work that grows with the chunk count.
uint32_t choose_chunks(uint64_t windows, uint32_t ntargets, uint32_t rows, uint32_t resident, uint32_t tb) {
    const uint32_t groups = (rows + tb - 1) / tb;
    uint32_t hi = (uint32_t)(windows / 8); if (hi > 2048) hi = 2048; if (hi < ntargets) hi = ntargets;
    uint32_t best = ntargets; double best_cost = 1e300;
    for (uint32_t c = ntargets; c <= hi; c++) {
        const double rounds = std::ceil((double)c * groups / resident);
        const double cost = rounds * (std::ceil((double)windows / c) + 2.5) + 0.25 * c / 8.0;
        if (cost < best_cost) { best_cost = cost; best = c; }
    }
    return best;
}
// (the parts, the layout, the digit rows and the offset counts of a chunking: g16_share.h)
int get_chunking(G16Key& K, bool g2, int part, uint32_t rows, const G16Key::Chunking** out) {
    const uint32_t resident = (uint32_t)dev().num_cu * g16_msm_blocks_per_cu(g2);      // workgroups the chip holds at a time
    if (part == G16_PART_ALL && !g2) return fail(ZKP_HIP_E_ARGUMENT, "G16_PART_ALL is the G2 launch");
    const std::vector<SlotList> targets = g16_part_targets(g2 ? K.targets_g2 : K.targets_g1, part);
    uint32_t c = choose_chunks(g16_windows(targets), (uint32_t)targets.size(), rows, resident, g16_msm_rows_per_block(g2));
    if (g_budget_request >= 10000) c = g_budget_request - 10000;                  // benchmarking knob
    auto& cache = g2 ? K.lays_g2 : K.lays_g1;
    const uint64_t key = (uint64_t)part << 32 | c;
    auto it = cache.find(key);
    if (it == cache.end()) {
        const G16Chunks P = g16_plan_chunks(targets, g2 ? K.hscal_g2 : K.hscal_g1, part, c);
        G16Key::Chunking ch; int rc;
        const GatherShape shape{K.rx.nent, K.rx.slot_ent, K.rx.uneven ? 1u : 0u, K.rx.digw};
        if ((rc = upload_layout(ch.lay, P.L, &shape, P.scal.data()))) return rc;
        std::vector<uint32_t> corr;
        for (uint32_t k : P.offsets) append_offset(corr, g2, k);
        if ((rc = dev_upload(K, &ch.corr, corr))) return rc;
        if ((rc = dev_upload(K, &ch.scal, P.scal))) return rc;
        it = cache.emplace(key, ch).first;
    }
    *out = &it->second;
    return 0;
}

// ---- ark-serialize (uncompressed) proving / verifying key: the point reader and the format rule are in g16_keyblob.h

// ---- key tables: sized at run time, shared by the shards of one physical GPU
// bytes of the two MSM tables of a key with n1 G1 and n2 G2 points at radix 2^wbits
uint64_t key_table_bytes(size_t n1, size_t n2, uint32_t wbits, bool uneven = false) {
    const G16Radix rx = g16_radix(wbits, uneven);
    return ((uint64_t)n1 * g16_table_entry_words(false, true) + (uint64_t)n2 * g16_table_entry_words(true, true)) * 4ull * rx.slot_ent;
}
// The radix of a key's tables.  DEFAULT: 2^13 (19-20 windows of 4096 entries: 27.8 GB measured for the two circuits of libzkp together) -- the knee
// of the measured curve (DESIGN.md 6b: 2^14-uneven, ~72 GB, is 1.7 % faster on the mixed batch; 2^13 against even 2^14: 0.4 %), because a
// drop-in library should not take a quarter of a 288 GB device silently.  Opt-ins: ZKP_HIP_G16_TABLE_BUDGET_MB=<MB per key> takes the
// largest radix (2^14 in its uneven form first) whose tables fit that budget; ZKP_HIP_G16_WBITS=8..15 forces one.  In every case the
// tables must also fit what the device has free (45 % of it per key beyond an 8 GB reserve for workspaces, so that the second
// circuit's key finds room too); smaller radices are taken when they do not.
int choose_radix(size_t n1, size_t n2, uint32_t* wbits_out, bool* uneven_out) {
    *uneven_out = false;
    const int forced = env_int("ZKP_HIP_G16_WBITS", 0);
    if (forced) {
        if (forced < (int)G16_WBITS_MIN || forced > (int)G16_WBITS_MAX) return fail(ZKP_HIP_E_ARGUMENT, "ZKP_HIP_G16_WBITS must be 8..15");
        *wbits_out = (uint32_t)forced; *uneven_out = forced == 14 && env_int("ZKP_HIP_G16_UNEVEN", 1) != 0; return 0;
    }
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const int budget_mb = env_int("ZKP_HIP_G16_TABLE_BUDGET_MB", 0);
    const uint64_t reserve = 8ull << 30;
    const uint64_t fits = free_b > reserve ? (uint64_t)((free_b - reserve) * 0.45) : 0;
    uint64_t budget = budget_mb > 0 ? (uint64_t)budget_mb << 20 : fits;
    uint32_t first = G16_WBITS_KNEE;
    if (budget_mb > 0) {           // an explicit budget: the fastest tables it allows
        first = G16_WBITS_DEFAULT;
        if (G16_WBITS_DEFAULT == 14 && env_int("ZKP_HIP_G16_UNEVEN", 1) != 0 && key_table_bytes(n1, n2, 14, true) <= budget) { *wbits_out = 14; *uneven_out = true; return 0; }
    }
    for (uint32_t w = first; w >= G16_WBITS_MIN; w--)
        if (key_table_bytes(n1, n2, w) <= budget) { *wbits_out = w; return 0; }
    char msg[256];
    snprintf(msg, sizeof msg, "not enough device memory for the proving key's window tables: %llu MB at the smallest radix (2^%u), budget %llu MB (%llu MB free)",
             (unsigned long long)(key_table_bytes(n1, n2, G16_WBITS_MIN) >> 20), G16_WBITS_MIN, (unsigned long long)(budget >> 20), (unsigned long long)(free_b >> 20));
    return fail(ZKP_HIP_E_RUNTIME, msg);
}
// One table set per (GPU, circuit, key bytes, radix) in the process: the shards registered on the same HIP device (zkp_hip_init_devices
// with a device listed twice, as the one-GPU tests do; several contexts of a server) share it instead of holding ~65 GB each.
struct SharedTables { int hip_dev, kind; uint8_t digest[32]; uint32_t wbits; bool share_ab; uint32_t *g1, *g2; int refs; };      // wbits | uneven << 8; share_ab: laid out with the shared A / B1 slots (g16_share.h)
struct TableRegistry { std::mutex mu; std::vector<SharedTables> v; std::map<int, std::mutex> build_mu; };
TableRegistry& table_registry() { static TableRegistry* r = new TableRegistry(); return *r; }
std::mutex& table_build_mutex(int hip_dev) { TableRegistry& R = table_registry(); std::lock_guard<std::mutex> lk(R.mu); return R.build_mu[hip_dev]; }
// Takes a reference to the live entry of `want`'s GPU, circuit, key bytes and share_ab: of exactly its radix, or with any_radix the first
// one, whose radix K takes with the tables.  false: there is none.
bool acquire_tables(G16Key& K, const SharedTables& want, bool any_radix) {
    TableRegistry& R = table_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    for (size_t i = 0; i < R.v.size(); i++) {
        SharedTables& e = R.v[i];
        if (e.refs <= 0 || e.hip_dev != want.hip_dev || e.kind != want.kind || e.share_ab != want.share_ab || memcmp(e.digest, want.digest, 32) || (!any_radix && e.wbits != want.wbits)) continue;
        e.refs++; K.shared_tables = (int)i; K.table_g1 = e.g1; K.table_g2 = e.g2; K.rx = g16_radix(e.wbits & 0xffu, (e.wbits >> 8) != 0);
        return true;
    }
    return false;
}
void register_tables(G16Key& K, SharedTables e) {
    TableRegistry& R = table_registry();
    std::lock_guard<std::mutex> lk(R.mu);
    e.refs = 1; R.v.push_back(e);          // freshly built tables, K their first holder
    K.shared_tables = (int)R.v.size() - 1; K.table_g1 = e.g1; K.table_g2 = e.g2;
}
// ---- the key check at load (g16_keycheck.h, DESIGN.md R20)
// ZKP_HIP_G16_TABLE_FLIP=<g1|g2|vk>:<word index>, read on every load: bit 0 of that word of the named table is flipped between its build and
// its check (a diagnostic modelled on ZKP_HIP_SELF_CHECK_FLIP).  No effect on tables that are acquired, not built.
struct KcFlip { int which = -1; uint64_t word = 0; };
int kc_read_flip(KcFlip& F) {
    F = KcFlip();
    const char* e = getenv("ZKP_HIP_G16_TABLE_FLIP");
    if (!e || !*e) return 0;
    static const char* names[3] = {"g1:", "g2:", "vk:"};
    for (int k = 0; k < 3; k++) {
        if (strncmp(e, names[k], 3)) continue;
        const char* q = e + 3; char* end = nullptr;
        if (*q < '0' || *q > '9') break;
        errno = 0;
        const unsigned long long v = strtoull(q, &end, 10);
        if (errno || !end || *end) break;
        F.which = k; F.word = v;
        return 0;
    }
    return fail(ZKP_HIP_E_ARGUMENT, "ZKP_HIP_G16_TABLE_FLIP must be <g1|g2|vk>:<word index>");
}
struct KcLoadOpts { KcFlip flip; bool check = true; };
int kc_read_load_opts(KcLoadOpts& O) { O.check = env_int("ZKP_HIP_G16_TABLE_CHECK", 1) != 0; return kc_read_flip(O.flip); }
static const char* const KC_TABLE_NAME[3] = {"G1", "G2", "VK"};
// what one table check found
struct KcTableResult { uint64_t entries = 0; uint32_t bad_pairs = 0, bad_entries = 0, slot = 0, win = 0, ent = 0; std::vector<uint32_t> pair_bad; };
// every entry of the `nslots` slots of `table` against d_bases; waits for the result.  Counts into the shard's keycheck counters.
int kc_check_table(bool g2, const uint32_t* d_bases, uint32_t nslots, const uint32_t* table, bool msm_form, const G16Radix& rx, KcTableResult& R, bool want_pairs = false) {
    Tally tally(dev().counters, FAM_KEY_CHECK, Tally::COMMITTED);          // a check that fails to run is not counted
    R = KcTableResult();
    if (nslots == 0) return 0;
    DevScope mem;
    uint32_t *d_pairs = nullptr, *d_out = nullptr;
    const size_t npairs = (size_t)nslots * rx.nwin;
    HIP_TRY(mem.alloc(&d_pairs, npairs * 4)); HIP_TRY(mem.alloc(&d_out, KC_OUT_WORDS * 4));
    HIP_TRY(g16_launch_check_table(g2, d_bases, nslots, table, msm_form, rx, d_pairs, d_out, dev().stream));
    uint32_t out[KC_OUT_WORDS];
    HIP_TRY(hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, dev().stream));
    if (want_pairs) { R.pair_bad.resize(npairs); HIP_TRY(hipMemcpyAsync(R.pair_bad.data(), d_pairs, npairs * 4, hipMemcpyDeviceToHost, dev().stream)); }
    HIP_TRY(hipStreamSynchronize(dev().stream));
    R.entries = (uint64_t)nslots * rx.slot_ent; R.bad_pairs = out[0]; R.bad_entries = out[1];
    if (R.bad_pairs) { const uint64_t key = (uint64_t)out[3] << 32 | out[2]; R.slot = (uint32_t)(key >> 40); R.win = (uint32_t)(key >> 32) & 0xffu; R.ent = (uint32_t)key; }
    tally[CTR_KEY_ENTRIES_CHECKED] = R.entries;
    tally.commit();
    return 0;
}
// a freshly built table: the flip diagnostic when it names this table, then the self-check.  `which`: 0 G1, 1 G2, 2 VK (KC_TABLE_NAME)
int kc_after_build(int which, const uint32_t* d_bases, uint32_t nslots, uint32_t* table, bool msm_form, const G16Radix& rx, const KcLoadOpts& O) {
    const bool g2 = which == 1;
    if (O.flip.which == which) {
        const uint64_t words = (uint64_t)nslots * rx.slot_ent * g16_table_entry_words(g2, msm_form);
        if (O.flip.word >= words) return fail(ZKP_HIP_E_ARGUMENT, "ZKP_HIP_G16_TABLE_FLIP: word index beyond the table");
        g16_launch_flip_word(table, O.flip.word, dev().stream);
        HIP_TRY(hipGetLastError());
    }
    if (!O.check) return 0;
    KcTableResult R; int rc;
    if ((rc = kc_check_table(g2, d_bases, nslots, table, msm_form, rx, R))) return rc;
    if (!R.bad_pairs) return 0;
    dev().counters[FAM_KEY_CHECK].v[CTR_KEY_REFUSED]++;
    char msg[200];
    snprintf(msg, sizeof msg, "Groth16 key tables failed their self-check (%s slot %u window %u, %u inconsistent windows)", KC_TABLE_NAME[which], R.slot, R.win, R.bad_pairs);
    return fail(ZKP_HIP_E_RUNTIME, msg);
}
// the finite G2 points of a key on the GPU, one lane each: ok[i] = 1 inside the prime-order subgroup
int kc_subgroup_run(const G16G2List& L, std::vector<uint8_t>& ok) {
    ok.assign(L.pts.size(), 0);
    if (L.pts.empty()) return 0;
    static_assert(sizeof(g2_aff) == 160, "40 plain words per G2 point");
    DevScope mem;
    uint32_t* d_pts = nullptr; uint8_t* d_ok = nullptr;
    HIP_TRY(mem.alloc(&d_pts, L.pts.size() * sizeof(g2_aff))); HIP_TRY(mem.alloc(&d_ok, L.pts.size()));
    HIP_TRY(hipMemcpyAsync(d_pts, L.pts.data(), L.pts.size() * sizeof(g2_aff), hipMemcpyHostToDevice, dev().stream));
    g16_launch_subgroup(d_pts, (uint32_t)L.pts.size(), d_ok, dev().stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ok.data(), d_ok, ok.size(), hipMemcpyDeviceToHost, dev().stream));
    HIP_TRY(hipStreamSynchronize(dev().stream));
    return 0;
}
// ark's rule at load (deserialize_uncompressed is Validate::Yes): every finite G2 point of the key file lies in the prime-order subgroup
int kc_load_subgroup(const G16VkBlob& B, const G16PkBlob* Q) {
    const G16G2List L = g16_key_g2_points(B, Q);
    std::vector<uint8_t> ok; int rc;
    if ((rc = kc_subgroup_run(L, ok))) return rc;
    for (size_t i = 0; i < ok.size(); i++) {
        if (ok[i]) continue;
        dev().counters[FAM_KEY_CHECK].v[CTR_KEY_REFUSED]++;
        char name[48], msg[160]; g16_g2_point_name(name, sizeof name, L.index[i]);
        snprintf(msg, sizeof msg, "key point %s is not in the prime-order subgroup of G2", name);
        return fail(ZKP_HIP_E_ARGUMENT, msg);
    }
    return 0;
}

// d_bases_out: the device copy of the bases the builder read (held by K), for the check that follows the build
template <uint32_t AW, class Pt>
int build_tables(G16Key& K, const std::vector<Pt>& bases, uint32_t** table, bool msm_form, const G16Radix& rx, bool owned = true, const uint32_t** d_bases_out = nullptr) {
    std::vector<uint32_t> flat; flat.reserve(bases.size() * AW);
    for (auto& b : bases) { const uint32_t* w = reinterpret_cast<const uint32_t*>(&b); for (uint32_t k = 0; k < AW; k++) flat.push_back(w[k]); }
    uint32_t* d_bases = nullptr; int rc;
    if ((rc = dev_upload(K, &d_bases, flat))) return rc;
    if (d_bases_out) *d_bases_out = d_bases;
    const size_t words = bases.size() * (size_t)rx.slot_ent * g16_table_entry_words(AW == 40, msm_form);
    uint32_t* tab = nullptr;
    if (hipMalloc(&tab, words * 4 + 64) != hipSuccess) {
        (void)hipGetLastError();
        char msg[200]; snprintf(msg, sizeof msg, "out of device memory allocating %llu MB of key tables (radix 2^%u)", (unsigned long long)((words * 4) >> 20), rx.wbits);
        return fail(ZKP_HIP_E_RUNTIME, msg);
    }
    if (owned) K.allocs.push_back(tab);
    *table = tab;                                            // (an unowned table is the caller's from here on, whatever follows)
    g16_launch_build_table(AW == 40, d_bases, (uint32_t)bases.size(), tab, dev().stream, msm_form, rx);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(dev().stream));
    return 0;
}

// everything a key slot holds on the device (a loaded key, or what a failed load got as far as acquiring)
void release_key(G16Key& K) {
    (void)hipDeviceSynchronize();
    if (K.shared_tables >= 0) {          // its reference to the shared MSM tables: the last holder frees them
        TableRegistry& R = table_registry();
        std::lock_guard<std::mutex> lk(R.mu);
        SharedTables& e = R.v[(size_t)K.shared_tables];
        if (--e.refs == 0) { (void)hipFree(e.g1); (void)hipFree(e.g2); e.g1 = e.g2 = nullptr; }
    }
    for (void* p : K.allocs) (void)hipFree(p);
    for (auto& e : K.lays_g1) free_layout(e.second.lay);
    for (auto& e : K.lays_g2) free_layout(e.second.lay);
    K = G16Key();
}
int load_key_body(int kind, const uint8_t* pk, uint64_t len);
// what a prove call answers when its circuit has no proving key on this shard
int no_proving_key(const G16Key& K) {
    return fail(ZKP_HIP_E_ARGUMENT, K.verifier_only() ? "only a verifying key is loaded for this circuit: proving needs the proving key (zkp_hip_groth16_load_key)"
                                                      : "no proving key loaded for this circuit (zkp_hip_groth16_load_key)");
}
int load_key_locked(int kind, const uint8_t* pk, uint64_t len) {
    if (kind != G16_EQUALITY && kind != G16_MEMBERSHIP) return fail(ZKP_HIP_E_ARGUMENT, "unknown circuit kind");
    G16Key& K = g16s().key[kind];
    if (K.loaded || K.shared_tables >= 0 || !K.allocs.empty()) release_key(K);
    int rc;
    ShardCounter& kc = dev().counters[FAM_KEY_CHECK];
    const uint64_t checked_before = kc.v[CTR_KEY_ENTRIES_CHECKED];
    try { rc = load_key_body(kind, pk, len); }
    catch (...) { release_key(K); throw; }               // (the ABI's barrier reports it; the registry reference and the blocks are not leaked)
    if (rc) { const std::string keep = t_err; release_key(K); t_err = keep; }      // a failed load leaves no table reference and no allocation behind
    if (kc.v[CTR_KEY_ENTRIES_CHECKED] != checked_before) kc.v[CTR_KEY_LOADS_CHECKED]++;      // freshly built tables went through the self-check
    return rc;
}
// The verifying-key part of a key, shared by both formats: gamma, delta, gamma_abc_g1 and the constant Miller-loop factor of
// (beta, -alpha), computed once on the host.  Nothing else is needed to verify (g16_verify.h, fq2vm.h, g16_rlc.h).
int install_verifying_key(G16Key& K, const G16VkBlob& B, const KcLoadOpts& O) {
    int rc;
    K.vk_ready = false;
    std::vector<g1_aff> ic_pts; for (auto& e : B.abc) ic_pts.push_back(e.p);
    ic_pts.push_back(B.alpha_g1.p);                  // point n_ic of the verifier's tables: alpha (the batch check's virtual envelope, g16_rlc.h)
    std::vector<uint32_t> icw; for (auto& p : ic_pts) append_words(icw, p);
    const uint32_t* d_ic = nullptr;
    if ((rc = dev_upload(K, &d_ic, icw))) return rc;
    // gamma_abc_g1 are fixed points of the key: the verifier's public-input accumulation walks radix-1024 window tables
    // (the prover's table builder) instead of doubling-and-adding
    uint32_t* d_ic_tab = nullptr;
    const G16Radix vrx = g16_radix(G16V_WBITS);
    const uint32_t* d_ic_bases = nullptr;
    if ((rc = build_tables<20>(K, ic_pts, &d_ic_tab, false, vrx, true, &d_ic_bases))) return rc;
    if ((rc = kc_after_build(2, d_ic_bases, (uint32_t)ic_pts.size(), d_ic_tab, false, vrx, O))) return rc;      // (the table is K's: a failed load frees it)
    K.vk_table_bytes = (uint64_t)ic_pts.size() * vrx.slot_ent * g16_table_entry_words(false, false) * 4ull;
    K.vk.gamma = B.gamma_g2.p; K.vk.delta = B.delta_g2.p; K.vk.beta = B.beta_g2.p; K.vk.n_ic = (uint32_t)B.abc.size(); K.vk.ic = d_ic; K.vk.ic_table = d_ic_tab;
    K.vk.ml_alpha_beta = miller_loop(B.beta_g2.p, aff_neg(B.alpha_g1.p));
    std::vector<uint32_t> kc(6 * 20), lines;
    g16_vm_key_constants(B.beta_g2.p, aff_neg(B.alpha_g1.p), B.gamma_g2.p, B.delta_g2.p, kc.data(), lines);
    if ((rc = dev_upload(K, &K.vm_kconst, kc)) || (rc = dev_upload(K, &K.vm_lines, lines))) return rc;
    K.vk_ready = true;
    return 0;
}
int ensure_mimc_dev() {
    if (g16s().mimc_dev) return 0;
    ensure_mimc_constants();
    std::vector<uint32_t> mc; for (auto& c : g_mimc_host) put_fr(mc, c);
    HIP_TRY(hipMalloc(&g16s().mimc_dev, mc.size() * 4)); HIP_TRY(hipMemcpy(g16s().mimc_dev, mc.data(), mc.size() * 4, hipMemcpyHostToDevice));
    return 0;
}
int load_key_body(int kind, const uint8_t* pk, uint64_t len) {
    G16Key& K = g16s().key[kind];
    const HostR1CS cs = kind == G16_EQUALITY ? build_equality_r1cs() : build_membership_r1cs();
    int rc;
    // parse: ProvingKey { vk { alpha_g1, beta_g2, gamma_g2, delta_g2, gamma_abc_g1 }, beta_g1, delta_g1, a_query, b_g1_query, b_g2_query, h_query, l_query },
    // or its vk alone: a blob that ends behind gamma_abc_g1 is a verifying key (g16_keyblob.h)
    KcLoadOpts O;
    if ((rc = kc_read_load_opts(O))) return rc;
    KeyReader R{pk, len};
    G16VkBlob B; G16PkBlob Q;
    const int format = g16_read_key_prefix(R, B);
    if (format == G16_BLOB_MALFORMED)
        return fail(ZKP_HIP_E_ARGUMENT, "malformed proving key or verifying key (expected ark-serialize uncompressed ProvingKey<Bn254>, or its VerifyingKey<Bn254> alone)");
    if (format == G16_BLOB_VERIFYING_KEY) {          // a verifier-only key: no circuit, no MiMC constants, no MSM tables, no registry entry, no layouts
        if (const char* why = g16_check_verifying_key(B, cs.n_inst)) return fail(ZKP_HIP_E_ARGUMENT, why);
        if ((rc = kc_load_subgroup(B, nullptr)) || (rc = install_verifying_key(K, B, O))) return rc;
        sha256_host(K.digest, pk, len); K.have_digest = true;
        return 0;
    }
    if (const char* why = g16_read_proving_key(R, B, g16_key_shape(cs), Q)) return fail(ZKP_HIP_E_ARGUMENT, why);
    if ((rc = kc_load_subgroup(B, &Q))) return rc;           // before any table is built or acquired
    // plan (g16_share.h).  ZKP_HIP_G16_SHARE_AB=0 gives every finite b_g1_query point its own slot and table again; it is read here, once
    // per load, and tables are shared only between loads that read the same value.
    const bool share_ab = env_int("ZKP_HIP_G16_SHARE_AB", 1) != 0;
    G16KeyPlan P;
    if (const char* why = g16_plan_key(P, B, Q, cs, share_ab)) return fail(ZKP_HIP_E_UNSUPPORTED, why);
    // the radix.  If another shard of this GPU already holds tables for these key bytes, this shard takes a reference AND their radix (what
    // is free now -- less than when the first shard chose -- must not pick a smaller one and build a second set); choose_radix only when
    // building.  A forced radix (ZKP_HIP_G16_WBITS) shares only an entry of exactly that radix.  One load at a time per GPU from here on.
    SharedTables want{}; want.hip_dev = dev().hip_dev; want.kind = kind; want.share_ab = share_ab; sha256_host(want.digest, pk, len);
    std::lock_guard<std::mutex> build_lock(table_build_mutex(want.hip_dev));
    if (env_int("ZKP_HIP_G16_WBITS", 0) != 0 || !acquire_tables(K, want, true)) {
        uint32_t wb = 0; bool uneven = false;
        if ((rc = choose_radix(P.radix_points_g1, P.radix_points_g2, &wb, &uneven))) return rc;
        K.rx = g16_radix(wb, uneven); want.wbits = K.rx.wbits | K.rx.uneven << 8;
        if (!acquire_tables(K, want, false)) {       // the MSM tables: built here
            // built, self-checked (kc_after_build), and only then registered: tables that fail are freed here
            const uint32_t *b1 = nullptr, *b2 = nullptr;
            if ((rc = build_tables<20>(K, P.bases_g1, &want.g1, true, K.rx, false, &b1)) || (rc = build_tables<40>(K, P.bases_g2, &want.g2, true, K.rx, false, &b2)) ||
                (rc = kc_after_build(0, b1, (uint32_t)P.bases_g1.size(), want.g1, true, K.rx, O)) || (rc = kc_after_build(1, b2, (uint32_t)P.bases_g2.size(), want.g2, true, K.rx, O))) {
                (void)hipDeviceSynchronize();
                if (want.g1) (void)hipFree(want.g1);
                if (want.g2) (void)hipFree(want.g2);
                return rc;
            }
            register_tables(K, want);
        }
    }
    K.table_bytes = key_table_bytes(P.bases_g1.size(), P.bases_g2.size(), K.rx.wbits, K.rx.uneven);
    if ((rc = upload_circuit(K, cs)) || (rc = ensure_mimc_dev())) return rc;
    K.targets_g1 = g16_plan_targets(P.cls_g1, K.rx); K.targets_g2 = g16_plan_targets(P.cls_g2, K.rx);
    K.win_g1 = g16_windows(K.targets_g1); K.win_g2 = g16_windows(K.targets_g2);
    K.hscal_g1 = P.row_g1; K.hscal_g2 = P.row_g2;
    if ((rc = upload_offset_point(K, false, &K.init_g1)) || (rc = upload_offset_point(K, true, &K.init_g2))) return rc;
    // the verifying key that leads the file; one that cannot verify (gamma or a gamma_abc_g1 point at infinity) leaves a key that only proves
    if (!g16_check_verifying_key(B, K.n_inst) && (rc = install_verifying_key(K, B, O))) return rc;
    memcpy(K.digest, want.digest, 32); K.have_digest = true;
    K.loaded = true;
    return 0;
}


// ---- zkpkeycheck_key (include/libzkp_hip_keycheck.h): the stages of a key check on the bound shard
// fresh bytes from the operating system; a call interrupted by a signal before it read anything is repeated
int kc_fresh_bytes(uint8_t* buf, size_t n) {
    size_t got = 0;
    while (got < n) {
        const ssize_t r = getrandom(buf + got, n - got, 0);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return fail(ZKP_HIP_E_RUNTIME, "getrandom failed");
        got += (size_t)r;
    }
    return 0;
}
bool kc_pairings_equal(const g1_aff& p1, const g2_aff& q1, const g1_aff& p2, const g2_aff& q2) {      // e(p1, q1) == e(p2, q2)
    return fq12_is_one(final_exponentiation_chain(fq12_mul(miller_loop(q1, p1), miller_loop(q2, aff_neg(p2)))));
}
// TWINS: S1 = sum rho_i b_g1_query[i], S2 = sum rho_i b_g2_query[i] on the GPU (a lane per point, then the sum tree), the pairings on the host
int kc_twins_run(const G16VkBlob& B, const G16PkBlob& Q, zkp_keycheck_report& rep) {
    const G16Twins T = g16_key_twins(Q);
    rep.twins_checked = (uint32_t)T.index.size(); rep.twin_inf_mismatches = T.inf_mismatches;
    if (T.inf_mismatches) { rep.twins_query_ok = 0; return 0; }          // fails the stage before any arithmetic
    const uint32_t n = (uint32_t)T.index.size();
    if (n > 65535u) return fail(ZKP_HIP_E_UNSUPPORTED, "too many twins for one sum (16-bit chunk indices)");
    rep.twins_beta_delta_ok = kc_pairings_equal(Q.beta_g1.p, B.delta_g2.p, Q.delta_g1.p, B.beta_g2.p) ? 1 : 0;
    if (n == 0) { rep.twins_query_ok = 1; return 0; }
    std::vector<g1_aff> p1(n); std::vector<g2_aff> p2(n); std::vector<uint8_t> rho(16 * (size_t)n);
    for (uint32_t k = 0; k < n; k++) { p1[k] = Q.b_g1_query[T.index[k]].p; p2[k] = Q.b_g2_query[T.index[k]].p; }
    int rc;
    if ((rc = kc_fresh_bytes(rho.data(), rho.size()))) return rc;
    static_assert(sizeof(g1_aff) == 80 && sizeof(g2_aff) == 160, "plain affine points: 20 / 40 words");
    const uint16_t tcb[2] = {0, (uint16_t)n};
    DevScope mem;
    uint32_t *d_p1 = nullptr, *d_p2 = nullptr, *d_rho = nullptr, *d_part1 = nullptr, *d_part2 = nullptr, *d_sums = nullptr; uint16_t* d_tcb = nullptr;
    HIP_TRY(mem.alloc(&d_p1, 80 * (size_t)n)); HIP_TRY(mem.alloc(&d_p2, 160 * (size_t)n)); HIP_TRY(mem.alloc(&d_rho, rho.size()));
    HIP_TRY(mem.alloc(&d_part1, (size_t)G1_JAC_W * 4 * n)); HIP_TRY(mem.alloc(&d_part2, (size_t)G2_JAC_W * 4 * n));
    HIP_TRY(mem.alloc(&d_sums, (size_t)(G1_JAC_W + G2_JAC_W) * 4)); HIP_TRY(mem.alloc(&d_tcb, sizeof tcb));
    hipStream_t st = dev().stream;
    HIP_TRY(hipMemcpyAsync(d_p1, p1.data(), 80 * (size_t)n, hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(d_p2, p2.data(), 160 * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rho, rho.data(), rho.size(), hipMemcpyHostToDevice, st)); HIP_TRY(hipMemcpyAsync(d_tcb, tcb, sizeof tcb, hipMemcpyHostToDevice, st));
    g16_launch_twin_weighted(false, d_p1, d_rho, n, d_part1, st); HIP_TRY(hipGetLastError());
    g16_launch_twin_weighted(true, d_p2, d_rho, n, d_part2, st); HIP_TRY(hipGetLastError());
    ReduceView R1{}; R1.rows = 1; R1.ntargets = 1; R1.partial = d_part1; R1.target_chunk_begin = d_tcb;
    ReduceView R2 = R1; R2.partial = d_part2;
    g16_launch_sum(false, R1, d_sums, st); HIP_TRY(hipGetLastError());
    g16_launch_sum(true, R2, d_sums + G1_JAC_W, st); HIP_TRY(hipGetLastError());
    uint32_t sums[G1_JAC_W + G2_JAC_W];
    HIP_TRY(hipMemcpyAsync(sums, d_sums, sizeof sums, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));          // (the host vectors above are read by the uploads until here)
    g1_aff s1; g2_aff s2;
    const bool f1 = jac_to_aff(s1, ld_g1_jac(sums, 0, 0, 1)), f2 = jac_to_aff(s2, ld_g2_jac(sums + G1_JAC_W, 0, 0, 1));
    // a sum at infinity pairs to one: the identity then holds exactly when the other sum is at infinity too
    rep.twins_query_ok = (f1 && f2) ? (kc_pairings_equal(s1, B.beta_g2.p, Q.beta_g1.p, s2) ? 1 : 0) : (f1 == f2 ? 1 : 0);
    return 0;
}
// TABLES: the tables resident on this shard for `kind` against the points of the blob.  The MSM tables of a proving key are laid out by
// g16_plan_key under the ZKP_HIP_G16_SHARE_AB of now, which must be that of the load (the registry entry of K says which it was).
int kc_tables_run(int kind, const G16VkBlob& B, const G16PkBlob* Q, const HostR1CS& cs, const uint8_t digest[32], zkp_keycheck_report& rep) {
    G16Key& K = g16s().key[kind];
    if (!(K.loaded || K.vk_ready) || !K.have_digest || memcmp(K.digest, digest, 32) || (Q != nullptr) != K.loaded)
        return fail(ZKP_HIP_E_ARGUMENT, "ZKP_KEYCHECK_TABLES: this is not the key loaded for this circuit on this shard");
    int rc;
    // one table: upload the bases the builder read, check, fold into the report
    auto run = [&](int which, const uint32_t* words, uint32_t nslots, uint32_t aw, const uint32_t* table, bool msm_form, const G16Radix& rx, uint64_t& entries) -> int {
        DevScope mem; uint32_t* d_bases = nullptr;
        HIP_TRY(mem.alloc(&d_bases, (size_t)nslots * aw * 4));
        HIP_TRY(hipMemcpyAsync(d_bases, words, (size_t)nslots * aw * 4, hipMemcpyHostToDevice, dev().stream));
        KcTableResult R;
        if (int rcc = kc_check_table(which == 1, d_bases, nslots, table, msm_form, rx, R)) return rcc;      // (waits for the stream: `words` is free again)
        entries = R.entries;
        if (R.bad_pairs && rep.table_first_which < 0) { rep.table_first_which = which; rep.table_first_slot = R.slot; rep.table_first_window = R.win; rep.table_first_entry = R.ent; }
        rep.table_bad_pairs += R.bad_pairs;
        return 0;
    };
    if (Q) {
        bool share_ab = env_int("ZKP_HIP_G16_SHARE_AB", 1) != 0;
        if (K.shared_tables >= 0) { TableRegistry& TR = table_registry(); std::lock_guard<std::mutex> lk(TR.mu); share_ab = TR.v[(size_t)K.shared_tables].share_ab; }
        G16KeyPlan P;
        if (const char* why = g16_plan_key(P, B, *Q, cs, share_ab)) return fail(ZKP_HIP_E_UNSUPPORTED, why);
        if ((rc = run(0, reinterpret_cast<const uint32_t*>(P.bases_g1.data()), (uint32_t)P.bases_g1.size(), 20, K.table_g1, true, K.rx, rep.table_entries_g1)) ||
            (rc = run(1, reinterpret_cast<const uint32_t*>(P.bases_g2.data()), (uint32_t)P.bases_g2.size(), 40, K.table_g2, true, K.rx, rep.table_entries_g2))) return rc;
    }
    if (K.vk_ready) {
        std::vector<g1_aff> ic; for (auto& e : B.abc) ic.push_back(e.p);
        ic.push_back(B.alpha_g1.p);
        if ((rc = run(2, reinterpret_cast<const uint32_t*>(ic.data()), (uint32_t)ic.size(), 20, K.vk.ic_table, false, g16_radix(G16V_WBITS), rep.table_entries_vk))) return rc;
    }
    return 0;
}
int keycheck_locked(int kind, const uint8_t* key, uint64_t len, uint32_t what, zkp_keycheck_report& rep) {
    using clk = std::chrono::steady_clock;
    auto ms_since = [](clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); };
    memset(&rep, 0, sizeof rep);
    rep.format = ZKP_KEYCHECK_FORMAT_UNKNOWN; rep.g2_first_outside = -1; rep.twins_query_ok = rep.twins_beta_delta_ok = -1; rep.table_first_which = -1;
    auto verdict = [&](uint32_t v, const char* msg) { rep.verdict = v; snprintf(rep.message, sizeof rep.message, "%s", msg); dev().counters[FAM_KEY_CHECK].v[CTR_KEY_REFUSED]++; return 0; };
    const HostR1CS cs = kind == G16_EQUALITY ? build_equality_r1cs() : build_membership_r1cs();
    int rc;
    // POINTS
    clk::time_point t0 = clk::now();
    KeyReader R{key, len};
    G16VkBlob B; G16PkBlob Q;
    const int format = g16_read_key_prefix(R, B);
    if (format == G16_BLOB_MALFORMED)
        return verdict(ZKP_KEYCHECK_FAILED_FORMAT, "malformed proving key or verifying key (expected ark-serialize uncompressed ProvingKey<Bn254>, or its VerifyingKey<Bn254> alone)");
    const bool is_pk = format == G16_BLOB_PROVING_KEY;
    rep.format = is_pk ? ZKP_KEYCHECK_FORMAT_PROVING_KEY : ZKP_KEYCHECK_FORMAT_VERIFYING_KEY;
    if (const char* why = is_pk ? g16_read_proving_key(R, B, g16_key_shape(cs), Q) : g16_check_verifying_key(B, cs.n_inst)) return verdict(ZKP_KEYCHECK_FAILED_FORMAT, why);
    {
        const G16G2List L = g16_key_g2_points(B, is_pk ? &Q : nullptr);
        std::vector<uint8_t> ok;
        if ((rc = kc_subgroup_run(L, ok))) return rc;
        rep.g2_checked = (uint32_t)ok.size();
        for (size_t i = 0; i < ok.size(); i++) if (!ok[i]) { if (rep.g2_first_outside < 0) rep.g2_first_outside = (int32_t)L.index[i]; rep.g2_outside++; }
    }
    rep.ms_points = ms_since(t0);
    if (rep.g2_outside) {
        char name[48], msg[160]; g16_g2_point_name(name, sizeof name, (uint32_t)rep.g2_first_outside);
        snprintf(msg, sizeof msg, "key point %s is not in the prime-order subgroup of G2", name);
        return verdict(ZKP_KEYCHECK_FAILED_SUBGROUP, msg);
    }
    rep.stages_run |= ZKP_KEYCHECK_POINTS;
    // TWINS (a verifying key has none: the two verdicts stay -1, not applicable)
    if ((what & ZKP_KEYCHECK_TWINS) && is_pk) {
        t0 = clk::now();
        if ((rc = kc_twins_run(B, Q, rep))) return rc;
        rep.ms_twins = ms_since(t0);
        if (rep.twin_inf_mismatches) return verdict(ZKP_KEYCHECK_FAILED_TWINS, "b_g1_query and b_g2_query are at infinity at different indices");
        if (rep.twins_query_ok != 1) return verdict(ZKP_KEYCHECK_FAILED_TWINS, "b_g1_query and b_g2_query do not share their discrete logarithms (e(S1, beta_g2) != e(beta_g1, S2))");
        if (rep.twins_beta_delta_ok != 1) return verdict(ZKP_KEYCHECK_FAILED_TWINS, "beta and delta do not share their discrete logarithms between G1 and G2 (e(beta_g1, delta_g2) != e(delta_g1, beta_g2))");
        rep.stages_run |= ZKP_KEYCHECK_TWINS;
    }
    // TABLES
    if (what & ZKP_KEYCHECK_TABLES) {
        t0 = clk::now();
        uint8_t digest[32]; sha256_host(digest, key, len);
        if ((rc = kc_tables_run(kind, B, is_pk ? &Q : nullptr, cs, digest, rep))) return rc;
        rep.ms_tables = ms_since(t0);
        if (rep.table_bad_pairs) {
            char msg[160];
            snprintf(msg, sizeof msg, "Groth16 key tables failed their check (%s slot %u window %u, %u inconsistent windows)", KC_TABLE_NAME[rep.table_first_which], rep.table_first_slot,
                     rep.table_first_window, rep.table_bad_pairs);
            return verdict(ZKP_KEYCHECK_FAILED_TABLES, msg);
        }
        rep.stages_run |= ZKP_KEYCHECK_TABLES;
    }
    return 0;
}

// ---- native trusted setup (Groth16::circuit_specific_setup, snark.rs:309-339).  The QAP is evaluated at tau on the host
// (a few thousand Fr operations); every key point is then scalar * generator, computed on the GPU as a one-slot
// fixed-base MSM with one lane per key point.  Generators: the standard (1, 2) and the EIP-197 G2 generator
// (ark-groth16 draws random generators; any generator pair yields a valid key).
fr tape_fr(const uint32_t seed[8], uint32_t idx, uint32_t slot) { uint32_t w[16]; tape_draw64(w, seed, idx, slot); return fp_from_wide<FrParams>(w); }

TableShape g16_table_shape(const G16Radix& rx) { return {rx.nwin, rx.nent, rx.digw, rx.slot_ent, rx.uneven}; }      // of a key's tables, for msm_view (zkp_hip.hip)

int gpu_scalar_mults(bool g2, const std::vector<fr>& scalars, std::vector<uint8_t>& out_bytes) {
    const uint32_t rows = (uint32_t)scalars.size(), AW = g2 ? 40 : 20, JW = g2 ? G2_JAC_W : G1_JAC_W, PB = g2 ? 128 : 64;
    std::vector<uint32_t> base;
    if (!g2) append_words(base, host_g1_generator()); else append_words(base, host_g2_generator());
    std::vector<uint32_t> offs; append_offset(offs, g2, 0); append_offset(offs, g2, 1);      // [O | -O]
    const G16Radix rx = g16_radix(10);           // one base point, thousands of scalars: a small table is plenty
    std::vector<uint32_t> dig((size_t)rx.digw * rows);
    for (uint32_t i = 0; i < rows; i++) {
        sc raw; fp_to_raw(raw.v, scalars[i]); uint32_t pk[G16_DIGW_MAX]; g16_recode(pk, raw, rx);
        for (uint32_t k = 0; k < rx.digw; k++) dig[(size_t)k * rows + i] = pk[k];
    }
    uint32_t *d_base = nullptr, *d_tab = nullptr, *d_dig = nullptr, *d_part = nullptr, *d_offs = nullptr, *d_sums = nullptr; uint8_t* d_out = nullptr;
    DevScope mem;
    HIP_TRY(mem.alloc(&d_base, AW * 4)); HIP_TRY(mem.alloc(&d_tab, (size_t)rx.slot_ent * g16_table_entry_words(g2, true) * 4 + 64)); HIP_TRY(mem.alloc(&d_dig, dig.size() * 4));
    HIP_TRY(mem.alloc(&d_part, (size_t)JW * 4 * rows)); HIP_TRY(mem.alloc(&d_sums, (size_t)JW * 4 * rows)); HIP_TRY(mem.alloc(&d_offs, offs.size() * 4));
    HIP_TRY(hipMemcpy(d_offs, offs.data(), offs.size() * 4, hipMemcpyHostToDevice)); HIP_TRY(mem.alloc(&d_out, (size_t)PB * rows));
    HIP_TRY(hipMemcpy(d_base, base.data(), AW * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_dig, dig.data(), dig.size() * 4, hipMemcpyHostToDevice));
    // one slot (base 0, digit row 0, every window of the radix) in one chunk of one target
    struct OneSlot { DevLayout d; ~OneSlot() { free_layout(d); } } lay;
    const GatherShape shape{rx.nent, rx.slot_ent, rx.uneven ? 1u : 0u, rx.digw};
    if (int rc = upload_layout(lay.d, make_layout_even({SlotList{{0, (uint8_t)rx.nwin}}}, 1), &shape)) return rc;
    g16_launch_build_table(g2, d_base, 1, d_tab, dev().stream, true, rx);
    g16_launch_msm(g2, msm_view(g16_table_shape(rx), lay.d, nullptr, d_tab, d_offs, rows, d_dig, d_part), dev().stream);
    g16_launch_sum(g2, reduce_view(lay.d, rows, d_part, d_offs + JW), d_sums, dev().stream);
    g16_launch_serialize(g2, d_sums, rows, d_out, dev().stream);
    out_bytes.resize((size_t)PB * rows);
    HIP_TRY(hipMemcpyAsync(out_bytes.data(), d_out, out_bytes.size(), hipMemcpyDeviceToHost, dev().stream));
    HIP_TRY(hipStreamSynchronize(dev().stream));
    return 0;
}

int generate_key_locked(int kind, const uint8_t* setup_seed, std::vector<uint8_t>& pk, std::vector<uint8_t>& vk) {
    if (kind != G16_EQUALITY && kind != G16_MEMBERSHIP) return fail(ZKP_HIP_E_ARGUMENT, "unknown circuit kind");
    const HostR1CS cs = kind == G16_EQUALITY ? build_equality_r1cs() : build_membership_r1cs();
    const HostCircuitTables T = build_circuit_tables(cs);
    uint32_t seed[8];
    if (setup_seed) memcpy(seed, setup_seed, 32);
    else { std::vector<uint8_t> f; int rc0 = fresh_seeds(f, 1); if (rc0) return rc0; memcpy(seed, f.data(), 32); }
    const char* tagname = kind == G16_EQUALITY ? "equality_mimc" : "membership_mimc";     // snark.rs:306,327 key prefixes
    uint8_t th[32]; sha256_host(th, (const uint8_t*)tagname, strlen(tagname));
    const uint32_t tag = (uint32_t)th[0] | ((uint32_t)th[1] << 8) | ((uint32_t)th[2] << 16);
    fr tw[5];
    for (uint32_t k = 0; k < 5; k++) { tw[k] = tape_fr(seed, 0x47313601u, 8 * tag + k); if (fp_is_zero(tw[k])) tw[k] = fp_one<FrParams>(); }
    const fr alpha = tw[0], beta = tw[1], gamma = tw[2], delta = tw[3], tau = tw[4];
    const uint32_t m = T.m, nv = T.nv;
    const fr one = fp_one<FrParams>();
    fr taum = one; for (uint32_t i = 0; i < m; i++) taum = fp_mul(taum, tau);
    const fr zt = fp_sub(taum, one), minv = fp_inv(fp_from_u64<FrParams>(m));
    const fr w = fr9_to_fr<FrParams>(ld_fr9_c(T.tw.data(), 1));      // the domain tables hold nine-limb elements (g16_circuit.h)
    std::vector<fr> lag(m);
    fr wj = one;
    for (uint32_t j = 0; j < m; j++) { lag[j] = fp_mul(fp_mul(fp_mul(zt, minv), wj), fp_inv(fp_sub(tau, wj))); wj = fp_mul(wj, w); }
    std::vector<fr> At(nv, fp_zero<FrParams>()), Bt = At, Ct = At;
    std::vector<fr>* dst[3] = {&At, &Bt, &Ct};
    for (int q = 0; q < 3; q++)
        for (uint32_t j = 0; j < T.n_rows; j++)
            for (uint32_t e = T.ptr[q][j]; e < T.ptr[q][j + 1]; e++)
                (*dst[q])[T.col[q][e]] = fp_add((*dst[q])[T.col[q][e]], fp_mul(ld_fr_c(T.coef[q].data(), e), lag[j]));
    for (uint32_t i = 0; i < T.n_inst; i++) At[i] = fp_add(At[i], lag[T.n_rows + i]);
    const fr ginv = fp_inv(gamma), dinv = fp_inv(delta);
    auto mix = [&](uint32_t k) { return fp_add(fp_add(fp_mul(beta, At[k]), fp_mul(alpha, Bt[k])), Ct[k]); };
    // G1 order: alpha, beta, delta | gamma_abc (n_inst) | a_query (nv) | b_g1_query (nv) | h_query (m-1) | l_query (n_wit)
    std::vector<fr> s1 = {alpha, beta, delta}, s2 = {beta, gamma, delta};
    for (uint32_t i = 0; i < T.n_inst; i++) s1.push_back(fp_mul(mix(i), ginv));
    for (uint32_t k = 0; k < nv; k++) s1.push_back(At[k]);
    for (uint32_t k = 0; k < nv; k++) s1.push_back(Bt[k]);
    { fr tp = fp_mul(zt, dinv); for (uint32_t i = 0; i + 1 < m; i++) { s1.push_back(tp); tp = fp_mul(tp, tau); } }
    for (uint32_t k = T.n_inst; k < nv; k++) s1.push_back(fp_mul(mix(k), dinv));
    for (uint32_t k = 0; k < nv; k++) s2.push_back(Bt[k]);
    std::vector<uint8_t> b1, b2; int rc;
    if ((rc = gpu_scalar_mults(false, s1, b1)) || (rc = gpu_scalar_mults(true, s2, b2))) return rc;
    auto g1at = [&](size_t i) { return b1.data() + 64 * i; };
    auto g2at = [&](size_t i) { return b2.data() + 128 * i; };
    auto put = [](std::vector<uint8_t>& v, const uint8_t* p, size_t n) { v.insert(v.end(), p, p + n); };
    auto put_len = [](std::vector<uint8_t>& v, uint64_t n) { for (int i = 0; i < 8; i++) v.push_back((uint8_t)(n >> (8 * i))); };
    size_t o_abc = 3, o_a = o_abc + T.n_inst, o_b = o_a + nv, o_h = o_b + nv, o_l = o_h + (m - 1);
    vk.clear();
    put(vk, g1at(0), 64); put(vk, g2at(0), 128); put(vk, g2at(1), 128); put(vk, g2at(2), 128);
    put_len(vk, T.n_inst); put(vk, g1at(o_abc), 64ull * T.n_inst);
    pk = vk;
    put(pk, g1at(1), 64); put(pk, g1at(2), 64);
    put_len(pk, nv); put(pk, g1at(o_a), 64ull * nv);
    put_len(pk, nv); put(pk, g1at(o_b), 64ull * nv);
    put_len(pk, nv); put(pk, g2at(3), 128ull * nv);
    put_len(pk, m - 1); put(pk, g1at(o_h), 64ull * (m - 1));
    put_len(pk, T.n_wit); put(pk, g1at(o_l), 64ull * T.n_wit);
    return load_key_locked(kind, pk.data(), pk.size());
}

int launch_msm_key(bool g2, const G16Radix& rx, const G16Key::Chunking& ch, const uint32_t* table, const uint32_t* acc_init, uint32_t rows, const uint32_t* digits, uint32_t* partial, hipStream_t st) {
    const DevLayout& D = ch.lay;
    const MsmView m = msm_view(g16_table_shape(rx), D, ch.scal, table, acc_init, rows, digits, partial);
    Device::KProf& K = dev().prof[g2 ? 2 : 1];
    hipEvent_t e1 = nullptr;
    int rc = prof_begin(K, st, &e1);
    if (rc) return rc;
    ZKP_TRACED(g2 ? "k_msm_gather<G2Msm>" : "k_msm_gather<G1Msm>", st, g16_launch_msm(g2, m, st));
    prof_end(K, st, e1, D.adds_per_row * rows);
    return 0;
}

// the batched prover for `rows` valid ops of one circuit kind; all pointers are device pointers

int run_g16(int kind, uint32_t rows, const uint64_t* d_value, const uint64_t* d_set_vals, const uint32_t* d_set_len, const uint8_t* d_seeds,
            uint8_t* d_out, uint64_t stride, hipStream_t st, uint32_t lane = 0) {
    G16Key& K = g16s().key[kind];
    if (!K.loaded) return no_proving_key(K);
    // The steps of one batch in dependency order on three streams, so that the latency-bound ones
    // (QAP, partial sums, the two scalar multiplications) sit beside an MSM instead of between two:
    //   st    : witness, z digits | MSM A,B1 | MSM B2 (G2) -> sum |                       final
    //   side  :                   | QAP (h digits) -> MSM l,h -> sum --------------------- ^
    //   side2 :                              | sums of A, B1 -> s*A, r*B1 -----------------^
    const G16Key::Chunking *c1 = nullptr, *c1c = nullptr, *c2 = nullptr;
    int rc;
    if ((rc = get_chunking(K, false, G16_PART_AB, rows, &c1)) || (rc = get_chunking(K, true, G16_PART_ALL, rows, &c2))) return rc;
    if ((rc = get_chunking(K, false, G16_PART_C, rows, &c1c))) return rc;
    const G16ProvePlan P = g16_prove_plan(rows, K.nv, K.m, K.rx.digw, c1->lay.nchunks, c1c->lay.nchunks, c2->lay.nchunks);      // prover_plan.h
    G16Run& RW = g16s().run[kind][lane & 1u];
    if ((rc = RW.buf.reserve(P.total))) return rc;
    G16View V{}; V.rx = K.rx; V.rows = rows; V.kind = (uint32_t)kind; V.n_inst = K.n_inst; V.n_wit = K.n_wit; V.nv = K.nv; V.m = K.m;
    V.value = d_value; V.set_vals = d_set_vals; V.set_len = d_set_len; V.seeds = reinterpret_cast<const uint32_t*>(d_seeds); V.mimc_c = g16s().mimc_dev; V.out = d_out; V.stride = stride;
    const G16ProveBufs B = g16_prove_bind(V, RW.buf.p, P);
    uint32_t *const p1 = B.p1, *const p1c = B.p1c, *const p2 = B.p2, *const s1 = B.s1, *const s2 = B.s2, *const t1 = B.t1;
    if (!RW.last) {
        for (auto& e : RW.ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&RW.last, hipEventDisableTiming));
    }
    G16Run& R0 = g16s().run[kind][0];          // the side streams are lane 0's for both lanes (see ensure_sub, zkp_hip.hip)
    if (!R0.side) {
        // The runtime multiplexes streams onto four hardware queues per priority level, and two streams on one queue run one after the
        // other (traced in round 2: the G2 MSM of a circuit queued behind its own k_g16_cparts).  With the lanes' streams created on
        // demand (batch_impl.inc) a shard proving one batch at a time has four streams of the least priority -- equality and
        // membership main + `side` (QAP, l/h MSM).  The two `side2` streams (s*A, r*B1: a latency-bound chain of a few waves that the
        // final assembly waits for) take the GREATEST level, which nothing else uses: 13.2-13.3 ms per 4096-op mixed batch against
        // 13.7-13.8 at the least level and 15.9 at the default level, where they share queues with the Bulletproofs chain.
        static const int side_level = env_int("ZKP_HIP_G16_SIDE_PRIORITY", 2), side2_level = env_int("ZKP_HIP_G16_SIDE2_PRIORITY", 0);
        HIP_TRY(hipStreamCreateWithPriority(&R0.side, hipStreamNonBlocking, stream_priority(side_level)));
        HIP_TRY(hipStreamCreateWithPriority(&R0.side2, hipStreamNonBlocking, stream_priority(side2_level)));
    }
    hipStream_t const side = R0.side, side2 = R0.side2;
    hipEvent_t ev_wit = RW.ev[0], ev_ab = RW.ev[1], ev_c = RW.ev[2], ev_cp = RW.ev[3];
    const ReduceView R2 = reduce_view(c2->lay, rows, p2, c2->corr);
    if (RW.used) HIP_TRY(hipStreamWaitEvent(st, RW.last, 0));
    ZKP_TRACED("k_g16_witness", st, g16_launch_witness(V, st));
    ZKP_TRACED("k_g16_zdigits", st, g16_launch_zdigits(V, st));
    HIP_TRY(hipEventRecord(ev_wit, st));
    // side: h, then the l / h part of C
    HIP_TRY(hipStreamWaitEvent(side, ev_wit, 0));
    { TraceMark tm_("k_g16_qap", side); HIP_TRY(g16_launch_qap(V, K.C, side)); }
    if ((rc = launch_msm_key(false, K.rx, *c1c, K.table_g1, K.init_g1, rows, V.sdig, p1c, side))) return rc;
    ZKP_TRACED("k_sum_t<G1Msm>", side, g16_launch_sum(false, reduce_view(c1c->lay, rows, p1c, c1c->corr), s1 + (size_t)2 * G1_JAC_W * rows, side));      // s1's third sum
    HIP_TRY(hipEventRecord(ev_c, side));
    // st: A and B1, whose sums the scalar multiplications on side2 wait for, then B2
    if ((rc = launch_msm_key(false, K.rx, *c1, K.table_g1, K.init_g1, rows, V.sdig, p1, st))) return rc;
    ReduceView Rab = reduce_view(c1->lay, rows, p1, c1->corr);
    // three slot lists A' | S | B1' are still TWO sums: A over the chunks [begin[0], begin[2]), B1 over [begin[1], begin[3]) -- S's chunks go into both
    if (c1->lay.ntargets == 3) { Rab.ntargets = 2; Rab.target_chunk_end = c1->lay.target_chunk_begin + 2; }
    // The partial sums of A / B1 feed only the scalar multiplications: they go to side2 with them, so that the G2 MSM -- which needs
    // neither -- follows the G1 MSM directly instead of queueing behind a latency-bound kernel that waits for registers beside the other
    // streams' gather waves (traced: 0.8-3.9 ms for a 0.2 ms kernel).
    HIP_TRY(hipEventRecord(ev_ab, st));
    HIP_TRY(hipStreamWaitEvent(side2, ev_ab, 0));
    ZKP_TRACED("k_sum_t<G1Msm>", side2, g16_launch_sum(false, Rab, s1, side2));
    ZKP_TRACED("k_g16_cparts", side2, g16_launch_cparts(V, s1, t1, side2));
    HIP_TRY(hipEventRecord(ev_cp, side2));
    if ((rc = launch_msm_key(true, K.rx, *c2, K.table_g2, K.init_g2, rows, V.sdig, p2, st))) return rc;
    ZKP_TRACED("k_sum_t<G2Msm>", st, g16_launch_sum(true, R2, s2, st));
    HIP_TRY(hipStreamWaitEvent(st, ev_c, 0));
    HIP_TRY(hipStreamWaitEvent(st, ev_cp, 0));
    ZKP_TRACED("k_g16_final", st, g16_launch_final(V, s1, s2, t1, st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(RW.last, st)); RW.used = true;
    return 0;
}

// host-buffer front end shared by equality and membership: validates, compacts the valid ops, runs, scatters
int prove_g16_host(int kind, uint64_t n, const uint64_t* values, const uint64_t* sets_flat, const uint32_t* set_counts, const std::vector<uint8_t>& valid,
                   const uint8_t* seeds, uint8_t* out, uint64_t stride, uint32_t* out_len, int32_t* status) {
    if (g16s().key[kind].verifier_only()) return no_proving_key(g16s().key[kind]);          // before anything is written or enqueued
    std::vector<uint64_t> v, sv; std::vector<uint32_t> sl, idx; std::vector<uint8_t> sd;
    size_t pos = 0; int any = 0;
    memset(out, 0, stride * n);
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t cnt = set_counts ? set_counts[i] : 0;
        if (valid[i]) {
            idx.push_back((uint32_t)i); v.push_back(values[i]);
            sd.insert(sd.end(), seeds + 32 * i, seeds + 32 * i + 32);
            if (kind == G16_MEMBERSHIP) { sl.push_back(cnt); for (uint32_t k = 0; k < G16_MAX_SET; k++) sv.push_back(k < cnt ? sets_flat[pos + k] : 0); }
            const uint32_t plen = kind == G16_EQUALITY ? EQUALITY_ENVELOPE_BYTES : (uint32_t)membership_envelope_bytes(cnt);
            if (plen > stride) return fail(ZKP_HIP_E_ARGUMENT, "stride too small for the proof envelope");
            out_len[i] = plen; status[i] = ZKP_HIP_OK;
        } else { out_len[i] = 0; status[i] = ZKP_HIP_INVALID_INPUT; any = 1; }
        pos += cnt;
    }
    const uint32_t rows = (uint32_t)idx.size();
    if (rows == 0) return any;
    hipStream_t st = dev().stream;
    uint64_t *d_v = nullptr, *d_sv = nullptr; uint32_t* d_sl = nullptr; uint8_t *d_sd = nullptr, *d_out = nullptr;
    DevScope mem;
    HIP_TRY(mem.alloc(&d_v, 8ull * rows)); HIP_TRY(mem.alloc(&d_sd, 32ull * rows)); HIP_TRY(mem.alloc(&d_out, stride * rows));
    HIP_TRY(hipMemcpyAsync(d_v, v.data(), 8ull * rows, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_sd, sd.data(), 32ull * rows, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_out, 0, stride * rows, st));
    if (kind == G16_MEMBERSHIP) {
        HIP_TRY(mem.alloc(&d_sv, 8ull * sv.size())); HIP_TRY(mem.alloc(&d_sl, 4ull * rows));
        HIP_TRY(hipMemcpyAsync(d_sv, sv.data(), 8ull * sv.size(), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_sl, sl.data(), 4ull * rows, hipMemcpyHostToDevice, st));
    }
    int rc = run_g16(kind, rows, d_v, d_sv, d_sl, d_sd, d_out, stride, st);
    std::vector<uint8_t> tmp;
    if (rc == 0) {
        tmp.resize(stride * rows);
        HIP_TRY(hipMemcpyAsync(tmp.data(), d_out, stride * rows, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t k = 0; k < rows; k++) memcpy(out + (uint64_t)idx[k] * stride, tmp.data() + (uint64_t)k * stride, stride);
    }
    if (rc) return rc;
    return any;
}

// everything the Groth16 part holds on the device (called by zkp_hip_shutdown)
void g16_release_all() {
    G16State* S = dev().g16;
    if (!S) return;
    for (auto& circuit : S->run) for (auto& W : circuit) {
        if (W.side) { (void)hipStreamDestroy(W.side); (void)hipStreamDestroy(W.side2); }
        if (W.last) { for (auto e : W.ev) (void)hipEventDestroy(e); (void)hipEventDestroy(W.last); }
        W.buf.release();
    }
    for (auto& K : S->key) release_key(K);
    if (S->mimc_dev) (void)hipFree(S->mimc_dev);
    g16_vm_free(S->vm);
    delete S; dev().g16 = nullptr;
}

// The per-envelope check of n envelopes that lie in device memory, verdicts into d_ok (and into ok, host memory, when it is given); waits for
// them.  The Fq2 machine (fq2vm.h) checks every envelope whose proof points are all finite; a batch that holds any other valid encoding (a
// point at infinity drops a pair from the product) goes through the lane-per-chain kernels as a whole, which handle those cases; use_vm = false
// takes the lane-per-chain kernels for everything.  `mem` owns the scratch; the caller holds a Quiesce behind it (zkp_hip.hip).
int verify_g16_device(int kind, G16Key& K, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, uint8_t* d_ok, uint8_t* ok, bool use_vm, DevScope& mem) {
    hipStream_t st = dev().stream;
    if (use_vm) {
        uint8_t* d_scratch = nullptr; uint32_t* d_special = nullptr; uint32_t special = 0;
        HIP_TRY(mem.alloc(&d_scratch, g16_vm_scratch_bytes(n))); HIP_TRY(mem.alloc(&d_special, 4));
        HIP_TRY(hipMemsetAsync(d_special, 0, 4, st));
        g16_launch_verify_vm(kind, d_in, stride, d_len, n, K.vk, g16s().vm, K.vm_kconst, K.vm_lines, d_scratch, d_ok, d_special, st);
        HIP_TRY(hipGetLastError());
        if (ok) HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(&special, d_special, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (!special) return 0;          // (the stream synchronisation above came after the chains' join)
    }
    uint8_t* d_scratch2 = nullptr;
    HIP_TRY(mem.alloc(&d_scratch2, g16_verify_scratch_bytes(n)));
    g16_launch_verify(kind, d_in, stride, d_len, n, K.vk, d_scratch2, d_ok, st);
    HIP_TRY(hipGetLastError());
    if (ok) HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// After a batch check of these n envelopes that did not stand (d_rlc: its scratch, d_ok / ok: its verdicts, on the device and on the host):
// one check per segment says where the bad envelopes can be (g16_localise.h), and only the suspect segments' envelopes get the per-envelope
// check.  *done = false: nothing was decided here and the caller verifies the whole batch (localisation switched off, or suspects in half of it).
int localise_g16(int kind, G16Key& K, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint32_t n, uint8_t* d_rlc, uint8_t* d_ok, uint8_t* ok,
                 const uint32_t counters[4], DevScope& mem, Tally& tally, bool* done) {
    *done = false;
    if (env_int("ZKP_HIP_G16_LOCALISE", 1) == 0) return 0;
    hipStream_t st = dev().stream;
    // no envelope with a point at infinity, none live outside the subgroup and none live inside it: every envelope was refused at the parse, and those verdicts stand
    if (counters[0] == 0 && counters[1] == 0 && std::all_of(ok, ok + n, [](uint8_t v) { return v == 0; })) { *done = true; return 0; }
    const int forced = env_int("ZKP_HIP_G16_LOCALISE_SEGMENT", 0);
    const G16Segments g = g16_loc_segments(n, forced > 0 ? (uint32_t)forced : 0u);
    const uint32_t n_ic = K.vk.n_ic;
    uint8_t* d_loc = nullptr;
    HIP_TRY(mem.alloc(&d_loc, g16_loc_scratch_bytes(g.count, n_ic)));
    std::vector<uint8_t> suspect(g.count);
    g16_launch_localise(kind, d_in, stride, d_len, n, g, K.vk, g16s().vm, K.vm_kconst, K.vm_lines, d_rlc, d_ok, d_loc, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(suspect.data(), d_loc, g.count, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tally[CTR_G16_SEGMENT_CHECKS] += g.count;
    std::vector<uint32_t> off((size_t)g.count + 1);
    const uint32_t m = g16_loc_offsets(g, n, suspect.data(), off.data());
    if (g16_loc_whole_batch(m, n)) return 0;
    *done = true;
    if (m == 0) return 0;          // (every segment's check stands: the batch check failed on an anomaly of its own virtual envelope)
    uint8_t *d_in2 = nullptr, *d_ok2 = nullptr; uint32_t* d_len2 = nullptr;
    uint32_t* d_off = reinterpret_cast<uint32_t*>(d_loc + g16_loc_offsets_offset(g.count, n_ic));
    HIP_TRY(mem.alloc(&d_in2, stride * m)); HIP_TRY(mem.alloc(&d_len2, 4ull * m)); HIP_TRY(mem.alloc(&d_ok2, m));
    HIP_TRY(hipMemcpyAsync(d_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice, st));
    g16_launch_compact(d_in, stride, d_len, n, g, d_loc, d_off, d_in2, d_len2, st);
    HIP_TRY(hipGetLastError());
    tally[CTR_G16_ENVELOPES] += m;
    int rc = verify_g16_device(kind, K, d_in2, stride, d_len2, m, d_ok2, nullptr, true, mem);
    if (rc) return rc;
    g16_launch_scatter(n, g, d_loc, d_off, d_ok2, d_ok, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// ZKP_HIP_G16_BATCH_VERIFY_MIN: measured crossover, a single round of the per-envelope chains (<= 8192 envelopes) is faster than the batch check (profiles/r04_verify_g16_batch.json)
int g16_rlc_min() { static const int v = env_int("ZKP_HIP_G16_BATCH_VERIFY_MIN", 8193); return v; }

// Verdicts of n envelopes that lie in device memory (d_in, `stride` bytes each, d_len[i] bytes used) into d_ok (device) and ok (host, n bytes:
// the localisation pass reads the batch check's verdicts there): one weighted pairing check for a large batch (g16_rlc.h); when it does not
// stand, the localisation pass and the per-envelope check of the suspect envelopes, or of all of them.  ZKP_HIP_G16_VERIFY_VM=0 (tuning / test
// knob) takes the lane-per-chain kernels for everything.  `mem` owns the scratch.  The chains run on side streams against that scratch: after
// a failure (a non-zero return) the caller waits for the whole device before `mem` hands its blocks back (Quiesce, zkp_hip.hip).
int verify_g16_core(int kind, uint64_t n, const uint8_t* d_in, uint64_t stride, const uint32_t* d_len, uint8_t* d_ok, uint8_t* ok, DevScope& mem) {
    G16Key& K = g16s().key[kind];
    if (!K.vk_ready) return fail(ZKP_HIP_E_ARGUMENT, "no (usable) key loaded for this circuit (zkp_hip_groth16_load_key)");
    hipStream_t st = dev().stream;
    static const int use_vm = env_int("ZKP_HIP_G16_VERIFY_VM", 1);
    std::unique_ptr<Tally> tally;          // ZKP_HIP_COUNTER_G16_VERIFY: made once a batch check has not stood, added when the call returns, whichever way
    if (use_vm) {
        G16VmTables& T = g16s().vm;
        if (!T.ready) {
            const int urc = g16_vm_upload(T);
            if (urc == -2) return fail(ZKP_HIP_E_RUNTIME, "hipFuncSetAttribute: the device refused the 160 KB dynamic LDS that the Groth16 verifier's Fq2 machine needs");
            if (urc) return fail(ZKP_HIP_E_RUNTIME, "could not place the verifier's tables in device memory");
        }
        // Large batches: one pairing check for all of them (g16_rlc.h) -- one Miller loop, one subgroup check and two 128-bit scalar
        // multiplications per envelope, the loops on gamma / delta and the final exponentiation once.  Its verdicts stand when the batch's
        // product is one and no envelope needs the per-envelope treatment; otherwise (a tampered envelope, a point at infinity) the suspect
        // envelopes, or all of them, are verified again envelope by envelope below, so the answer is always the per-envelope one.
        const int rlc_min = g16_rlc_min();
        if (rlc_min > 0 && n >= (uint64_t)rlc_min && !getenv("ZKP_HIP_NO_BATCH_VERIFY")) {
            const uint32_t n_ic = K.vk.n_ic;
            uint8_t* d_rlc = nullptr;
            HIP_TRY(mem.alloc(&d_rlc, g16_rlc_scratch_bytes((uint32_t)n, n_ic)));
            std::vector<uint8_t> rnd; { int rcs = fresh_seeds(rnd, (n + 1) / 2); if (rcs) return rcs; }          // 16 bytes per envelope
            for (uint64_t j = 0; j < n; j++) { bool z = true; for (int k = 0; k < 16; k++) z = z && rnd[16 * j + k] == 0; if (z) rnd[16 * j] = 1; }
            uint32_t counters[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(d_rlc + g16_rlc_rho_offset((uint32_t)n, n_ic), rnd.data(), 16 * n, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemsetAsync(d_rlc + g16_rlc_counters_offset((uint32_t)n, n_ic), 0, sizeof counters, st));
            g16_launch_verify_rlc(kind, d_in, stride, d_len, (uint32_t)n, K.vk, T, K.vm_kconst, K.vm_lines, d_rlc, d_ok, st);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(counters, d_rlc + g16_rlc_counters_offset((uint32_t)n, n_ic), sizeof counters, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ok, d_ok, n, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (counters[0] == 0 && counters[1] == 0 && counters[2] == 0 && counters[3] == 1) return 0;
            if (getenv("ZKP_HIP_G16_BATCH_VERIFY_ONLY")) {          // diagnostic (tests): say that the batch check did not stand instead of verifying again
                char msg[160]; snprintf(msg, sizeof msg, "the batch check did not stand (special %u, outside the subgroup %u, anomalies %u, product is one: %u)", counters[0], counters[1], counters[2], counters[3]);
                return fail(ZKP_HIP_E_RUNTIME, msg);
            }
            tally.reset(new Tally(dev().counters, FAM_G16_VERIFY));
            bool done = false;
            const int rc = localise_g16(kind, K, d_in, stride, d_len, (uint32_t)n, d_rlc, d_ok, ok, counters, mem, *tally, &done);
            if (rc) return rc;
            if (done) return 0;
            (*tally)[CTR_G16_ENVELOPES] += n;
        }
    }
    return verify_g16_device(kind, K, d_in, stride, d_len, (uint32_t)n, d_ok, ok, use_vm != 0, mem);
}

// the batch-check threshold in force (ZKP_HIP_G16_BATCH_VERIFY_MIN) as the minimum slice of a fanned-out call
uint64_t g16_min_slice() { const int v = g16_rlc_min(); return v > 0 ? (uint64_t)v : 8193u; }
bool g16_shard_holds_vk(Device* d, int kind) { std::lock_guard<std::mutex> lk(d->mu); return d->g16 && d->g16->key[kind].vk_ready; }

// one slice of a host-buffer call on the bound shard: upload, then the core above
int verify_g16_host(int kind, uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, uint8_t* ok) {
    if (!g16s().key[kind].vk_ready) return fail(ZKP_HIP_E_ARGUMENT, "no (usable) key loaded for this circuit (zkp_hip_groth16_load_key)");
    EnvelopeUpload up;
    Quiesce quiesce;
    int rc = up.open(n, proofs, stride, lens);
    if (rc || (rc = verify_g16_core(kind, n, up.d_in, stride, up.d_len, up.d_ok, ok, up.mem))) return rc;
    quiesce.armed = false;
    return 0;
}
// The two host-buffer entry points after their argument checks.  Spread over the registered shards that hold a usable key of `kind`
// (verify_call), every slice draws its own weights and makes its own batch check.  A caller's shard without the key: not fanned, and the usual
// path reports the missing key.
int verify_g16_call(int kind, uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, uint8_t* ok) {
    return verify_call(n,
        [&](const std::vector<Device*>& shards, VerifyFanout& F) {
            for (Device* d : shards) F.holds.push_back(g16_shard_holds_vk(d, kind));
            F.min_jobs = g16_min_slice();
            return 0;
        },
        [&](uint64_t lo, uint64_t m) { return verify_g16_host(kind, m, proofs + stride * lo, stride, lens + lo, ok + lo); });
}

}  // namespace

// ================================================================================================ C ABI (Groth16 part)
extern "C" {

// every registered shard but `skip` gets the key (its tables are built on that shard's GPU, the shards in parallel)
static int load_key_all_shards(int kind, const uint8_t* pk, uint64_t len, Device* skip) {
    std::vector<Device*> todo;
    {
        Device* d0 = nullptr; int rc = find_shard(0, &d0);
        if (rc) return rc;
        Registry& R = registry(); std::lock_guard<std::mutex> lk(R.mu);
        for (Device* d : R.shards) if (d != skip) todo.push_back(d);
    }
    return for_each_device(todo, [&](size_t) { return load_key_locked(kind, pk, len); });
}

int zkp_hip_groth16_load_key(int kind, const uint8_t* pk, uint64_t len) try {
    if (!pk) return fail(ZKP_HIP_E_ARGUMENT, "null proving key");
    return load_key_all_shards(kind, pk, len, nullptr);
} ZKP_API_CATCH_INT

int zkp_hip_groth16_key_info(int kind, uint32_t* wbits, uint32_t* uneven, uint64_t* table_bytes) try {
    if (kind != G16_EQUALITY && kind != G16_MEMBERSHIP && kind != ZKP_HIP_TABLES_BP_GENERATORS) return fail(ZKP_HIP_E_ARGUMENT, "unknown circuit kind");
    Bind bind; int rc = bind.open();
    if (rc) return rc;
    if (kind == ZKP_HIP_TABLES_BP_GENERATORS) {          // the shard's Bulletproofs generator tables (zeros while ZKP_HIP_ED_TABLES=lazy has not built them)
        const EdgGeom& g = dev().edg;
        if (wbits) *wbits = g.wbits;
        if (uneven) *uneven = 0;
        if (table_bytes) *table_bytes = dev().d_edg_table ? (uint64_t)edg_table_words(g) * 4 : 0;
        return 0;
    }
    const G16Key& K = g16s().key[kind];
    if (K.verifier_only()) {          // no MSM tables: the gamma_abc_g1 window tables are all the key holds
        if (wbits) *wbits = G16V_WBITS;
        if (uneven) *uneven = 0;
        if (table_bytes) *table_bytes = K.vk_table_bytes;
        return 0;
    }
    if (!K.loaded) return fail(ZKP_HIP_E_ARGUMENT, "no proving key loaded for this circuit (zkp_hip_groth16_load_key)");
    if (wbits) *wbits = K.rx.wbits;
    if (uneven) *uneven = K.rx.uneven ? 1u : 0u;
    if (table_bytes) *table_bytes = K.table_bytes;
    return 0;
} ZKP_API_CATCH_INT

// ---- include/libzkp_hip_keycheck.h
int zkpkeycheck_key(int kind, const uint8_t* key, uint64_t len, uint32_t what, zkp_keycheck_report* report) try {
    if (kind != G16_EQUALITY && kind != G16_MEMBERSHIP) return fail(ZKP_HIP_E_ARGUMENT, "unknown circuit kind");
    if (!key || !report) return fail(ZKP_HIP_E_ARGUMENT, "null pointer argument");
    if (what & ~(ZKP_KEYCHECK_POINTS | ZKP_KEYCHECK_TWINS | ZKP_KEYCHECK_TABLES)) return fail(ZKP_HIP_E_ARGUMENT, "unknown ZKP_KEYCHECK_* stage");
    Bind bind; int rc = bind.open();
    if (rc) return rc;
    return keycheck_locked(kind, key, len, what, *report);
} ZKP_API_CATCH_INT

int zkpkeycheck_counters(double* ms, uint64_t* loads_checked, uint64_t* entries_checked, uint64_t* refused, int reset) try {
    return read_counters(FAM_KEY_CHECK, ms, {loads_checked, entries_checked, refused}, reset);
} ZKP_API_CATCH_INT

int zkp_hip_groth16_generate_key(int kind, const uint8_t* setup_seed, uint8_t* pk_out, uint64_t pk_cap, uint64_t* pk_len,
                                 uint8_t* vk_out, uint64_t vk_cap, uint64_t* vk_len) try {
    std::vector<uint8_t> pk, vk;
    Device* here = nullptr;
    {
        Bind bind; int rc = bind.open();
        if (rc) return rc;
        here = &dev();
        if ((rc = generate_key_locked(kind, setup_seed, pk, vk))) return rc;
    }
    int rc = load_key_all_shards(kind, pk.data(), pk.size(), here);       // ONE trusted setup for every GPU
    if (rc) return rc;
    if (pk_len) *pk_len = pk.size();
    if (vk_len) *vk_len = vk.size();
    if (pk_out) { if (pk_cap < pk.size()) return fail(ZKP_HIP_E_ARGUMENT, "pk buffer too small"); memcpy(pk_out, pk.data(), pk.size()); }
    if (vk_out) { if (vk_cap < vk.size()) return fail(ZKP_HIP_E_ARGUMENT, "vk buffer too small"); memcpy(vk_out, vk.data(), vk.size()); }
    return 0;
} ZKP_API_CATCH_INT

int zkp_hip_verify_equality_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, ok}, stride);
    return rc ? rc : verify_g16_call(G16_EQUALITY, n, proofs, stride, lens, ok);
} ZKP_API_CATCH_INT
int zkp_hip_verify_membership_batch(uint64_t n, const uint8_t* proofs, uint64_t stride, const uint32_t* lens, uint8_t* ok) try {
    if (n == 0) return 0;
    const int rc = verifier_args(n, {proofs, lens, ok}, stride);
    return rc ? rc : verify_g16_call(G16_MEMBERSHIP, n, proofs, stride, lens, ok);
} ZKP_API_CATCH_INT

int zkp_hip_snark_commit_value_batch(uint64_t n, const uint64_t* values, uint8_t* out) try {
    if (n == 0) return 0;
    Bind bind; int rc = host_args(n, {values, out});
    if (rc || (rc = bind.open())) return rc;
    if ((rc = ensure_mimc_dev())) return rc;
    uint64_t* d_v = nullptr; uint8_t* d_o = nullptr;
    DevScope mem;
    HIP_TRY(mem.alloc(&d_v, 8 * n)); HIP_TRY(mem.alloc(&d_o, 32 * n));
    HIP_TRY(hipMemcpyAsync(d_v, values, 8 * n, hipMemcpyHostToDevice, dev().stream));
    g16_launch_mimc(d_v, (uint32_t)n, g16s().mimc_dev, d_o, dev().stream);
    HIP_TRY(hipMemcpyAsync(out, d_o, 32 * n, hipMemcpyDeviceToHost, dev().stream));
    HIP_TRY(hipStreamSynchronize(dev().stream));
    return 0;
} ZKP_API_CATCH_INT

int zkp_hip_prove_equality_batch(uint64_t n, const uint64_t* val1, const uint64_t* val2, const uint8_t* seeds,
                                 uint8_t* out, uint64_t stride, uint32_t* out_len, int32_t* status) try {
    if (n == 0) return 0;
    std::vector<uint8_t> fresh;
    int rc = prover_args(fresh, seeds, n, {val1, val2, out, out_len, status}, nullptr, stride, EQUALITY_ENVELOPE_BYTES, "stride must be >= 298");
    if (rc) return rc;
    std::vector<uint8_t> valid(n);
    for (uint64_t i = 0; i < n; i++) valid[i] = equality_ok(val1[i], val2[i]);
    Bind bind;
    if ((rc = bind.open())) return rc;
    return prove_g16_host(G16_EQUALITY, n, val1, nullptr, nullptr, valid, seeds, out, stride, out_len, status);
} ZKP_API_CATCH_INT

int zkp_hip_prove_membership_batch(uint64_t n, const uint64_t* values, const uint64_t* sets, const uint32_t* set_counts, const uint8_t* seeds,
                                   uint8_t* out, uint64_t stride, uint32_t* out_len, int32_t* status) try {
    if (n == 0) return 0;
    std::vector<uint8_t> fresh;
    int rc = prover_args(fresh, seeds, n, {values, sets, set_counts, out, out_len, status}, set_counts);
    if (rc) return rc;
    std::vector<uint8_t> valid(n);
    for (uint64_t i = 0, pos = 0; i < n; pos += set_counts[i++]) valid[i] = membership_ok(values[i], sets + pos, set_counts[i]);
    Bind bind;
    if ((rc = bind.open())) return rc;
    return prove_g16_host(G16_MEMBERSHIP, n, values, sets, set_counts, valid, seeds, out, stride, out_len, status);
} ZKP_API_CATCH_INT

}  // extern "C"
