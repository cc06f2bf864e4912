// Which envelopes of a Bulletproofs batch (range, threshold, consistency) are bad, when the batch check (bp_verify.h: RlcView) does not
// stand: the planning and the per-lane steps of the segment kernel, shared by the host (bpv_impl.inc), the kernels (bpv_kernels.hip:
// k_bp_seg_*, k_bp_gather, k_bp_scatter) and the host build of tests/emul/emul_bp_localise.cpp.
//
// The batch is cut into contiguous segments of `size` envelopes (the last one partial), so an envelope's jobs never straddle two
// segments.  Every segment gets the batch check's sum over its own jobs only, from what the failed check left in device memory under the
// same weights: the Niels rows and signed radix-2^11 digits of the weighted proof points (RlcView::niels, ::dig) and the weighted
// generator coefficients (VfyView::fterm).  Nothing is decoded, replayed or drawn again.  The jobs of the suspect segments are compacted
// into dense arrays, in order, go through the per-job pass, and their encodings are scattered back; every other job keeps the all-zero
// encoding of an accepted batch.  When the suspects hold half of the batch's jobs or more the whole batch is verified where it lies.
//
// Soundness: a segment's sum uses only its own jobs' weights, which are independent 128-bit draws, so a segment that holds a job whose
// combination is not the identity passes its check with probability at most 2^-128.  With the batch check itself a call (or a slice of a
// fanned-out call) errs with probability at most (1 + segments) * 2^-128.
#pragma once
#include "bp_verify.h"

namespace zkp {

constexpr uint32_t BP_LOC_MAX_SEGMENTS = 1024;         // segment checks of one pass: 24 waves each in k_bp_seg_points, one row each in the generator MSM
constexpr uint32_t BP_LOC_SEGMENT_QUANTUM = 16;        // default sizes are multiples of this many envelopes ...
constexpr uint32_t BP_LOC_SEGMENT_MIN = 32;            // ... and at least this (profiles/bp_localise.json: smaller segments cost more checks than they save jobs)

struct BpSegments { uint32_t size, count; };

// default size: about n / 256 (ZKP_HIP_BP_LOCALISE_SEGMENT overrides it)
ZKP_HD inline uint32_t bp_loc_default_size(uint32_t n) {
    const uint32_t q = BP_LOC_SEGMENT_QUANTUM, want = (uint32_t)(((uint64_t)n + 255) / 256);
    const uint32_t size = (want + q - 1) / q * q;
    return size < BP_LOC_SEGMENT_MIN ? BP_LOC_SEGMENT_MIN : size;
}
// the segments of n envelopes for a wanted size (0: the default), the size raised until there are at most BP_LOC_MAX_SEGMENTS of them
ZKP_HD inline BpSegments bp_loc_segments(uint32_t n, uint32_t want) {
    uint32_t size = want ? want : bp_loc_default_size(n);
    const uint32_t least = (uint32_t)(((uint64_t)n + BP_LOC_MAX_SEGMENTS - 1) / BP_LOC_MAX_SEGMENTS);
    if (size < least) size = least;
    return BpSegments{size, (uint32_t)(((uint64_t)n + size - 1) / size)};
}
// segment s holds the envelopes [lo, hi)
ZKP_HD inline uint32_t bp_loc_lo(const BpSegments& g, uint32_t s) { return s * g.size; }
ZKP_HD inline uint32_t bp_loc_hi(const BpSegments& g, uint32_t n, uint32_t s) { const uint64_t h = ((uint64_t)s + 1) * g.size; return h < n ? (uint32_t)h : n; }
ZKP_HD inline uint32_t bp_loc_segment_of(const BpSegments& g, uint32_t env) { return env / g.size; }
// ... and the jobs [job_lo, job_hi): jobs_per of them per envelope (2: range, 1: threshold), or, with job_base (n + 1 entries, consistency),
// a count of its own per envelope, which may be zero
ZKP_HD inline uint32_t bp_loc_first_job(uint32_t env, uint32_t jobs_per, const uint32_t* job_base) { return job_base ? job_base[env] : jobs_per * env; }
ZKP_HD inline uint32_t bp_loc_job_lo(const BpSegments& g, uint32_t s, uint32_t jobs_per, const uint32_t* job_base) { return bp_loc_first_job(bp_loc_lo(g, s), jobs_per, job_base); }
ZKP_HD inline uint32_t bp_loc_job_hi(const BpSegments& g, uint32_t n, uint32_t s, uint32_t jobs_per, const uint32_t* job_base) { return bp_loc_first_job(bp_loc_hi(g, n, s), jobs_per, job_base); }
// Compaction plan: off[s] = jobs of suspect segments before segment s (count + 1 entries); returns off[count], the jobs to verify again.
ZKP_HD inline uint32_t bp_loc_offsets(const BpSegments& g, uint32_t n, uint32_t jobs_per, const uint32_t* job_base, const uint8_t* suspect, uint32_t* off) {
    uint32_t total = 0;
    for (uint32_t s = 0; s < g.count; s++) { off[s] = total; if (suspect[s]) total += bp_loc_job_hi(g, n, s, jobs_per, job_base) - bp_loc_job_lo(g, s, jobs_per, job_base); }
    off[g.count] = total;
    return total;
}
// where job j of the suspect segment s lies in the compact arrays (gather: compact[dst] = batch[j]; scatter: batch[j] = compact[dst])
ZKP_HD inline uint32_t bp_loc_compact_index(const uint32_t* off, uint32_t s, uint32_t job_lo, uint32_t j) { return off[s] + (j - job_lo); }
// suspects hold at least half of the batch's jobs: the compact pass would save less than it copies -- verify the batch where it lies
ZKP_HD inline bool bp_loc_whole_batch(uint32_t suspect_jobs, uint32_t M) { return 2 * (uint64_t)suspect_jobs >= M; }

// what the kernels need of the plan
struct BpLocView {
    BpSegments g; uint32_t n, jobs_per;
    const uint32_t* job_base;      // device copy (VfyView::job_base) or null
    const uint8_t* suspect;        // [count]
    const uint32_t* off;           // [count + 1] (gather / scatter)
};

// ------------------------------------------------------------------------------------------------ the segment kernel's steps
// sum_i d_i P_i over the 17 * jobs point terms of one segment in one window, by one wave (k_bp_seg_points; here lane by lane).  A digit's
// magnitude m <= 1024 is split as 32 h + l: lane l (1..31) sums the points with that low part, lane 31 + h (h = 1..32) those with that high
// part, each with the digit's sign, and the window's sum is 32 * sum_h h B_{31 + h} + sum_l l B_l.  The points of a tile of at most
// BP_LOC_TILE_JOBS jobs are counting-sorted by lane (count, scan, place), then every lane walks its own run with one mixed addition per
// point; a longer segment is walked tile by tile, the lanes' sums carried across.  About two mixed additions per point and window.
constexpr uint32_t BP_LOC_LANES = 64, BP_LOC_TILE_JOBS = 64, BP_LOC_TILE_POINTS = VP_NUM * BP_LOC_TILE_JOBS;
static_assert(RLC_NBUCKET == 32 * 32 && BP_LOC_TILE_POINTS < (1u << 15), "32 h + l with h <= 32; a list entry is a tile index and a sign in 16 bits");
struct BpLocTile {
    uint32_t cursor[BP_LOC_LANES];         // counts, then scatter cursors
    uint32_t start[BP_LOC_LANES + 1];      // exclusive prefix sums of the counts
    uint16_t list[2 * BP_LOC_TILE_POINTS]; // tile index | sign << 15, grouped by lane (a point is in at most two runs)
};
ZKP_HD inline uint32_t bp_loc_bump(uint32_t* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return atomicAdd(p, 1u);
#else
    return (*p)++;
#endif
}
// lanes of digit d (0: none)
ZKP_HD inline void bp_loc_split(int32_t d, uint32_t& lane_l, uint32_t& lane_h) {
    const uint32_t m = (uint32_t)(d < 0 ? -d : d), h = m >> 5;
    lane_l = m & 31u; lane_h = h ? 31u + h : 0u;
}
// tile index e of a tile of nj jobs from job j0 on -> index of the point term in RlcView (p * M + job)
ZKP_HD inline uint32_t bp_loc_point(uint32_t e, uint32_t j0, uint32_t nj, uint32_t M) { return (e / nj) * M + j0 + e % nj; }
// lane t: count (place = false) or place the tile's points e = t, t + 64, ...
ZKP_HD inline void bp_loc_step_sort(BpLocTile& T, const RlcView& R, uint32_t M, uint32_t w, uint32_t j0, uint32_t nj, uint32_t t, bool place) {
    for (uint32_t e = t; e < VP_NUM * nj; e += BP_LOC_LANES) {
        const int32_t d = R.dig[(size_t)w * R.N + bp_loc_point(e, j0, nj, M)];
        uint32_t ll, lh; bp_loc_split(d, ll, lh);
        const uint16_t entry = (uint16_t)(e | (d < 0 ? 0x8000u : 0u));
        if (ll) { const uint32_t pos = bp_loc_bump(&T.cursor[ll]); if (place) T.list[pos] = entry; }
        if (lh) { const uint32_t pos = bp_loc_bump(&T.cursor[lh]); if (place) T.list[pos] = entry; }
    }
}
// one lane, between the two: counts -> starts, cursors at the starts
ZKP_HD inline void bp_loc_step_scan(BpLocTile& T) {
    uint32_t run = 0;
    for (uint32_t b = 0; b < BP_LOC_LANES; b++) { const uint32_t c = T.cursor[b]; T.start[b] = run; T.cursor[b] = run; run += c; }
    T.start[BP_LOC_LANES] = run;
}
// lane t: add the points of its run to its sum
ZKP_HD inline ge bp_loc_step_walk(ge acc, const BpLocTile& T, const RlcView& R, uint32_t M, uint32_t j0, uint32_t nj, uint32_t t) {
    for (uint32_t k = T.start[t]; k < T.start[t + 1]; k++) {
        const uint32_t entry = T.list[k];
        acc = msm_accumulate_digit(acc, (entry >> 15) ? -1 : 1, R.niels + (size_t)bp_loc_point(entry & 0x7fffu, j0, nj, M) * RLC_NIELS_W);
    }
    return acc;
}
// the window's sum from the 64 lanes' sums (the kernel forms the same by suffix sums across lanes): running sums from the top lane down
ZKP_HD inline ge bp_loc_combine(const ge* B) {
    ge run = ge_identity(), H = ge_identity(), L = ge_identity();
    for (uint32_t b = 63; b >= 32; b--) { run = ge_add(run, B[b]); H = ge_add(H, run); }
    run = ge_identity();
    for (uint32_t b = 31; b >= 1; b--) { run = ge_add(run, B[b]); L = ge_add(L, run); }
    for (int k = 0; k < 5; k++) H = ge_dbl(H);
    return ge_add(H, L);
}

}  // namespace zkp
