// Which envelopes of a Groth16 batch are bad, when the batch check (g16_rlc.h) does not stand: the planning, pure index arithmetic shared by
// the host (g16_impl.inc), the kernels (fq2vm_kernels.hip: k_g16_seg_*) and the host build of tests/emul/emul_g16_localise.cpp.
//
// The batch is cut into contiguous segments of `size` envelopes (the last one partial); every segment gets a batch check of its own --
// a virtual envelope per segment, lane = segment in the Fq2 machine -- from what the failed check left in device memory.  The envelopes of
// the suspect segments are compacted into a dense buffer, in order, go through the per-envelope check, and their verdicts are scattered
// back; everybody else keeps the batch pass's verdict.  When the suspects are half of the batch or more the whole batch is verified
// envelope by envelope where it lies.
#pragma once
#include "zkp_common.h"

namespace zkp {

constexpr uint32_t G16_LOC_MAX_SEGMENTS = 8192;          // virtual envelopes of one localisation pass: 256 workgroups of the machine's chain A, one per CU
constexpr uint32_t G16_LOC_SEGMENT_QUANTUM = 64;         // default sizes are multiples of the lane count of the kernels that walk a segment

struct G16Segments { uint32_t size, count; };

// default size: about n / 256 (ZKP_HIP_G16_LOCALISE_SEGMENT overrides it)
ZKP_HD inline uint32_t g16_loc_default_size(uint32_t n) {
    const uint32_t q = G16_LOC_SEGMENT_QUANTUM, want = (uint32_t)(((uint64_t)n + 255) / 256);
    return want <= q ? q : (want + q - 1) / q * q;
}
// the segments of n envelopes for a wanted size (0: the default), the size raised until there are at most G16_LOC_MAX_SEGMENTS of them
ZKP_HD inline G16Segments g16_loc_segments(uint32_t n, uint32_t want) {
    uint32_t size = want ? want : g16_loc_default_size(n);
    const uint32_t least = (uint32_t)(((uint64_t)n + G16_LOC_MAX_SEGMENTS - 1) / G16_LOC_MAX_SEGMENTS);
    if (size < least) size = least;
    return G16Segments{size, (uint32_t)(((uint64_t)n + size - 1) / size)};
}
// segment s holds the envelopes [lo, hi)
ZKP_HD inline uint32_t g16_loc_lo(const G16Segments& g, uint32_t s) { return s * g.size; }
ZKP_HD inline uint32_t g16_loc_hi(const G16Segments& g, uint32_t n, uint32_t s) { const uint64_t h = ((uint64_t)s + 1) * g.size; return h < n ? (uint32_t)h : n; }
ZKP_HD inline uint32_t g16_loc_segment_of(const G16Segments& g, uint32_t j) { return j / g.size; }
// Compaction plan: off[s] = envelopes of suspect segments before segment s (count + 1 entries); returns off[count], the envelopes to verify again.
ZKP_HD inline uint32_t g16_loc_offsets(const G16Segments& g, uint32_t n, const uint8_t* suspect, uint32_t* off) {
    uint32_t total = 0;
    for (uint32_t s = 0; s < g.count; s++) { off[s] = total; if (suspect[s]) total += g16_loc_hi(g, n, s) - g16_loc_lo(g, s); }
    off[g.count] = total;
    return total;
}
// where envelope j of a suspect segment lies in the compacted buffer (gather: compact[dst] = batch[j]; scatter: verdict[j] = compact_verdict[dst])
ZKP_HD inline uint32_t g16_loc_compact_index(const G16Segments& g, const uint32_t* off, uint32_t j) { const uint32_t s = g16_loc_segment_of(g, j); return off[s] + (j - g16_loc_lo(g, s)); }
// suspects cover at least half of the batch: compaction saves less than a round of the machine and costs a copy -- verify the batch where it lies
ZKP_HD inline bool g16_loc_whole_batch(uint32_t suspects, uint32_t n) { return 2 * (uint64_t)suspects >= n; }

}  // namespace zkp
