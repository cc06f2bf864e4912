// TEST INFRASTRUCTURE: host build of the Groth16 batch verifier's localisation planning (g16_localise.h): segment bounds, the cap on the
// number of segments, suspect flags -> compaction offsets, gather / scatter through those offsets as the kernels index them, and the
// half-of-the-batch rule.
#include "../../libzkp_amd/csrc/g16_localise.h"
using namespace zkp;

extern "C" {
uint32_t emul_g16_loc_default_size(uint32_t n) { return g16_loc_default_size(n); }
uint32_t emul_g16_loc_max_segments(void) { return G16_LOC_MAX_SEGMENTS; }
// out[0] = segment size, out[1] = number of segments
void emul_g16_loc_segments(uint32_t n, uint32_t want, uint32_t out[2]) { const G16Segments g = g16_loc_segments(n, want); out[0] = g.size; out[1] = g.count; }
// lo[s], hi[s] for every segment
void emul_g16_loc_bounds(uint32_t n, uint32_t want, uint32_t* lo, uint32_t* hi) {
    const G16Segments g = g16_loc_segments(n, want);
    for (uint32_t s = 0; s < g.count; s++) { lo[s] = g16_loc_lo(g, s); hi[s] = g16_loc_hi(g, n, s); }
}
uint32_t emul_g16_loc_segment_of(uint32_t n, uint32_t want, uint32_t j) { return g16_loc_segment_of(g16_loc_segments(n, want), j); }
uint32_t emul_g16_loc_offsets(uint32_t n, uint32_t want, const uint8_t* suspect, uint32_t* off) { return g16_loc_offsets(g16_loc_segments(n, want), n, suspect, off); }
// compact[dst] = batch[j] for every envelope j of a suspect segment (k_g16_seg_gather's placement, one 32-bit word per envelope)
void emul_g16_loc_gather(uint32_t n, uint32_t want, const uint8_t* suspect, const uint32_t* off, const uint32_t* batch, uint32_t* compact) {
    const G16Segments g = g16_loc_segments(n, want);
    for (uint32_t j = 0; j < n; j++) if (suspect[g16_loc_segment_of(g, j)]) compact[g16_loc_compact_index(g, off, j)] = batch[j];
}
// batch[j] = compact[dst] for the same envelopes (k_g16_seg_scatter); the others are left as they are
void emul_g16_loc_scatter(uint32_t n, uint32_t want, const uint8_t* suspect, const uint32_t* off, const uint32_t* compact, uint32_t* batch) {
    const G16Segments g = g16_loc_segments(n, want);
    for (uint32_t j = 0; j < n; j++) if (suspect[g16_loc_segment_of(g, j)]) batch[j] = compact[g16_loc_compact_index(g, off, j)];
}
int emul_g16_loc_whole_batch(uint32_t suspects, uint32_t n) { return g16_loc_whole_batch(suspects, n) ? 1 : 0; }
}
