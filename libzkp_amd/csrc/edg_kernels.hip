// ed25519 fixed-base MSM over HBM-resident radix-2^10 .. 2^16 tables (edg.h) and the kernels that build those tables: a translation unit of
// its own so that the Bulletproofs host code and the Groth16 kernels need not recompile with it.
#include "edg_launch.h"
#include "msm_kernel.h"

struct EdGather {      // edwards25519, affine-Niels entries gathered per lane from HBM, extended-coordinate accumulator
    static constexpr uint32_t ACC_W = GE_W, DIG_PER_WORD = 2;
    static __device__ __forceinline__ int32_t digit(uint32_t word, uint32_t w) { return (int32_t)(int16_t)(word >> (16 * (w & 1u))); }
    using Acc = ge;
    static __device__ __forceinline__ Acc identity() { return ge_identity(); }
    // Three waves per SIMD with the entries of the next TWO steps in flight (2 x 24 registers, 155 VGPRs, no spills).  Measured (MI355X, 4096 x
    // prove_range staged, ms per batch): four waves and no lead 11.7 -- the 128-register budget leaves no room for an entry in flight and the
    // gather's latency shows on every step --, four waves with one step of lead (64 spilled registers) 11.5, four waves with the lead through
    // LDS by DMA 7.9, three waves with one step of lead 7.4, with two 7.5 (mixed batch: 12.6 / 12.4); the LDS-streamed radix-1024 kernel
    // this replaces: 9.6 (profiles/r04_edg_ab.jsonl)
    static constexpr uint32_t GATHER_WAVES = 3; static constexpr int GATHER_PREFETCH = 2;
    static constexpr uint32_t GATHER_W = EDG_ENTRY_W, GATHER_STRIDE = EDG_SLOT_W, GATHER_PRIO = 0;
    using GAcc = ge;
    static __device__ __forceinline__ GAcc to_gather(const ge& a) { return a; }
    static __device__ __forceinline__ ge from_gather(const GAcc& a) { return a; }
    static __device__ __forceinline__ GAcc accumulate_entry(const GAcc& acc, int32_t d, const uint32_t* e) { return edg_accumulate(acc, d, e); }
    static __device__ __forceinline__ void store(uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows, const Acc& a) { st_ge(p, idx, row, rows, a); }
    static __device__ __forceinline__ Acc load(const uint32_t* p, uint32_t idx, uint32_t row, uint32_t rows) { return ld_ge(p, idx, row, rows); }
    static __device__ __forceinline__ Acc add(const Acc& a, const Acc& b) { return ge_add(a, b); }
};
template __global__ void k_msm_gather<EdGather>(MsmView, uint32_t, uint32_t);
// The same kernel with its waves' issue priority raised (s_setprio; levels 1, 2 and 3 measured alike): for the chain's launches in a batch
// that also holds Groth16 work, whose G1 / G2 gather waves share the SIMDs (batch_impl.inc).
struct EdGatherPrio : EdGather { static constexpr uint32_t GATHER_PRIO = 1; };
template __global__ void k_msm_gather<EdGatherPrio>(MsmView, uint32_t, uint32_t);

uint32_t edg_msm_rows_per_block() { return 256; }
uint32_t edg_msm_blocks_per_cu() {
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k_msm_gather<EdGather>, 256, gather_lds_bytes<EdGather>()) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return occ > 0 ? (uint32_t)occ : 0;
}
void edg_launch_msm(const MsmView& m, uint32_t ngroups, uint32_t nblocks, hipStream_t st, bool raised) {
    const uint32_t grid = ((nblocks + 7) / 8) * 8;
    if (raised) k_msm_gather<EdGatherPrio><<<grid, 256, gather_lds_bytes<EdGather>(), st>>>(m, ngroups, nblocks);
    else k_msm_gather<EdGather><<<grid, 256, gather_lds_bytes<EdGather>(), st>>>(m, ngroups, nblocks);
}

// ---- table construction (edg.h: steps 1-5), one instantiation per radix: the geometry is a compile-time constant inside each kernel, so
// the radix-2^16 kernels are the code they were before the other radices existed (a run-time geometry cost them 2-6 registers)
template <uint32_t WB> __global__ void __launch_bounds__(64) k_edg_bases(const uint32_t* gens, uint32_t* bases) {
    const uint32_t b = blockIdx.x * 64 + threadIdx.x;
    if (b < NBASE) edg_step_bases(edg_geom(WB), gens, bases, b);
}
template <uint32_t WB> __global__ void __launch_bounds__(64) k_edg_starts(const uint32_t* bases, uint32_t* starts) {
    constexpr EdgGeom g = edg_geom(WB);
    const uint32_t bw = blockIdx.x * 64 + threadIdx.x;
    if (bw < NBASE * g.nwin) edg_step_starts(g, bases, starts, bw);
}
template <uint32_t WB> __global__ void __launch_bounds__(256) k_edg_fill(const uint32_t* bases, const uint32_t* starts, uint32_t* table) {
    constexpr EdgGeom g = edg_geom(WB);
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;                 // (bw, run), run fastest
    if (t < NBASE * g.nwin * g.nseg) edg_step_fill(g, bases, starts, table, t / g.nseg, t % g.nseg);
}
template <uint32_t WB> __global__ void __launch_bounds__(256) k_edg_affine(uint32_t* table) {
    constexpr EdgGeom g = edg_geom(WB);
    const size_t grp = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (grp < (size_t)NBASE * g.nwin * g.nent / EDG_INV) edg_step_affine(table, grp);
}
template <uint32_t WB> __global__ void __launch_bounds__(256) k_edg_check(const uint32_t* table, const uint32_t* gens, int* bad) {
    constexpr EdgGeom g = edg_geom(WB);
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (size_t)NBASE * g.nwin * g.nent) return;
    const uint32_t e = (uint32_t)(t % g.nent), bw = (uint32_t)(t / g.nent);
    if (!edg_step_check(g, table, gens, bw / g.nwin, bw % g.nwin, e)) atomicAdd(bad, 1);
}
template <uint32_t WB> void edg_launch_build_at(const uint32_t* d_gens, uint32_t* d_table, uint32_t* d_scratch, int* d_bad, hipStream_t st) {
    constexpr EdgGeom g = edg_geom(WB);
    uint32_t* bases = d_scratch;                                        // [NBASE * nwin][40]
    uint32_t* starts = d_scratch + (size_t)NBASE * g.nwin * GE_W;       // [NBASE * nwin][nseg][40]
    k_edg_bases<WB><<<(NBASE + 63) / 64, 64, 0, st>>>(d_gens, bases);
    k_edg_starts<WB><<<(NBASE * g.nwin + 63) / 64, 64, 0, st>>>(bases, starts);
    k_edg_fill<WB><<<(NBASE * g.nwin * g.nseg + 255) / 256, 256, 0, st>>>(bases, starts, d_table);
    const size_t groups = (size_t)NBASE * g.nwin * g.nent / EDG_INV, slots = (size_t)NBASE * g.nwin * g.nent;
    k_edg_affine<WB><<<(uint32_t)((groups + 255) / 256), 256, 0, st>>>(d_table);
    k_edg_check<WB><<<(uint32_t)((slots + 255) / 256), 256, 0, st>>>(d_table, d_gens, d_bad);
}
size_t edg_build_scratch_words(const EdgGeom& g) { return (size_t)NBASE * g.nwin * (g.nseg + 1) * GE_W; }
void edg_launch_build(const EdgGeom& g, const uint32_t* d_gens, uint32_t* d_table, uint32_t* d_scratch, int* d_bad, hipStream_t st) {
    switch (g.wbits) {
        case 10: edg_launch_build_at<10>(d_gens, d_table, d_scratch, d_bad, st); break;
        case 11: edg_launch_build_at<11>(d_gens, d_table, d_scratch, d_bad, st); break;
        case 12: edg_launch_build_at<12>(d_gens, d_table, d_scratch, d_bad, st); break;
        case 13: edg_launch_build_at<13>(d_gens, d_table, d_scratch, d_bad, st); break;
        case 14: edg_launch_build_at<14>(d_gens, d_table, d_scratch, d_bad, st); break;
        case 15: edg_launch_build_at<15>(d_gens, d_table, d_scratch, d_bad, st); break;
        default: edg_launch_build_at<16>(d_gens, d_table, d_scratch, d_bad, st); break;
    }
}
