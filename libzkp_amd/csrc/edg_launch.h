// Host-callable launchers of the ed25519 gather MSM and of the builder of its HBM-resident tables (defined in edg_kernels.hip, a separate
// translation unit: the Bulletproofs host code in zkp_hip.hip calls these).
#pragma once
#include <hip/hip_runtime.h>
#include "edg.h"

uint32_t edg_msm_rows_per_block();            // lanes (= proofs) per MSM workgroup
uint32_t edg_msm_blocks_per_cu();             // resident workgroups per CU of the built kernel (occupancy query; 0 on failure)
void edg_launch_msm(const zkp::MsmView& m, uint32_t ngroups, uint32_t nblocks, hipStream_t st, bool raised = false);      // raised: the instantiation whose waves raise their issue priority
// builds the whole table of geometry `g` (edg.h) on `st` from the 130 generators (extended coordinates, [NBASE][40] words on the device)
// and checks every slot against its neighbours; scratch: [NBASE * g.nwin][g.nseg + 1][40] words; *bad (device int, zeroed by the caller)
// counts mismatches
void edg_launch_build(const zkp::EdgGeom& g, const uint32_t* d_gens, uint32_t* d_table, uint32_t* d_scratch, int* d_bad, hipStream_t st);
size_t edg_build_scratch_words(const zkp::EdgGeom& g);
// k_sum_t<EdMsm> (8 slices of 32 rows per 256-lane block), defined beside its kernel in zkp_hip.hip
void edg_launch_sum(const zkp::ReduceView& R, uint32_t* sums, hipStream_t st);
