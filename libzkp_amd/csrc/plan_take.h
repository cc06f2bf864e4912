// The one take helper of the host plans (batch_plan.h, bpv_plan.h, prover_plan.h): a block is a sequence of regions taken in order from its
// offset 0, each padded to 256 bytes.  No HIP call and no HIP header.
#pragma once
#include <cstddef>

namespace zkp {

struct PlanTake { size_t off = 0; size_t operator()(size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; } };      // the running end of a block

}  // namespace zkp
