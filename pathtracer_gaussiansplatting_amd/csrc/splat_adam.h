// splat_adam.h — the optimizer step of a 3DGS training run and the opacity reset (see splat_adam.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptgs/ptgs.h"

namespace ptgs {

// One Adam step over every row of the table in one launch (contract in ptgs.h; arguments checked by the caller:
// n > 0, 0 < n_rows <= PTGS_ADAM_MAX_ROWS). radii == nullptr: dense. hipErrorInvalidValue: more work than one
// grid holds.
hipError_t adam_step(uint32_t n, const ptgs_adam_rows* rows, uint32_t n_rows, const ptgs_adam_params& params,
                     const int32_t* radii, hipStream_t s);
// logit' = min(logit, cap) and zeros to the moments that are given; n > 0
hipError_t opacity_reset(float* logits, uint32_t n, float cap, float* exp_avg, float* exp_avg_sq, hipStream_t s);

}  // namespace ptgs
