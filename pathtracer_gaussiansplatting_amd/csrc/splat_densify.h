// splat_densify.h — densification and pruning of a 3DGS training run (see splat_densify.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptgs/ptgs.h"

namespace ptgs {

struct DensifyWorkspace;  // the plan's device buffers and the latest plan (one per context)
DensifyWorkspace* densify_workspace_create();
void densify_workspace_destroy(DensifyWorkspace* ws);

// the statistic of one training view (contract in ptgs.h); n > 0
hipError_t densify_accumulate(const float* g2d, const int32_t* radii, uint32_t n, uint32_t W, uint32_t H, float* accum,
                              float* denom, float* max_radii, hipStream_t s);
// decision + scan + source map; waits for s; 0 < n <= 2^30. The plan replaces the workspace's previous one
// (and invalidates it on failure).
hipError_t densify_plan(DensifyWorkspace* ws, const float* scales, const float* opacities, const float* accum,
                        const float* denom, const float* max_radii, uint32_t n, const ptgs_densify_params& p,
                        ptgs_densify_counts* out, hipStream_t s);
void densify_plan_empty(DensifyWorkspace* ws);  // the plan of n == 0: 0 -> 0
// the latest plan's n and total; false when there is none
bool densify_last_plan(const DensifyWorkspace* ws, uint32_t* n, uint32_t* n_out);
// the gather through the latest plan's source map (arguments checked by the caller; n_out > 0).
// hipErrorInvalidValue: more work than one grid holds.
hipError_t densify_apply(const DensifyWorkspace* ws, const float* means, const float* log_scales,
                         const float* rotations, const float* scales, const float* noise, float* means_out,
                         float* log_scales_out, const ptgs_densify_rows* rows, uint32_t n_rows, uint32_t* source_out,
                         hipStream_t s);

}  // namespace ptgs
