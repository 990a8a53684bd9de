// splat_backward.h — backward pass of the 3DGS rasterizer (see splat_backward.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ptgs/ptgs.h"
#include "splat.h"

namespace ptgs {

// The published frame a backward pass consumes: what the workspace's latest splat_gaussians call left
// (splat.hip fills it). valid: that call was a complete full-frame ptgs_splat_gaussians (no tile-row
// restriction, no `over` composite) with publish and stats.
struct SplatFrame {
  bool valid;
  uint32_t n, W, H, tiles;
  const uint32_t* sorted_values;  // the tiles' depth-sorted Gaussians
  const uint2* ranges;            // per tile: [begin, end) in sorted_values
  const float4* rec;              // three float4 per Gaussian (gs_preprocess_one, splat_preprocess.h)
  const int* radii;               // 0: culled
};
void splat_last_frame(const SplatWorkspace* w, SplatFrame* out);
// the backward's per-Gaussian accumulator (GS_BWD_ACC floats per Gaussian; grown like the other
// workspace buffers: growth frees the old one, which waits for the device)
#define GS_BWD_ACC 9
#define GS_BWD_ACC_DEPTH 10  // with dL/d(1/d): the backward that also takes dL/d(inverse depth)
hipError_t splat_backward_scratch(SplatWorkspace* w, uint32_t n, uint32_t floats_per_gaussian, float** acc);
// the pose gradient's per-workgroup partial sums: ceil(n / 256) rows of GS_POSE_K floats (dL/d view[r][c] at
// r * 4 + c, r < 3), grown like the accumulator
#define GS_POSE_K 12
hipError_t splat_backward_pose_scratch(SplatWorkspace* w, uint32_t n, float** partials);

// view/mvp column-major float[16]; p00 = proj[0][0], p11 = proj[1][1]; f: the frame (splat_last_frame,
// valid), acc: splat_backward_scratch(n, GS_BWD_ACC), or (n, GS_BWD_ACC_DEPTH) with dL_dinvdepth (W*H floats,
// the gradient with respect to splat_gaussians_invdepth's output; null: the loss depends on the image alone).
// dL_dview (device float[16], column-major; null: not asked for) with proj (the ubo's, host float[16]) and
// pose_partials (splat_backward_pose_scratch(n)): the gradient with respect to the view as well.
// Stream-ordered on s.
hipError_t splat_gaussians_backward(const SplatFrame& f, float* acc, const ptgs_gaussians* g, const float* view,
                                    const float* mvp, float p00, float p11, const float bg[3], const float* dL_dout,
                                    const float* dL_dinvdepth, const ptgs_gaussian_grads* grads, hipStream_t s,
                                    const float* proj = nullptr, float* pose_partials = nullptr,
                                    float* dL_dview = nullptr);
// dL_dview = the sum of `rows` partial rows (0: sixteen zeros; partials is then not read). Stream-ordered on s.
hipError_t splat_pose_finish(const float* partials, uint32_t rows, float* dL_dview, hipStream_t s);
// out[W*H] = the frame's expected inverse depth, sum alpha T / d per pixel (no background term). Reads the
// frame only: it stays valid. Stream-ordered on s; no atomics.
hipError_t splat_gaussians_invdepth(const SplatFrame& f, float* out, hipStream_t s);

}  // namespace ptgs
