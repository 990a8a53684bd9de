// splat_sh.h — per-frame colours of trained 3DGS checkpoints (see splat_sh.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptgs {

// colors[3 i..] = max(SH(dir_i) + 0.5, 0); sh rows of (sh_degree + 1)^2 * 3 floats, active_degree <= sh_degree <= 3
hipError_t splat_sh_colors(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                           uint32_t active_degree, const float cam[3], float* colors, hipStream_t s);
// scales = expx(log_scales) (3N), opacities = 1 / (1 + expx(-logits)) (N)
hipError_t splat_sh_activate(const float* log_scales, const float* logits, uint32_t count, float* scales,
                             float* opacities, hipStream_t s);
// the backward of splat_sh_colors: dsh (count rows, every element written) = dL/d(sh); dmeans: NULL, or
// dL/d(mean) is added to it (skipped at sh_degree == 0 or active_degree == 0)
hipError_t splat_sh_colors_backward(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                                    uint32_t active_degree, const float cam[3], const float* dcolors, float* dsh,
                                    float* dmeans, hipStream_t s);
// splat_sh_colors_backward plus deye (device float[3]) = dL/d(cam) = -(the sum of what it adds to dL/d(mean)),
// formed with dmeans NULL too; exact zeros at count == 0, sh_degree == 0 or active_degree == 0. eye_partials:
// 3 * splat_sh_eye_rows(count) device floats of scratch, one row per workgroup, all written by the call; a
// second launch adds them in float64 in a fixed order (no atomics).
inline uint32_t splat_sh_eye_rows(uint32_t count) { return (uint32_t)(((uint64_t)count + 255u) / 256u); }
hipError_t splat_sh_colors_backward_eye(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                                        uint32_t active_degree, const float cam[3], const float* dcolors, float* dsh,
                                        float* dmeans, float* eye_partials, float* deye, hipStream_t s);
// the backward of splat_sh_activate from the activated values: dlog_scales = dscales * scales (3N),
// dlogits = (dopacities * o) * (1 - o) (N); an output may alias its upstream gradient
hipError_t splat_sh_activate_backward(const float* scales, const float* opacities, uint32_t count,
                                      const float* dscales, const float* dopacities, float* dlog_scales,
                                      float* dlogits, hipStream_t s);
// out row i = sh row ids[i] (a row of zeros for ids[i] >= count)
hipError_t splat_sh_permute(const float* sh, uint32_t sh_degree, const uint32_t* ids, uint32_t count, float* out,
                            hipStream_t s);

}  // namespace ptgs
