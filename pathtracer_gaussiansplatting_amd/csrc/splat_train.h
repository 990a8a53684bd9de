// splat_train.h — the two device calls a 3DGS training loop needs besides its stages: a checkpoint's leaves
// from initialised Gaussians, and the evaluation metric (see splat_train.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptgs {

// log_scales = log(scales) (3N), logits = logit(opacities) (N), sh rows of 3 (sh_degree + 1)^2 floats = (RGB2SH of
// the colour, zeros); one launch; log_scales / logits may be scales / opacities themselves. Arguments checked by
// the caller: n > 0, sh_degree <= 3.
hipError_t train_checkpoint_init(const float* scales, const float* opacities, const float* colors, uint32_t n,
                                 uint32_t sh_degree, float* log_scales, float* logits, float* sh, hipStream_t s);

// the doubles of scratch image_mse needs, whatever the image's size
constexpr uint32_t TRAIN_MSE_MAX_WG = 1024;

// out_sum[0] = sum over the pixels' rgb of (double)((a - b)^2), a = image [H, W, 4], b = target [H, W, channels];
// partials: TRAIN_MSE_MAX_WG device doubles. Two launches, a fixed order, no atomics. pixels > 0.
hipError_t train_image_mse(const float* image, const float* target, uint32_t channels, uint64_t pixels,
                           double* partials, double* out_sum, hipStream_t s);

}  // namespace ptgs
