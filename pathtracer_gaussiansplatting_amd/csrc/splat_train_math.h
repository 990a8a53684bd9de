// splat_train_math.h — the arithmetic of splat_train.hip as host / device functions (plain f32 in the order
// written, no FMA; the logarithm is detmath's log2x): the inverse activations and RGB2SH of
// ptgs_gaussians_checkpoint_init and one term of ptgs_image_mse. The host build is what the CPU check against the
// numpy float32 restatement compiles. The contract is stated in include/ptgs/ptgs.h.
#pragma once

#include <stdint.h>

#include "detmath.h"
#include "splat_sh_math.h"

namespace ptgs {

constexpr float TRAIN_LN2 = 0.69314718055994531f;

// log(s): the inverse of ptgs_gaussians_activate's exp
PTGS_HD float train_log_scale(float s) { return log2x(s) * TRAIN_LN2; }

// log(o / (1 - o)): the inverse of its sigmoid. o <= 0 and o >= 1 give the huge finite values log2x's -1e30 leads to
PTGS_HD float train_logit(float o) { return (log2x(o) - log2x(1.0f - o)) * TRAIN_LN2; }

// RGB2SH: the DC coefficient whose colour is c
PTGS_HD float train_rgb2sh(float c) { return (c - 0.5f) / SH_C0; }

// Element e of a Gaussian's SH row (`col` = its index within the row of 3 (d + 1)^2 floats): the DC term from the
// Gaussian's colour, +0 for every higher band
PTGS_HD float train_sh_element(const float* color3, uint32_t col) { return col < 3u ? train_rgb2sh(color3[col]) : 0.0f; }

// one term of the squared error: d = a - b in f32, (double)(d * d)
PTGS_HD double train_sq_err(float a, float b) {
  const float d = a - b;
  return (double)(d * d);
}

}  // namespace ptgs
