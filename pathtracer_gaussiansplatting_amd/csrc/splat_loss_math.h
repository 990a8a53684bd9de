// splat_loss_math.h — the per-pixel arithmetic of splat_loss.hip as host / device functions: the 11-tap Gaussian
// window of the 3DGS training loss (sigma 1.5), its dot product with eleven samples, and the SSIM map of one
// pixel and channel with its three partial derivatives. f32 throughout; the taps are explicit fmaf (this call's
// contract is a tolerance against a float64 reference, not bit-exactness against a restatement). The host build
// is what the CPU check against tests/loss_ref.py compiles. The contract is stated in include/ptgs/ptgs.h.
#pragma once

#include <math.h>
#include <stdint.h>

#include "detmath.h"

namespace ptgs {

constexpr int LOSS_WIN = 11, LOSS_HALO = 5;
constexpr float LOSS_C1 = 0.0001f;  // 0.01^2
constexpr float LOSS_C2 = 0.0009f;  // 0.03^2

// g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)) / sum: float32 of the double-precision values
#define PTGS_LOSS_W0 0.00102838012f
#define PTGS_LOSS_W1 0.00759875821f
#define PTGS_LOSS_W2 0.0360007733f
#define PTGS_LOSS_W3 0.109360687f
#define PTGS_LOSS_W4 0.213005543f
#define PTGS_LOSS_W5 0.266011715f

PTGS_HD float loss_window(int k) {
  const float w[LOSS_WIN] = {PTGS_LOSS_W0, PTGS_LOSS_W1, PTGS_LOSS_W2, PTGS_LOSS_W3, PTGS_LOSS_W4, PTGS_LOSS_W5,
                             PTGS_LOSS_W4, PTGS_LOSS_W3, PTGS_LOSS_W2, PTGS_LOSS_W1, PTGS_LOSS_W0};
  return w[k];
}

// sum over k of g[k] * v[k * stride], accumulated from k = 0 upwards
PTGS_HD float loss_tap11(const float* v, int stride = 1) {
  float acc = PTGS_LOSS_W0 * v[0];
  acc = fmaf(PTGS_LOSS_W1, v[1 * stride], acc);
  acc = fmaf(PTGS_LOSS_W2, v[2 * stride], acc);
  acc = fmaf(PTGS_LOSS_W3, v[3 * stride], acc);
  acc = fmaf(PTGS_LOSS_W4, v[4 * stride], acc);
  acc = fmaf(PTGS_LOSS_W5, v[5 * stride], acc);
  acc = fmaf(PTGS_LOSS_W4, v[6 * stride], acc);
  acc = fmaf(PTGS_LOSS_W3, v[7 * stride], acc);
  acc = fmaf(PTGS_LOSS_W2, v[8 * stride], acc);
  acc = fmaf(PTGS_LOSS_W1, v[9 * stride], acc);
  acc = fmaf(PTGS_LOSS_W0, v[10 * stride], acc);
  return acc;
}

struct LossPixel {
  float m;      // the SSIM map
  float d_mu1;  // dm / d mu1
  float d_s1;   // dm / d sigma1^2
  float d_s12;  // dm / d sigma12
};

// mu1 = conv(a), mu2 = conv(b), e11 = conv(a a), e22 = conv(b b), e12 = conv(a b) of one pixel and channel
PTGS_HD LossPixel loss_ssim_pixel(float mu1, float mu2, float e11, float e22, float e12) {
  const float mu11 = mu1 * mu1, mu22 = mu2 * mu2, mu12 = mu1 * mu2;
  const float s1 = e11 - mu11, s2 = e22 - mu22, s12 = e12 - mu12;
  const float A = 2.0f * mu12 + LOSS_C1;
  const float B = 2.0f * s12 + LOSS_C2;
  const float Cc = (mu11 + mu22) + LOSS_C1;
  const float D = (s1 + s2) + LOSS_C2;
  const float den = Cc * D;
  LossPixel p;
  p.m = (A * B) / den;  // (exactly 1 where a == b over the window)
  p.d_s1 = -p.m / D;
  p.d_s12 = (2.0f * A) / den;
  p.d_mu1 = (((2.0f * mu2) * B) / den - ((2.0f * mu1) * p.m) / Cc) - ((2.0f * mu1) * p.d_s1 + mu2 * p.d_s12);
  return p;
}

PTGS_HD float loss_sign(float d) { return (float)(d > 0.0f) - (float)(d < 0.0f); }

}  // namespace ptgs
