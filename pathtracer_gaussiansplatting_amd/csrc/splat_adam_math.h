// splat_adam_math.h — the arithmetic of splat_adam.hip as host / device functions (plain f32 add / sub / mul /
// div / sqrt in the order written, no FMA, no transcendental on the device): the scalars the host derives once
// per call, the update of one element and the opacity reset of one logit. The host build is what the CPU check
// against the numpy float32 reference compiles. The contract is stated in include/ptgs/ptgs.h.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/ptgs/ptgs.h"
#include "detmath.h"

namespace ptgs {

// what every element of a call shares
struct AdamScalars {
  float beta1, beta2, ob1, ob2, bc2s, eps;
};

// the scalars of one call and bc1, the divisor of every row's rate (host: the two powers are evaluated in double)
inline AdamScalars adam_scalars(const ptgs_adam_params& p, float* bc1) {
  AdamScalars s;
  s.beta1 = p.beta1;
  s.beta2 = p.beta2;
  s.ob1 = 1.0f - p.beta1;
  s.ob2 = 1.0f - p.beta2;
  *bc1 = (float)(1.0 - pow((double)p.beta1, (double)p.step));
  s.bc2s = (float)sqrt(1.0 - pow((double)p.beta2, (double)p.step));
  s.eps = p.eps;
  return s;
}

// a row's step size: ss = lr / bc1
inline float adam_step_size(float lr, float bc1) { return lr / bc1; }

// one element: gradient g, step size ss (the row's ss or ss_head); *p, *m, *v updated in place
PTGS_HD void adam_update(const AdamScalars& s, float ss, float g, float* p, float* m, float* v) {
  const float m1 = (s.beta1 * *m) + (s.ob1 * g);
  const float v1 = (s.beta2 * *v) + ((s.ob2 * g) * g);
  const float d = (sqrtx(v1) / s.bc2s) + s.eps;
  *p = *p - (ss * (m1 / d));
  *m = m1;
  *v = v1;
}

// the logit of max_opacity (host, in double)
inline float adam_reset_cap(float max_opacity) {
  return (float)log((double)max_opacity / (1.0 - (double)max_opacity));
}

// a NaN stays a NaN
PTGS_HD float adam_reset_logit(float logit, float cap) { return logit > cap ? cap : logit; }

}  // namespace ptgs
