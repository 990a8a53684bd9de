// splat_densify_math.h — the per-Gaussian arithmetic of splat_densify.hip as host / device functions (plain
// f32 add / sub / mul / div / sqrt in the order written, no FMA, no transcendental): the densification
// statistic, the decision of densify_and_prune and the mean of a split child. The host build is what the CPU
// check against the sequential numpy reference compiles. The contract is stated in include/ptgs/ptgs.h.
#pragma once

#include <stdint.h>

#include "../../include/ptgs/ptgs.h"
#include "detmath.h"

namespace ptgs {

// what becomes of source Gaussian i (bits of one byte; the plan scans the first three)
constexpr uint32_t DN_KEEP = 1u;             // the original survives
constexpr uint32_t DN_CLONE = 2u;            // its clone exists
constexpr uint32_t DN_CHILDREN = 4u;         // its two children exist
constexpr uint32_t DN_PRUNED = 8u;           // an original (not split) that the prune test removed
constexpr uint32_t DN_PRUNED_CHILDREN = 16u; // a split source whose two children the prune test removed
constexpr int DN_FATES = 5;

// entries of the source map: the source index in the low 30 bits, the kind above
constexpr uint32_t DN_KIND_SHIFT = 30u;
constexpr uint32_t DN_INDEX_MASK = (1u << DN_KIND_SHIFT) - 1u;
constexpr uint32_t DN_KIND_ORIGINAL = 0u, DN_KIND_CLONE = 1u, DN_KIND_CHILD0 = 2u, DN_KIND_CHILD1 = 3u;
constexpr uint32_t DN_MAX_N = 1u << DN_KIND_SHIFT;

constexpr float DN_SPLIT_DIV = 1.6f;         // the trainer's 0.8 * 2
constexpr float DN_LOG_SPLIT = 0.4700036f;   // ln 1.6 rounded to f32

// One training view's contribution of a visible Gaussian (radius > 0; the caller tests that): the pixel gradient
// in the NDC convention of the trainer's threshold, its norm added, the view counted, the radius kept.
PTGS_HD void dn_accumulate_one(float g2dx, float g2dy, int32_t radius, uint32_t W, uint32_t H, float* accum,
                               float* denom, float* max_radius) {
  const float gx = g2dx * (0.5f * (float)W);
  const float gy = g2dy * (0.5f * (float)H);
  *accum = *accum + sqrtx(gx * gx + gy * gy);
  *denom = *denom + 1.0f;
  *max_radius = fmaxx(*max_radius, (float)radius);
}

// the prune test of opacity o, largest scale m and screen radius r
PTGS_HD bool dn_pruned(const ptgs_densify_params& p, float o, float m, float r) {
  return o < p.min_opacity || (p.max_screen_radius > 0.0f && r > p.max_screen_radius) ||
         (p.max_scale > 0.0f && m > p.max_scale);
}

// DN_* bits of one source Gaussian (s: its three activated scales)
PTGS_HD uint32_t dn_decide(const ptgs_densify_params& p, const float* s, float o, float accum, float denom,
                           float max_radius) {
  const float avg = denom > 0.0f ? accum / denom : 0.0f;
  const float smax = fmaxx(fmaxx(s[0], s[1]), s[2]);
  const bool hot = avg >= p.grad_threshold;
  const bool clone = hot && smax <= p.scale_split;
  const bool split = hot && smax > p.scale_split;
  if (split) return dn_pruned(p, o, smax / DN_SPLIT_DIV, max_radius) ? DN_PRUNED_CHILDREN : DN_CHILDREN;
  if (dn_pruned(p, o, smax, max_radius)) return DN_PRUNED;
  return DN_KEEP | (clone ? DN_CLONE : 0u);
}

// Row r of the rotation of the quaternion q = (w, x, y, z) / n, n = sqrt(((w*w + x*x) + y*y) + z*z), the entries
// in the forward projection's order (gs_preprocess_one); n == 0: the identity.
PTGS_HD void dn_rotation(const float* q, float R[3][3]) {
  const float n = sqrtx(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  if (!(n != 0.0f)) {
    for (int r = 0; r < 3; ++r)
      for (int k = 0; k < 3; ++k) R[r][k] = r == k ? 1.0f : 0.0f;
    return;
  }
  const float qr = q[0] / n, qx = q[1] / n, qy = q[2] / n, qz = q[3] / n;
  R[0][0] = 1.0f - 2.0f * (qy * qy + qz * qz);
  R[0][1] = 2.0f * (qx * qy - qr * qz);
  R[0][2] = 2.0f * (qx * qz + qr * qy);
  R[1][0] = 2.0f * (qx * qy + qr * qz);
  R[1][1] = 1.0f - 2.0f * (qx * qx + qz * qz);
  R[1][2] = 2.0f * (qy * qz - qr * qx);
  R[2][0] = 2.0f * (qx * qz - qr * qy);
  R[2][1] = 2.0f * (qy * qz + qr * qx);
  R[2][2] = 1.0f - 2.0f * (qx * qx + qy * qy);
}

// mean' = mean + R v, v = scales * z (z: the child's standard-normal draw), each row (R_r0*v0 + R_r1*v1) + R_r2*v2
PTGS_HD void dn_child_mean(const float* mean, const float* q, const float* s, const float* z, float* out) {
  float R[3][3];
  dn_rotation(q, R);
  const float v0 = s[0] * z[0], v1 = s[1] * z[1], v2 = s[2] * z[2];
  for (int r = 0; r < 3; ++r) out[r] = mean[r] + ((R[r][0] * v0 + R[r][1] * v1) + R[r][2] * v2);
}

// one component of the same (what a work-item that owns one output float evaluates)
PTGS_HD float dn_child_mean_component(const float* mean, const float* q, const float* s, const float* z, int r) {
  float out[3];
  dn_child_mean(mean, q, s, z, out);
  return r == 0 ? out[0] : (r == 1 ? out[1] : out[2]);
}

}  // namespace ptgs
