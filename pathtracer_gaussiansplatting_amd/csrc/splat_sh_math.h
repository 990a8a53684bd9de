// splat_sh_math.h — the per-Gaussian spherical-harmonic colour of splat_sh.hip and its backward as host /
// device functions (plain f32, no FMA; the host build is what a CPU check against the float64 reference
// compiles). The forward's contract is stated in splat_sh.hip and include/ptgs/ptgs.h.
#pragma once

#include <stdint.h>

#include "detmath.h"

namespace ptgs {

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
constexpr float SH_C2_0 = 1.0925484305920792f, SH_C2_1 = -1.0925484305920792f, SH_C2_2 = 0.31539156525252005f,
                SH_C2_3 = -1.0925484305920792f, SH_C2_4 = 0.5462742152960396f;
constexpr float SH_C3_0 = -0.5900435899266435f, SH_C3_1 = 2.890611442640554f, SH_C3_2 = -0.4570457994644658f,
                SH_C3_3 = 0.3731763325901154f, SH_C3_4 = -0.4570457994644658f, SH_C3_5 = 1.445305721320277f,
                SH_C3_6 = -0.5900435899266435f;

constexpr int sh_row(int deg) { return 3 * (deg + 1) * (deg + 1); }

// (x, y, z) = len > 0 ? d / len : 0 with d = mean - cam; *len_out = len
PTGS_HD v3 sh_dir(const float* mean, v3 cam, float* len_out) {
  const v3 d = mk3(mean[0], mean[1], mean[2]) - cam;
  const float len = length3(d);
  *len_out = len;
  return len > 0.0f ? d / len : mk3(0.0f);
}

// row: the Gaussian's coefficients [k][c]; active <= DEG bands are evaluated. out[c] = res + 0.5, the value
// the clamp tests (color = out < 0 ? 0 : out)
template <int DEG>
PTGS_HD void sh_res(const float* row, uint32_t active, v3 dir, float* out) {
  float res[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) res[c] = SH_C0 * row[c];
  if (DEG >= 1 && active >= 1) {
    const float x = dir.x, y = dir.y, z = dir.z;
    const float w1 = SH_C1 * y, w2 = SH_C1 * z, w3 = SH_C1 * x;
#pragma unroll
    for (int c = 0; c < 3; ++c) res[c] = res[c] - w1 * row[3 + c] + w2 * row[6 + c] - w3 * row[9 + c];
    if (DEG >= 2 && active >= 2) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      const float w4 = SH_C2_0 * xy, w5 = SH_C2_1 * yz, w6 = SH_C2_2 * (2.0f * zz - xx - yy);
      const float w7 = SH_C2_3 * xz, w8 = SH_C2_4 * (xx - yy);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        res[c] = res[c] + w4 * row[12 + c] + w5 * row[15 + c] + w6 * row[18 + c] + w7 * row[21 + c] +
                 w8 * row[24 + c];
      if (DEG >= 3 && active >= 3) {
        const float w9 = SH_C3_0 * y * (3.0f * xx - yy), w10 = SH_C3_1 * xy * z;
        const float w11 = SH_C3_2 * y * (4.0f * zz - xx - yy);
        const float w12 = SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        const float w13 = SH_C3_4 * x * (4.0f * zz - xx - yy), w14 = SH_C3_5 * z * (xx - yy);
        const float w15 = SH_C3_6 * x * (3.0f * xx - yy);
#pragma unroll
        for (int c = 0; c < 3; ++c)
          res[c] = res[c] + w9 * row[27 + c] + w10 * row[30 + c] + w11 * row[33 + c] + w12 * row[36 + c] +
                   w13 * row[39 + c] + w14 * row[42 + c] + w15 * row[45 + c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = res[c] + 0.5f;
}

template <int DEG>
PTGS_HD void sh_eval(const float* row, uint32_t active, v3 dir, float* out) {
  float r[3];
  sh_res<DEG>(row, active, dir, r);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[c] = fmaxx(r[c], 0.0f);
}

// f[k], k < (DEG + 1)^2: the factor sh_res forms in front of sh[k] (C0, -(C1*y), C1*z, -(C1*x), C2[0]*xy, ...:
// the same expressions; the negation is exact), 0 for the bands above `active`
template <int DEG>
PTGS_HD void sh_factors(uint32_t active, v3 dir, float* f) {
  f[0] = SH_C0;
  if constexpr (DEG >= 1) {
    const float x = dir.x, y = dir.y, z = dir.z;
    const bool on = active >= 1;
    f[1] = on ? -(SH_C1 * y) : 0.0f;
    f[2] = on ? SH_C1 * z : 0.0f;
    f[3] = on ? -(SH_C1 * x) : 0.0f;
    if constexpr (DEG >= 2) {
      const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
      const bool on2 = active >= 2;
      f[4] = on2 ? SH_C2_0 * xy : 0.0f;
      f[5] = on2 ? SH_C2_1 * yz : 0.0f;
      f[6] = on2 ? SH_C2_2 * (2.0f * zz - xx - yy) : 0.0f;
      f[7] = on2 ? SH_C2_3 * xz : 0.0f;
      f[8] = on2 ? SH_C2_4 * (xx - yy) : 0.0f;
      if constexpr (DEG >= 3) {
        const bool on3 = active >= 3;
        f[9] = on3 ? SH_C3_0 * y * (3.0f * xx - yy) : 0.0f;
        f[10] = on3 ? SH_C3_1 * xy * z : 0.0f;
        f[11] = on3 ? SH_C3_2 * y * (4.0f * zz - xx - yy) : 0.0f;
        f[12] = on3 ? SH_C3_3 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) : 0.0f;
        f[13] = on3 ? SH_C3_4 * x * (4.0f * zz - xx - yy) : 0.0f;
        f[14] = on3 ? SH_C3_5 * z * (xx - yy) : 0.0f;
        f[15] = on3 ? SH_C3_6 * x * (3.0f * xx - yy) : 0.0f;
      }
    }
  }
}

// v = dL/d(dir) = sum_k grad(f_k)(x, y, z) t[k], t[k] = sum_c dres[c] sh[k][c]: the polynomial derivatives of the
// factors above with respect to x, y, z taken as independent variables
template <int DEG>
PTGS_HD v3 sh_dir_grad(const float* row, uint32_t active, v3 dir, const float* dres) {
  if constexpr (DEG < 1) {
    return mk3(0.0f);
  } else {
    if (active < 1) return mk3(0.0f);
    float t[(DEG + 1) * (DEG + 1)];
#pragma unroll
    for (int k = 1; k < (DEG + 1) * (DEG + 1); ++k)
      t[k] = (dres[0] * row[3 * k] + dres[1] * row[3 * k + 1]) + dres[2] * row[3 * k + 2];
    const float x = dir.x, y = dir.y, z = dir.z;
    float vx = -(SH_C1 * t[3]), vy = -(SH_C1 * t[1]), vz = SH_C1 * t[2];
    if constexpr (DEG >= 2) if (active >= 2) {
      vx = vx + (SH_C2_0 * y) * t[4] - (SH_C2_2 * 2.0f * x) * t[6] + (SH_C2_3 * z) * t[7] + (SH_C2_4 * 2.0f * x) * t[8];
      vy = vy + (SH_C2_0 * x) * t[4] + (SH_C2_1 * z) * t[5] - (SH_C2_2 * 2.0f * y) * t[6] - (SH_C2_4 * 2.0f * y) * t[8];
      vz = vz + (SH_C2_1 * y) * t[5] + (SH_C2_2 * 4.0f * z) * t[6] + (SH_C2_3 * x) * t[7];
      if constexpr (DEG >= 3) if (active >= 3) {
        const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
        vx = vx + (SH_C3_0 * 6.0f * xy) * t[9] + (SH_C3_1 * yz) * t[10] - (SH_C3_2 * 2.0f * xy) * t[11] -
             (SH_C3_3 * 6.0f * xz) * t[12] + (SH_C3_4 * (4.0f * zz - 3.0f * xx - yy)) * t[13] +
             (SH_C3_5 * 2.0f * xz) * t[14] + (SH_C3_6 * (9.0f * xx - yy)) * t[15];
        vy = vy + (SH_C3_0 * 3.0f * (xx - yy)) * t[9] + (SH_C3_1 * xz) * t[10] +
             (SH_C3_2 * (4.0f * zz - xx - 3.0f * yy)) * t[11] - (SH_C3_3 * 6.0f * yz) * t[12] -
             (SH_C3_4 * 2.0f * xy) * t[13] - (SH_C3_5 * 2.0f * yz) * t[14] - (SH_C3_6 * 2.0f * xy) * t[15];
        vz = vz + (SH_C3_1 * xy) * t[10] + (SH_C3_2 * 8.0f * yz) * t[11] +
             (SH_C3_3 * 3.0f * (2.0f * zz - xx - yy)) * t[12] + (SH_C3_4 * 8.0f * xz) * t[13] +
             (SH_C3_5 * (xx - yy)) * t[14];
      }
    }
    return mk3(vx, vy, vz);
  }
}

// One Gaussian of ptgs_gaussians_sh_colors_backward. row: its coefficients; dcol: dL/d(color) (3); drow: its
// row of dL/d(sh), every element written, and MAY BE row itself (row is read completely before drow is
// written); dmean: NULL, or 3 floats that dL/d(mean) is ADDED to. dir, len: sh_dir of the Gaussian.
//   dres[c] = (res + 0.5 < 0) ? 0 : dcol[c]      (the forward's own test, recomputed with its arithmetic)
//   drow[k][c] = f_k * dres[c]                   (one multiply; bands above `active`: 0)
//   dmean += (v - dir (dir . v)) / len           (v: sh_dir_grad; nothing is added at len == 0)
// dm_out: NULL, or 3 floats that receive that same (v - dir (dir . v)) / len, zeros where nothing is added: the
// Gaussian's share of -dL/d(camera_pos) (the colour sees mean - camera_pos alone); it is formed with dmean NULL too.
template <int DEG>
PTGS_HD void sh_backward_one(const float* row, uint32_t active, v3 dir, float len, const float* dcol, float* drow,
                             float* dmean, float* dm_out = nullptr) {
  float r[3], dres[3];
  sh_res<DEG>(row, active, dir, r);
#pragma unroll
  for (int c = 0; c < 3; ++c) dres[c] = r[c] < 0.0f ? 0.0f : dcol[c];
  if (dm_out) dm_out[0] = dm_out[1] = dm_out[2] = 0.0f;
  if (DEG >= 1 && (dmean || dm_out) && active >= 1 && len > 0.0f) {
    const v3 v = sh_dir_grad<DEG>(row, active, dir, dres);
    const float dv = dot3(dir, v);
    const v3 dm = (v - dir * dv) / len;
    if (dmean) {
      dmean[0] = dmean[0] + dm.x;
      dmean[1] = dmean[1] + dm.y;
      dmean[2] = dmean[2] + dm.z;
    }
    if (dm_out) {
      dm_out[0] = dm.x;
      dm_out[1] = dm.y;
      dm_out[2] = dm.z;
    }
  }
  float f[(DEG + 1) * (DEG + 1)];
  sh_factors<DEG>(active, dir, f);
#pragma unroll
  for (int k = 0; k < (DEG + 1) * (DEG + 1); ++k)
#pragma unroll
    for (int c = 0; c < 3; ++c) drow[3 * k + c] = f[k] * dres[c];
}

// run-time degree (host builds and tests); false: sh_degree above 3
PTGS_HD bool sh_backward_one_deg(uint32_t sh_degree, const float* row, uint32_t active, v3 dir, float len,
                                 const float* dcol, float* drow, float* dmean) {
  switch (sh_degree) {
    case 0: sh_backward_one<0>(row, active, dir, len, dcol, drow, dmean); return true;
    case 1: sh_backward_one<1>(row, active, dir, len, dcol, drow, dmean); return true;
    case 2: sh_backward_one<2>(row, active, dir, len, dcol, drow, dmean); return true;
    case 3: sh_backward_one<3>(row, active, dir, len, dcol, drow, dmean); return true;
  }
  return false;
}

// the activations' backward, from the ACTIVATED values: d exp = exp, d sigmoid = o (1 - o)
PTGS_HD float sh_dlog_scale(float dL_dscale, float scale) { return dL_dscale * scale; }
PTGS_HD float sh_dlogit(float dL_dopacity, float o) { return (dL_dopacity * o) * (1.0f - o); }

}  // namespace ptgs
