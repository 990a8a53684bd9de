// splat_backward_math.h — the per-Gaussian projection backward of splat_backward.hip as a host / device
// function (plain f32; the host build is what a CPU check against the float64 reference compiles).
#pragma once

#include <stdint.h>

#include "detmath.h"

namespace ptgs {

struct GbCam {
  float view[16];
  float mvp[16];
  float fx, fy, limx, limy;  // P00*W/2, P11*H/2 (fy negative: Vulkan y-down); 1.3 tan_fov: the EWA clamp
  uint32_t W, H, grid_x;
};

// One visible Gaussian: (dL/d means2d (dgx, dgy), dL/d conic (da, db, dc)) -> dL/d mean (dm), the linear
// scales (dsc) and the un-normalised quaternion (dq), through conic = cov^-1, cov = T Sigma T^T + 0.3 I,
// T = J W with J at the clamped point, Sigma = R S^2 R^T and q / |q| (gs_preprocess_one's forward, recomputed).
// DEPTH: dinvd = dL/d(1/d) as well, the inverse depth's share (D = sum wgt / d): it reaches the mean through
// d = -(V row 2) . (mean, 1) alone, dL/dd = -dinvd / d^2. Order and membership carry no gradient.
template <bool DEPTH = false>
PTGS_HD void gs_project_backward_one(const GbCam& cam, const float* mean, const float* scale, const float* rot,
                                     float dgx, float dgy, float da, float db, float dc, float* dm, float* dsc,
                                     float* dq, float dinvd = 0.0f) {
  // ---- the forward again (gs_preprocess_one) ----
  const float* V = cam.view;  // column-major: row r, col c = V[c*4 + r]
  const float* P = cam.mvp;
  const float mx = mean[0], my = mean[1], mz = mean[2];
  const float sx = scale[0], sy = scale[1], sz = scale[2];
  const float q0 = rot[0], q1 = rot[1], q2 = rot[2], q3 = rot[3];
  const float pvx = ((V[0] * mx + V[4] * my) + V[8] * mz) + V[12];
  const float pvy = ((V[1] * mx + V[5] * my) + V[9] * mz) + V[13];
  const float d = -(((V[2] * mx + V[6] * my) + V[10] * mz) + V[14]);
  const float phx = ((P[0] * mx + P[4] * my) + P[8] * mz) + P[12];
  const float phy = ((P[1] * mx + P[5] * my) + P[9] * mz) + P[13];
  const float phw = ((P[3] * mx + P[7] * my) + P[11] * mz) + P[15];
  const float pw = 1.0f / (phw + 0.0000001f);
  const float qn = sqrtx(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
  const float qr = q0 / qn, qx = q1 / qn, qy = q2 / qn, qz = q3 / qn;
  const float R[3][3] = {{1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qr * qz), 2.0f * (qx * qz + qr * qy)},
                         {2.0f * (qx * qy + qr * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qr * qx)},
                         {2.0f * (qx * qz - qr * qy), 2.0f * (qy * qz + qr * qx), 1.0f - 2.0f * (qx * qx + qy * qy)}};
  const float sc[3] = {sx, sy, sz};
  float M[3][3], S[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) M[r][k] = R[r][k] * sc[k];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) S[r][k] = (M[r][0] * M[k][0] + M[r][1] * M[k][1]) + M[r][2] * M[k][2];
  const float txtz = pvx / d, tytz = pvy / d;
  const bool clx = txtz < -cam.limx || txtz > cam.limx, cly = tytz < -cam.limy || tytz > cam.limy;
  const float tx = fminx(cam.limx, fmaxx(-cam.limx, txtz)) * d;
  const float ty = fminx(cam.limy, fmaxx(-cam.limy, tytz)) * d;
  const float d2 = d * d;
  const float J00 = cam.fx / d, J02 = (cam.fx * tx) / d2, J11 = cam.fy / d, J12 = (cam.fy * ty) / d2;
  const float Wm[3][3] = {{V[0], V[4], V[8]}, {V[1], V[5], V[9]}, {V[2], V[6], V[10]}};  // view rotation rows
  float T[2][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    T[0][k] = J00 * Wm[0][k] + J02 * Wm[2][k];
    T[1][k] = J11 * Wm[1][k] + J12 * Wm[2][k];
  }
  float U[2][3];  // T Sigma
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) U[r][k] = (T[r][0] * S[0][k] + T[r][1] * S[1][k]) + T[r][2] * S[2][k];
  const float ca = ((U[0][0] * T[0][0] + U[0][1] * T[0][1]) + U[0][2] * T[0][2]) + 0.3f;
  const float cb = (U[0][0] * T[1][0] + U[0][1] * T[1][1]) + U[0][2] * T[1][2];
  const float cc = ((U[1][0] * T[1][0] + U[1][1] * T[1][1]) + U[1][2] * T[1][2]) + 0.3f;
  const float det_inv = 1.0f / (ca * cc - cb * cb);
  const float a = cc * det_inv, b = -cb * det_inv, c = ca * det_inv;  // the conic Q = cov^-1
  // ---- conic -> cov: dL = tr(Mc dcov) with Mc = -Q G Q, G = [[da, db/2], [db/2, dc]] ----
  const float hb = 0.5f * db;
  const float g00 = a * da + b * hb, g01 = a * hb + b * dc, g10 = b * da + c * hb, g11 = b * hb + c * dc;
  const float m00 = -(g00 * a + g01 * b), m01 = -(g00 * b + g01 * c), m11 = -(g10 * b + g11 * c);
  // ---- cov = T Sigma T^T: dL/dSigma = T^T Mc T, dL/dT = 2 Mc T Sigma ----
  float MT[2][3], N[3][3], dT[2][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    MT[0][k] = m00 * T[0][k] + m01 * T[1][k];
    MT[1][k] = m01 * T[0][k] + m11 * T[1][k];
  }
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) N[r][k] = T[0][r] * MT[0][k] + T[1][r] * MT[1][k];
#pragma unroll
  for (int r = 0; r < 2; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) dT[r][k] = 2.0f * ((MT[r][0] * S[0][k] + MT[r][1] * S[1][k]) + MT[r][2] * S[2][k]);
  // ---- Sigma = M M^T, M = R S: dL/dM = 2 N M; scales and R ----
  float dR[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) dsc[k] = 0.0f;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float dM = 2.0f * ((N[r][0] * M[0][k] + N[r][1] * M[1][k]) + N[r][2] * M[2][k]);
      dsc[k] += dM * R[r][k];
      dR[r][k] = dM * sc[k];
    }
  // ---- R(q / |q|) ----
  const float hr = 2.0f * (((-qz * dR[0][1] + qy * dR[0][2]) + (qz * dR[1][0] - qx * dR[1][2])) +
                           (-qy * dR[2][0] + qx * dR[2][1]));
  const float hx = 2.0f * ((((qy * dR[0][1] + qz * dR[0][2]) + (qy * dR[1][0] - 2.0f * qx * dR[1][1])) +
                            ((-qr * dR[1][2] + qz * dR[2][0]) + (qr * dR[2][1] - 2.0f * qx * dR[2][2]))));
  const float hy = 2.0f * ((((-2.0f * qy * dR[0][0] + qx * dR[0][1]) + (qr * dR[0][2] + qx * dR[1][0])) +
                            ((qz * dR[1][2] - qr * dR[2][0]) + (qz * dR[2][1] - 2.0f * qy * dR[2][2]))));
  const float hz = 2.0f * ((((-2.0f * qz * dR[0][0] - qr * dR[0][1]) + (qx * dR[0][2] + qr * dR[1][0])) +
                            ((-2.0f * qz * dR[1][1] + qy * dR[1][2]) + (qx * dR[2][0] + qy * dR[2][1]))));
  const float hq = ((qr * hr + qx * hx) + qy * hy) + qz * hz;
  dq[0] = (hr - qr * hq) / qn;
  dq[1] = (hx - qx * hq) / qn;
  dq[2] = (hy - qy * hq) / qn;
  dq[3] = (hz - qz * hq) / qn;
  // ---- T = J W, J at the clamped point: a clamped tx depends on the mean through d only ----
  const float dJ00 = (dT[0][0] * Wm[0][0] + dT[0][1] * Wm[0][1]) + dT[0][2] * Wm[0][2];
  const float dJ02 = (dT[0][0] * Wm[2][0] + dT[0][1] * Wm[2][1]) + dT[0][2] * Wm[2][2];
  const float dJ11 = (dT[1][0] * Wm[1][0] + dT[1][1] * Wm[1][1]) + dT[1][2] * Wm[1][2];
  const float dJ12 = (dT[1][0] * Wm[2][0] + dT[1][1] * Wm[2][1]) + dT[1][2] * Wm[2][2];
  const float d3 = d2 * d;
  float dpx = clx ? 0.0f : dJ02 * cam.fx / d2;
  float dpy = cly ? 0.0f : dJ12 * cam.fy / d2;
  float dd = -(dJ00 * cam.fx + dJ11 * cam.fy) / d2;
  dd -= (clx ? 1.0f : 2.0f) * dJ02 * cam.fx * tx / d3;
  dd -= (cly ? 1.0f : 2.0f) * dJ12 * cam.fy * ty / d3;
  if (DEPTH) dd -= dinvd / d2;  // ---- 1 / d of the inverse depth ----
  // ---- means2d = ndc2pix(ph.xy / (ph.w + 1e-7)) ----
  const float dnx = dgx * 0.5f * (float)cam.W, dny = dgy * 0.5f * (float)cam.H;
  const float dphx = dnx * pw, dphy = dny * pw, dphw = -(dnx * phx + dny * phy) * pw * pw;
#pragma unroll
  for (int k = 0; k < 3; ++k)
    dm[k] = ((dpx * Wm[0][k] + dpy * Wm[1][k]) - dd * Wm[2][k]) +
            ((dphx * P[4 * k] + dphy * P[4 * k + 1]) + dphw * P[4 * k + 3]);
}

}  // namespace ptgs
