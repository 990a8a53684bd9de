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
// T = J W with J at the clamped point, Sigma = R S^2 R^T and q / |q| (gs_preprocess_one's function).
//
// The covariance is handled as cov = A A^T + 0.3 I, A = T R S (2x3), one column A_k = sc[k] T R[:, k] at a time,
// and neither Sigma nor Mc = dL/dcov = -Q G Q is formed. With Mc built from the rounded conic Q and carried
// through T^T Mc T Sigma, the gradient of a needle's long axis (axis ratio 200 and more) was what is left when
// terms (l1 / l2) times larger cancel, l1, l2 the eigenvalues of cov: 6e-3 relative in a single dL/dsc, 1.8e-4
// relative L2 over a case, 10x float32 autograd's error, and no single stage in double repaired it. Here
//   Q A_k = adj(cov) A_k / det = adj(cov - A_k A_k^T) A_k / det,  since adj is linear on 2x2 matrices and
//   adj(A_k A_k^T) A_k = 0 exactly: the long axis meets only the other two columns and the dilation;
//   det(A A^T + 0.3 I) = |row 0 x row 1|^2 + 0.3 tr(A A^T) + 0.09 (Cauchy-Binet): a sum of positive terms;
//   dL/dA_k = -2 Q G (Q A_k), dL/dsc[k] = -2 sc[k] (Q t_k)^T G (Q t_k) with t_k = T R[:, k].
// The same case then lands at 7e-6, under float32 autograd's error.
// DEPTH: dinvd = dL/d(1/d) as well, the inverse depth's share (D = sum wgt / d): it reaches the mean through
// d = -(V row 2) . (mean, 1) alone, dL/dd = -dinvd / d^2. Order and membership carry no gradient.
// POSE: dview[r * 4 + c], r < 3, c < 4 = this Gaussian's share of dL/d view[r][c] as well (twelve floats, every
// one written), the same function read as a function of the view: (x, y, -d) = view (mean, 1), W = the view's
// upper-left 3x3 in T = J W, ph = (proj view)(mean, 1) with proj (column-major float[16]) a constant; fx, fy and
// the clamp limits are constants, a clamped tx depends on the view through d only, and row 3 of the view is held
// at (0, 0, 0, 1). With mh = (mean, 1):
//   dview[r][c] = g_r mh[c],  g = (dpx, dpy, -dd) + the first three entries of proj^T (dphx, dphy, 0, dphw)
//   dview[r][k] += (J^T dT)[r][k], k < 3: J00 dT[0][k]; J11 dT[1][k]; J02 dT[0][k] + J12 dT[1][k]
// GbCam stays as it is (its layout is packed by the host tests): proj comes beside it.
template <bool DEPTH = false, bool POSE = false>
PTGS_HD void gs_project_backward_one(const GbCam& cam, const float* mean, const float* scale, const float* rot,
                                     float dgx, float dgy, float da, float db, float dc, float* dm, float* dsc,
                                     float* dq, float dinvd = 0.0f, const float* proj = nullptr,
                                     float* dview = nullptr) {
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
  // cov = A A^T + 0.3 I with A = T R S, column by column: column k is sc[k] (ux, uy)[k], the image of the
  // Gaussian's axis k. Sigma = R S^2 R^T is never formed (see the note above the function).
  float ux[3], uy[3], pxx[3], pxy[3], pyy[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    ux[k] = (T[0][0] * R[0][k] + T[0][1] * R[1][k]) + T[0][2] * R[2][k];
    uy[k] = (T[1][0] * R[0][k] + T[1][1] * R[1][k]) + T[1][2] * R[2][k];
    const float ax = ux[k] * sc[k], ay = uy[k] * sc[k];
    pxx[k] = ax * ax;
    pxy[k] = ax * ay;
    pyy[k] = ay * ay;
  }
  // det(A A^T + 0.3 I) = |row 0 x row 1|^2 + 0.3 tr(A A^T) + 0.09: positive terms only (Cauchy-Binet)
  const float n01 = (ux[0] * uy[1] - ux[1] * uy[0]) * (sc[0] * sc[1]);
  const float n02 = (ux[0] * uy[2] - ux[2] * uy[0]) * (sc[0] * sc[2]);
  const float n12 = (ux[1] * uy[2] - ux[2] * uy[1]) * (sc[1] * sc[2]);
  const float exx = (pxx[0] + pxx[1]) + pxx[2], exy = (pxy[0] + pxy[1]) + pxy[2], eyy = (pyy[0] + pyy[1]) + pyy[2];
  const float det_inv = 1.0f / (((n01 * n01 + n02 * n02) + n12 * n12) + (0.3f * (exx + eyy) + 0.09f));
  const float a = (eyy + 0.3f) * det_inv, b = -exy * det_inv, c = (exx + 0.3f) * det_inv;  // the conic Q = cov^-1
  // ---- conic -> cov -> A: dL = tr(Mc dcov) with Mc = -Q G Q, G = [[da, db/2], [db/2, dc]]; dL/dA = 2 Mc A.
  // Column k: Q A_k = sc[k] adj(B_k) (ux, uy)[k] / det with B_k = cov - A_k A_k^T, then G, then Q. ----
  const float hb = 0.5f * db;
  float dAx[3], dAy[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int i = (k + 1) % 3, j = (k + 2) % 3;
    const float bxx = (pxx[i] + pxx[j]) + 0.3f, bxy = pxy[i] + pxy[j], byy = (pyy[i] + pyy[j]) + 0.3f;
    const float wx = (byy * ux[k] - bxy * uy[k]) * det_inv, wy = (bxx * uy[k] - bxy * ux[k]) * det_inv;
    const float gx = da * wx + hb * wy, gy = hb * wx + dc * wy;
    const float f = -2.0f * sc[k];
    dsc[k] = f * (wx * gx + wy * gy);  // dL/dA_k . d A_k / d sc[k]
    dAx[k] = (f * sc[k]) * (a * gx + b * gy);  // dL/dA_k times sc[k] (both uses below carry that factor)
    dAy[k] = (f * sc[k]) * (b * gx + c * gy);
  }
  // ---- A = T R S: dL/dT = dL/dA (R S)^T, dL/dR = T^T dL/dA S ----
  float dT[2][3], dR[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    dT[0][r] = (dAx[0] * R[r][0] + dAx[1] * R[r][1]) + dAx[2] * R[r][2];
    dT[1][r] = (dAy[0] * R[r][0] + dAy[1] * R[r][1]) + dAy[2] * R[r][2];
#pragma unroll
    for (int k = 0; k < 3; ++k) dR[r][k] = T[0][r] * dAx[k] + T[1][r] * dAy[k];
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
  if (POSE) {
    const float mh[4] = {mx, my, mz, 1.0f};
    const float g3[3] = {dpx, dpy, -dd};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      // d ph / d (view (mean, 1))[r] = column r of proj
      const float gr = g3[r] + ((dphx * proj[4 * r] + dphy * proj[4 * r + 1]) + dphw * proj[4 * r + 3]);
#pragma unroll
      for (int c = 0; c < 4; ++c) dview[4 * r + c] = gr * mh[c];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      dview[k] += J00 * dT[0][k];
      dview[4 + k] += J11 * dT[1][k];
      dview[8 + k] += J02 * dT[0][k] + J12 * dT[1][k];
    }
  }
}

}  // namespace ptgs
