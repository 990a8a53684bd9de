// splat_preprocess.h — stage: the per-Gaussian preprocess (frustum cull, EWA projection, conic, radius, tile
// rect, blend record) that both front ends run per work-item, and the chunk cull of tile-row-restricted
// frames. Relies on SplatCam and the tile constants (splat_plan.h) and the exact math of detmath.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "detmath.h"
#include "splat_plan.h"

namespace ptgs {

__device__ __forceinline__ v4 mv4(const float* m, float x, float y, float z, float w) {
  return mk4(((m[0] * x + m[4] * y) + m[8] * z) + m[12] * w, ((m[1] * x + m[5] * y) + m[9] * z) + m[13] * w,
             ((m[2] * x + m[6] * y) + m[10] * z) + m[14] * w, ((m[3] * x + m[7] * y) + m[11] * z) + m[15] * w);
}

__device__ __forceinline__ float ndc2pix(float v, int S) { return ((v + 1.0f) * (float)S - 1.0f) * 0.5f; }

struct PreArgs {
  const float *means, *scales, *rots, *opac, *colors;
  uint32_t n;
  float2* means2d;
  float* depths;      // walk order (i): the three-launch scatter's depths
  float* dbg_depths;  // caller order (o): ptgs_splat_get_buffers
  float4* conic_o;
  int* radii;
  uint32_t* touched;
  ushort4* rects;
  float4* rec;
  const uint32_t* ids;  // caller's index of Gaussian i (NULL: i): keys, values, records and the
                        // per-Gaussian outputs use it, so a reordered set renders like the original
  uint32_t* bad_ids;    // pinned host word set to 1 when an id is >= n (the Gaussian is dropped)
  const uint8_t* cskip;  // per 256-Gaussian chunk: 1 = its bound misses the frame's rows (gs_chunk_cull_kernel)
  const float4* cbounds;  // the chunk bounds themselves (the fused front end tests its own chunk: no cull launch)
};

// Image stores stream past L2 (non-temporal): C2 0.0686 -> 0.0677 ms, fewer dirty lines at the kernel end.
// (Non-temporal blend records and key rows measured slower: the blend reads both right after.)
__device__ __forceinline__ void gs_st4_nt(float4* p, const float4& v) {
  typedef float f4v __attribute__((ext_vector_type(4)));
  __builtin_nontemporal_store(f4v{v.x, v.y, v.z, v.w}, reinterpret_cast<f4v*>(p));
}
// (Write-through (sc1) stores, which leave the XCD's L2 at once instead of at the kernel-end release,
// measured slower for every output: image 0.0633, key rows 0.0585, records 0.0603, all 0.0679 vs 0.0565 ms.)

// Upper bound (px) of the 3-sigma radius of a Gaussian of largest scale s at view-space point (x, y, d),
// d > 0.2: radius = ceil(3 sqrt(l1)) with l1 <= lambda_max(cov) + sqrt(0.1) (the max(0.1, .) clamp of
// gs_preprocess_one), cov = T Sigma T^T + 0.3 I, T = J W, so lambda_max(cov) <= |J|_2^2 |W|_2^2 s^2 + 0.3
// with |J|_2^2 = max(fx, fy)^2 (1 + a^2 + b^2) / d^2 (J = diag(fx, fy) / d [[1, 0, -a], [0, 1, -b]], a and b
// the clamped x / d and y / d of the EWA Jacobian). 1% and 2 px absorb the float rounding of both sides.
__device__ __forceinline__ float gs_radius_bound(const SplatCam& cam, float a, float b, float d, float s) {
  const float lam = cam.fmax2 * ((1.0f + a * a) + b * b) / (d * d) * cam.w2 * (s * s);
  return 3.0f * sqrtf(1.01f * (lam + 0.62f)) + 2.0f;
}

// Row pre-cull of a tile-row-restricted frame (cam.rowcull): from the mean and the scales only (one load
// round trip before the rotation / opacity / colour loads), true when the Gaussian cannot reach the
// frame's tile rows: its rect rows [(int)((y - r) / 16), (int)((y + r + 15) / 16)) miss [row_begin,
// row_end) for every r <= the radius bound (the exact rect is then empty: the skip is exact). False for
// d <= 0.2 and non-finite values (the exact path decides).
__device__ __forceinline__ bool gs_row_miss(const SplatCam& cam, float mx, float my, float mz, float sx, float sy,
                                            float sz) {
  const v4 pv = mv4(cam.view, mx, my, mz, 1.0f);
  const float d = -pv.z;
  if (!(d > 0.2f)) return false;
  const v4 ph = mv4(cam.mvp, mx, my, mz, 1.0f);
  const float y = ndc2pix(ph.y * (1.0f / (ph.w + 0.0000001f)), (int)cam.H);
  const float limx = 1.3f * cam.tan_fovx, limy = 1.3f * cam.tan_fovy;
  const float a = fminf(limx, fmaxf(-limx, pv.x / d)), b = fminf(limy, fmaxf(-limy, pv.y / d));
  const float R = gs_radius_bound(cam, a, b, d, fmaxf(fabsf(sx), fmaxf(fabsf(sy), fabsf(sz))));
  const float t = (float)GS_BLOCK_Y;
  return (y + R + t < t * (float)cam.row_begin) || (y - R - t > t * (float)cam.row_end);
}

// One Gaussian: frustum cull (d <= 0.2), Sigma = R S^2 R^T, EWA Sigma' = J W Sigma W^T J^T + 0.3,
// conic, 3-sigma radius, tile rect (returned; empty if culled) and, with STORE, every per-Gaussian
// output incl. the blend record. (Blocks of other bands recompute the rect without storing.)
// ROWCULL: a tile-row-restricted frame (cam.rowcull), its own instantiation of the front-end kernels (the
// full frame's preprocess keeps its single load round trip, unchanged code)
template <bool STORE, bool ROWCULL = false>
__device__ __forceinline__ ushort4 gs_preprocess_one(const SplatCam& cam, const PreArgs& A, uint32_t i,
                                                     float* dep_out = nullptr) {
  const float* __restrict__ means = A.means;
  const float* __restrict__ scales = A.scales;
  const float* __restrict__ rots = A.rots;
  const float* __restrict__ opac = A.opac;
  const float* __restrict__ colors = A.colors;
  float2* __restrict__ means2d = A.means2d;
  float* __restrict__ depths = A.depths;
  float4* __restrict__ conic_o = A.conic_o;
  int* __restrict__ radii = A.radii;
  uint32_t* __restrict__ touched = A.touched;
  ushort4* __restrict__ rects = A.rects;
  float4* __restrict__ rec = A.rec;
  const ushort4 none = make_ushort4(0, 0, 0, 0);
  // per-Gaussian outputs: rec (the blend's records) always; rects / depths (the three-launch scatter's
  // walk, at i) and radii / touched / means2d / conic (ptgs_splat_get_buffers) when their pointers are
  // set (the fused path without PTGS_FLAG_SPLAT_PUBLISH leaves them out)
  const uint32_t o = A.ids ? A.ids[i] : i;
  float mx = means[3 * i], my = means[3 * i + 1], mz = means[3 * i + 2];
  float sx = scales[3 * i], sy = scales[3 * i + 1], sz = scales[3 * i + 2];
  float qr = 0.0f, qx = 0.0f, qy = 0.0f, qz = 0.0f, op = 0.0f, cr = 0.0f, cg = 0.0f, cbl = 0.0f;
  bool miss = false;
  if (!ROWCULL) {
    // every input is loaded here, with the id and before the id check and the depth test: one memory round
    // trip per Gaussian (loads behind either branch were issued only once the id / the means had arrived)
    qr = rots[4 * i]; qx = rots[4 * i + 1]; qy = rots[4 * i + 2]; qz = rots[4 * i + 3];
    op = opac[i];
    if (STORE) {
      cr = colors[3 * i];
      cg = colors[3 * i + 1];
      cbl = colors[3 * i + 2];
      asm volatile("" : "+v"(cr), "+v"(cg), "+v"(cbl));
    }
    // (the empty asm needs the values here, so the compiler cannot sink the loads behind the branches)
    asm volatile("" : "+v"(mx), "+v"(my), "+v"(mz), "+v"(qr), "+v"(qx), "+v"(qy), "+v"(qz), "+v"(sx), "+v"(sy),
                 "+v"(sz), "+v"(op));
  } else {
    // a tile-row shard: most Gaussians miss its rows; the rest of the inputs are loaded only for those
    // whose radius bound reaches them (a second round trip for them, none for the others)
    miss = gs_row_miss(cam, mx, my, mz, sx, sy, sz);
    if (!miss) {
      qr = rots[4 * i]; qx = rots[4 * i + 1]; qy = rots[4 * i + 2]; qz = rots[4 * i + 3];
      op = opac[i];
      if (STORE) {
        cr = colors[3 * i];
        cg = colors[3 * i + 1];
        cbl = colors[3 * i + 2];
      }
    }
  }
  if (STORE && rects) rects[i] = none;  // empty rect: the scatter reads rects only
  if (o >= A.n) {  // ids must be a permutation of [0, n): an index outside it is dropped, not written
    if (STORE) __atomic_store_n(A.bad_ids, 1u, __ATOMIC_RELAXED);  // (reported by the next call)
    return none;
  }
  if (STORE && radii) {
    radii[o] = 0;
    touched[o] = 0;
  }
  if (miss) return none;
  // frustum: view-space depth d = -z (RH, camera looks down -Z)
  v4 pv = mv4(cam.view, mx, my, mz, 1.0f);
  float d = -pv.z;
  if (dep_out) *dep_out = d;
  if (d <= 0.2f) return none;
  v4 ph = mv4(cam.mvp, mx, my, mz, 1.0f);
  float pw = 1.0f / (ph.w + 0.0000001f);
  float px = ph.x * pw, py = ph.y * pw;

  // Sigma = R S^2 R^T
  float qn = sqrtx(((qr * qr + qx * qx) + qy * qy) + qz * qz);
  qr = qr / qn; qx = qx / qn; qy = qy / qn; qz = qz / qn;
  float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qr * qz), R02 = 2.0f * (qx * qz + qr * qy);
  float R10 = 2.0f * (qx * qy + qr * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz), R12 = 2.0f * (qy * qz - qr * qx);
  float R20 = 2.0f * (qx * qz - qr * qy), R21 = 2.0f * (qy * qz + qr * qx), R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
  float M00 = R00 * sx, M01 = R01 * sy, M02 = R02 * sz;
  float M10 = R10 * sx, M11 = R11 * sy, M12 = R12 * sz;
  float M20 = R20 * sx, M21 = R21 * sy, M22 = R22 * sz;
  float S00 = (M00 * M00 + M01 * M01) + M02 * M02;
  float S01 = (M00 * M10 + M01 * M11) + M02 * M12;
  float S02 = (M00 * M20 + M01 * M21) + M02 * M22;
  float S11 = (M10 * M10 + M11 * M11) + M12 * M12;
  float S12 = (M10 * M20 + M11 * M21) + M12 * M22;
  float S22 = (M20 * M20 + M21 * M21) + M22 * M22;

  // EWA: J (2x3) at the clamped view-space point, W = view rotation rows
  float limx = 1.3f * cam.tan_fovx, limy = 1.3f * cam.tan_fovy;
  float txtz = pv.x / d, tytz = pv.y / d;
  float tx = fminx(limx, fmaxx(-limx, txtz)) * d;
  float ty = fminx(limy, fmaxx(-limy, tytz)) * d;
  float J00 = cam.fx / d, J02 = (cam.fx * tx) / (d * d);
  float J11 = cam.fy / d, J12 = (cam.fy * ty) / (d * d);
  const float* V = cam.view;  // column-major: row r, col c = V[c*4 + r]
  float T00 = J00 * V[0] + J02 * V[2], T01 = J00 * V[4] + J02 * V[6], T02 = J00 * V[8] + J02 * V[10];
  float T10 = J11 * V[1] + J12 * V[2], T11 = J11 * V[5] + J12 * V[6], T12 = J11 * V[9] + J12 * V[10];
  // cov = T Sigma T^T
  float U00 = (T00 * S00 + T01 * S01) + T02 * S02;
  float U01 = (T00 * S01 + T01 * S11) + T02 * S12;
  float U02 = (T00 * S02 + T01 * S12) + T02 * S22;
  float U10 = (T10 * S00 + T11 * S01) + T12 * S02;
  float U11 = (T10 * S01 + T11 * S11) + T12 * S12;
  float U12 = (T10 * S02 + T11 * S12) + T12 * S22;
  float ca = ((U00 * T00 + U01 * T01) + U02 * T02) + 0.3f;
  float cb = (U00 * T10 + U01 * T11) + U02 * T12;
  float cc = ((U10 * T10 + U11 * T11) + U12 * T12) + 0.3f;

  float det = ca * cc - cb * cb;
  if (det == 0.0f) return none;
  float det_inv = 1.0f / det;
  float4 con = make_float4(cc * det_inv, -cb * det_inv, ca * det_inv, op);
  float mid = 0.5f * (ca + cc);
  float disc = sqrtx(fmaxx(0.1f, mid * mid - det));
  float l1 = mid + disc, l2 = mid - disc;
  float radius = __builtin_ceilf(3.0f * sqrtx(fmaxx(l1, l2)));
  float2 pimg = make_float2(ndc2pix(px, (int)cam.W), ndc2pix(py, (int)cam.H));
  int r = (int)radius;
  int rmin_x = min((int)cam.grid_x, max(0, (int)((pimg.x - (float)r) / (float)GS_BLOCK_X)));
  int rmin_y = min((int)cam.grid_y, max(0, (int)((pimg.y - (float)r) / (float)GS_BLOCK_Y)));
  int rmax_x = min((int)cam.grid_x, max(0, (int)((pimg.x + (float)r + (float)(GS_BLOCK_X - 1)) / (float)GS_BLOCK_X)));
  int rmax_y = min((int)cam.grid_y, max(0, (int)((pimg.y + (float)r + (float)(GS_BLOCK_Y - 1)) / (float)GS_BLOCK_Y)));
  rmin_y = max(rmin_y, (int)cam.row_begin);
  rmax_y = min(rmax_y, (int)cam.row_end);
  // (ex, ey): half-extents of the ellipse where alpha >= 1/255 can hold (power >= -ln(255 o), minus a
  // 1e-3 margin, +1% and +0.01 px): the blend skips whole 8x8 pixel blocks outside that box
  const float skip = -(log2x(255.0f * con.w) * 0.69314718055994531f) - 0.001f;
  const float sq = -2.0f * skip;
  const float ex = sq > 0.0f ? sqrtx(sq * ca) * 1.01f + 0.01f : -1.0f;
  const float ey = sq > 0.0f ? sqrtx(sq * cc) * 1.01f + 0.01f : -1.0f;
  if (cam.tight) {
    // Timed frames bin each Gaussian only to the tiles its alpha box overlaps (pixel x in [16 t, 16 t +
    // 15]); the reference's 3-sigma rectangle (kept for stats and published buffers) also holds tiles
    // where no pixel reaches alpha 1/255: 29% of C2's pairs. The blend skips such a pair (alpha 0:
    // T and colour unchanged, exactly), so the image is the same, bit for bit.
    if (!(sq > 0.0f)) return none;
    rmin_x = max(rmin_x, (int)__builtin_ceilf((pimg.x - ex - (float)(GS_BLOCK_X - 1)) * (1.0f / GS_BLOCK_X)));
    rmax_x = min(rmax_x, (int)__builtin_floorf((pimg.x + ex) * (1.0f / GS_BLOCK_X)) + 1);
    rmin_y = max(rmin_y, (int)__builtin_ceilf((pimg.y - ey - (float)(GS_BLOCK_Y - 1)) * (1.0f / GS_BLOCK_Y)));
    rmax_y = min(rmax_y, (int)__builtin_floorf((pimg.y + ey) * (1.0f / GS_BLOCK_Y)) + 1);
  }
  int area = (rmax_x - rmin_x) * (rmax_y - rmin_y);
  if (rmax_x <= rmin_x || rmax_y <= rmin_y || area == 0) return none;
  const ushort4 rect = make_ushort4((unsigned short)rmin_x, (unsigned short)rmin_y, (unsigned short)rmax_x,
                                    (unsigned short)rmax_y);
  if (!STORE) return rect;
  if (rects) {
    depths[i] = d;
    rects[i] = rect;
  }
  if (radii) {
    A.dbg_depths[o] = d;
    radii[o] = r;
    means2d[o] = pimg;
    conic_o[o] = con;
    touched[o] = (uint32_t)area;
  }
  // Blend record (3 x float4), the form the blend loop consumes:
  //   (x, y, A, B), (C, log2 o, r, g), (b, ex, ey, depth)  with  A = -a/2 log2e, B = -b log2e, C = -c/2 log2e
  // so that z = A dx^2 + B dx dy + C dy^2 + log2 o = power * log2e + log2 o and alpha = min(0.99, 2^z).
  // (ex, ey): the alpha box (above).
  const float L2E = 1.4426950408889634f;
  rec[3 * o] = make_float4(pimg.x, pimg.y, -0.5f * con.x * L2E, -con.y * L2E);
  rec[3 * o + 1] = make_float4(-0.5f * con.z * L2E, __log2f(con.w), cr, cg);
  rec[3 * o + 2] = make_float4(cbl, ex, ey, d);
  return rect;
}

// Can any Gaussian of a chunk touch a tile of the frame's rows (cam.row_begin, row_end) and columns?
// Conservative, from the chunk's bounds (box of the means, largest scale): view depths over the box's
// corners are exact (linear); every mean projects inside the hull of the corners' projections when all
// of them lie in front of the camera; and a Gaussian's 3-sigma radius is at most
// 3 sqrt(|J|_F^2 |W|_F^2 s_max^2 + 0.3 + sqrt(0.1)) + 1 px with |J|_F^2 <= (fx^2 (1 + (1.3 tan_x)^2)
// + fy^2 (1 + (1.3 tan_y)^2)) / d_min^2 (the EWA Jacobian at the clamped point, gs_preprocess_one).
// Margins of 1 % and a tile on every side absorb the rounding. Returns true when the chunk is sure to
// contribute nothing: every mean within the near plane (d <= 0.2), or its bound misses the rows /
// columns. Unbounded cases (a corner close to the camera, non-finite bounds) return false.
__device__ __forceinline__ bool gs_chunk_misses(const SplatCam& cam, const float4 lo, const float4 hi) {
  if (!(isfinite(lo.x) && isfinite(lo.y) && isfinite(lo.z) && isfinite(hi.x) && isfinite(hi.y) && isfinite(hi.z) &&
        isfinite(lo.w)))
    return false;
  float dmin = INFINITY, dmax = -INFINITY, xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
  bool front = true;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = (k & 1) ? hi.x : lo.x, y = (k & 2) ? hi.y : lo.y, z = (k & 4) ? hi.z : lo.z;
    const v4 pv = mv4(cam.view, x, y, z, 1.0f);
    const v4 ph = mv4(cam.mvp, x, y, z, 1.0f);
    const float d = -pv.z;
    dmin = fminf(dmin, d);
    dmax = fmaxf(dmax, d);
    front = front && ph.w > 0.1f;
    const float iw = 1.0f / ph.w;
    const float sx = ndc2pix(ph.x * iw, (int)cam.W), sy = ndc2pix(ph.y * iw, (int)cam.H);
    xmin = fminf(xmin, sx);
    xmax = fmaxf(xmax, sx);
    ymin = fminf(ymin, sy);
    ymax = fmaxf(ymax, sy);
  }
  if (dmax < 0.19f) return true;                // every Gaussian is culled by the near test
  if (dmin < 0.25f || !front) return false;     // too close to bound the projection
  // the largest |x / d|, |y / d| over the box: at its corners (x / d is linear-fractional, d > 0 on the box),
  // clamped like the EWA Jacobian's; the radius bound of gs_radius_bound at the nearest depth
  float amax = 0.0f, bmax = 0.0f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float x = (k & 1) ? hi.x : lo.x, y = (k & 2) ? hi.y : lo.y, z = (k & 4) ? hi.z : lo.z;
    const v4 pv = mv4(cam.view, x, y, z, 1.0f);
    amax = fmaxf(amax, fabsf(pv.x / -pv.z));
    bmax = fmaxf(bmax, fabsf(pv.y / -pv.z));
  }
  amax = fminf(amax * 1.001f, 1.3f * cam.tan_fovx);
  bmax = fminf(bmax * 1.001f, 1.3f * cam.tan_fovy);
  const float R = gs_radius_bound(cam, amax, bmax, dmin * 0.999f, lo.w) + 1.0f;  // px
  if (!isfinite(R)) return false;
  const float t = (float)GS_BLOCK_Y;
  const float r0 = floorf((ymin - R) / t) - 1.0f, r1 = floorf((ymax + R + t) / t) + 1.0f;  // rows [r0, r1]
  const float c0 = floorf((xmin - R) / t) - 1.0f, c1 = floorf((xmax + R + t) / t) + 1.0f;
  return r1 < (float)cam.row_begin || r0 >= (float)cam.row_end || c1 < 0.0f || c0 >= (float)cam.grid_x;
}

// The stores a Gaussian of a skipped chunk owes: the empty rect (the scatter and gs_spill_tile read
// it) and, on a published frame, zero radius / tiles touched
__device__ __forceinline__ void gs_store_skipped(const PreArgs& A, uint32_t i) {
  if (A.rects) A.rects[i] = make_ushort4(0, 0, 0, 0);
  if (A.radii) {
    const uint32_t o = A.ids ? A.ids[i] : i;
    if (o < A.n) {
      A.radii[o] = 0;
      A.touched[o] = 0;
    }
  }
}

// One flag per 256-Gaussian chunk for a tile-row-restricted frame (its own small launch, so that the
// front-end kernels keep no bound arithmetic: they read the flag before loading a chunk)
__global__ __launch_bounds__(256) void gs_chunk_cull_kernel(SplatCam cam, const float4* __restrict__ cb, uint32_t nch,
                                                            uint8_t* __restrict__ skip) {
  const uint32_t c = blockIdx.x * 256u + threadIdx.x;
  if (c < nch) skip[c] = gs_chunk_misses(cam, cb[2 * c], cb[2 * c + 1]) ? 1 : 0;
}

}  // namespace ptgs
