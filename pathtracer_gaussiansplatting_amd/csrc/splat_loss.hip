// splat_loss.hip — the 3DGS training loss (Kerbl et al.): (1 - lambda) mean|a - b| + lambda (1 - mean SSIM(a, b))
// over the RGB channels of an RGBA32F image a and a target b, and its gradient with respect to a. The contract is
// in include/ptgs/ptgs.h, the per-pixel arithmetic in splat_loss_math.h (host / device).
//
// Two launches and a tiny one. A workgroup of 256 owns a tile of LS_T x LS_T = 32 x 32 pixels.
//   gs_loss_stats_kernel  stages a and b (three channels) with the 5-pixel halo, 42 x 42, zero outside the image;
//     per channel it convolves a, b, a a, b b, a b along x into 42 rows x 32 columns, then along y, evaluates the
//     SSIM map and its partials (dm/dmu1, dm/ds1, dm/ds12) at the tile's pixels, stores the partials to the
//     workspace (nine planes of W x H floats) and sums |a - b| and m: per work-item in f32 (at most 12 terms),
//     then over the workgroup in f64 by a fixed tree. One (sum|a - b|, sum m) pair per workgroup.
//   gs_loss_grad_kernel   stages one channel's three partial maps with the halo, convolves them (the window is
//     symmetric, so the adjoint of the correlation is the correlation), and writes
//     grad = k1 sign(a - b) - k2 (conv(dmu1) + 2 a conv(ds1) + b conv(ds12)), alpha 0, as one float4 per pixel.
//   gs_loss_final_kernel  one workgroup walks the pairs LS_STEP = 256 at a time, each work-item carrying its own
//     f64 sums, then the same fixed tree; writes loss_out. No atomics anywhere: two runs are bit-equal.
//
// A work-item convolves LS_R = 4 neighbouring outputs from 14 samples held in registers (3.5 LDS reads per output
// and pass instead of 11). Along x an item is (row, column group) with consecutive lanes on consecutive rows; the
// staged rows have an odd pitch (43 floats), so the lanes of a 32-lane group read 32 different banks. Along y
// consecutive lanes own consecutive columns (pitch 33), which is conflict-free for any pitch.
// LDS: the statistics kernel 2 x 3 x 42 x 43 x 4 (a, b) + 5 x 42 x 33 x 4 (row pass) + 4096 (tree) = 75 160 B:
// two workgroups per CU; the gradient kernel 3 x 42 x 43 x 4 + 3 x 42 x 33 x 4 = 38 304 B: four per CU by LDS,
// three by its registers. Each work-item issues all of its staging loads before the LDS stores.
// Bytes per pixel: 16 + 4 C read and 36 written by the first kernel, 36 + 16 + 4 C read and 16 written by the
// second (halo re-reads come from the caches).
//
// The depth regulariser (ptgs_image_loss_invdepth_l1) is at the end: an L1 on rendered inverse depth against a
// view-depth target, one streaming kernel and a final sum of the same kind.
#include "splat_loss.h"

#include "dev_buf.h"
#include "splat_loss_math.h"

namespace ptgs {
namespace {

constexpr uint32_t LS_T = 32, LS_WG = 256, LS_R = 4;
constexpr uint32_t LS_S = LS_T + 2 * LOSS_HALO;  // staged rows / columns
constexpr uint32_t LS_PS = LS_S + 1;             // pitch of a staged row (odd)
constexpr uint32_t LS_PH = LS_T + 1;             // pitch of a row of the x pass
constexpr uint32_t LS_CG = LS_T / LS_R;          // column groups of a row
constexpr uint32_t LS_ITEMS = LS_S * LS_CG;      // (row, column group) items of the x pass
constexpr uint32_t LS_N = LS_R + LOSS_WIN - 1;   // samples of LS_R neighbouring outputs
constexpr uint32_t LS_STAGE = (LS_S * LS_S + LS_WG - 1) / LS_WG;  // staged pixels per work-item
constexpr uint32_t LS_STEP = 256;                // pairs the final sum takes per step
constexpr uint32_t LS_MAPS = 9;                  // planes of the workspace: [channel][dmu1, ds1, ds12]
static_assert(LS_WG == LS_T * (LS_T / LS_R), "one work-item per column and group of LS_R rows");

struct LsRgb {
  float c[3];
};

// channels 0..2 of pixel p of an array with `ch` floats per pixel (vec: ch == 4 and the base 16-byte aligned)
__device__ __forceinline__ LsRgb ls_load_rgb(const float* __restrict__ base, size_t p, uint32_t ch, bool vec) {
  LsRgb r;
  if (vec) {
    const float4 v = reinterpret_cast<const float4*>(base)[p];
    r.c[0] = v.x;
    r.c[1] = v.y;
    r.c[2] = v.z;
  } else {
    r.c[0] = base[p * ch];
    r.c[1] = base[p * ch + 1];
    r.c[2] = base[p * ch + 2];
  }
  return r;
}

// the workgroup's sums of v0 and v1 in a fixed order; valid in work-item 0
__device__ __forceinline__ void ls_tree_sum(double (*red)[LS_WG], double& v0, double& v1) {
  const uint32_t t = threadIdx.x;
  red[0][t] = v0;
  red[1][t] = v1;
  __syncthreads();
  for (uint32_t o = LS_WG / 2; o > 0; o >>= 1) {
    if (t < o) {
      red[0][t] += red[0][t + o];
      red[1][t] += red[1][t + o];
    }
    __syncthreads();
  }
  v0 = red[0][0];
  v1 = red[1][0];
}

template <int C, bool MAPS>
__global__ __launch_bounds__(LS_WG) void gs_loss_stats_kernel(const float* __restrict__ image,
                                                             const float* __restrict__ target, uint32_t W, uint32_t H,
                                                             bool vec_image, bool vec_target, float* __restrict__ maps,
                                                             double* __restrict__ partials) {
  __shared__ float sa[3][LS_S * LS_PS];
  __shared__ float sb[3][LS_S * LS_PS];
  __shared__ float sh[5][LS_S * LS_PH];
  __shared__ double red[2][LS_WG];
  const uint32_t t = threadIdx.x;
  const int x0 = (int)(blockIdx.x * LS_T), y0 = (int)(blockIdx.y * LS_T);
  {  // every load of the work-item first, then the LDS stores: one exposed memory latency per tile
    LsRgb a[LS_STAGE], b[LS_STAGE];
#pragma unroll
    for (uint32_t it = 0; it < LS_STAGE; ++it) {
      const uint32_t i = t + it * LS_WG, ly = i / LS_S, lx = i - ly * LS_S;
      const int gx = x0 + (int)lx - LOSS_HALO, gy = y0 + (int)ly - LOSS_HALO;
      a[it] = b[it] = LsRgb{{0.0f, 0.0f, 0.0f}};
      if (i < LS_S * LS_S && gx >= 0 && gy >= 0 && gx < (int)W && gy < (int)H) {
        const size_t p = (size_t)gy * W + (size_t)gx;
        a[it] = ls_load_rgb(image, p, 4, vec_image);
        b[it] = ls_load_rgb(target, p, C, C == 4 && vec_target);
      }
    }
#pragma unroll
    for (uint32_t it = 0; it < LS_STAGE; ++it) {
      const uint32_t i = t + it * LS_WG, ly = i / LS_S, lx = i - ly * LS_S;
      if (i < LS_S * LS_S) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          sa[c][ly * LS_PS + lx] = a[it].c[c];
          sb[c][ly * LS_PS + lx] = b[it].c[c];
        }
      }
    }
  }
  __syncthreads();
  const uint32_t x = t & (LS_T - 1), rg = t / LS_T;
  const size_t plane = (size_t)W * H;
  float sum_l1 = 0.0f, sum_m = 0.0f;
  for (int c = 0; c < 3; ++c) {
    for (uint32_t i = t; i < LS_ITEMS; i += LS_WG) {
      const uint32_t cg = i / LS_S, r = i - cg * LS_S;
      const float* pa = &sa[c][r * LS_PS + cg * LS_R];
      const float* pb = &sb[c][r * LS_PS + cg * LS_R];
      float a[LS_N], b[LS_N], aa[LS_N], bb[LS_N], ab[LS_N];
#pragma unroll
      for (uint32_t k = 0; k < LS_N; ++k) {
        a[k] = pa[k];
        b[k] = pb[k];
        aa[k] = a[k] * a[k];
        bb[k] = b[k] * b[k];
        ab[k] = a[k] * b[k];
      }
      const uint32_t o = r * LS_PH + cg * LS_R;
#pragma unroll
      for (uint32_t j = 0; j < LS_R; ++j) {
        sh[0][o + j] = loss_tap11(a + j);
        sh[1][o + j] = loss_tap11(b + j);
        sh[2][o + j] = loss_tap11(aa + j);
        sh[3][o + j] = loss_tap11(bb + j);
        sh[4][o + j] = loss_tap11(ab + j);
      }
    }
    __syncthreads();
    float st[5][LS_R];
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      float v[LS_N];
#pragma unroll
      for (uint32_t k = 0; k < LS_N; ++k) v[k] = sh[s][(rg * LS_R + k) * LS_PH + x];
#pragma unroll
      for (uint32_t j = 0; j < LS_R; ++j) st[s][j] = loss_tap11(v + j);
    }
#pragma unroll
    for (uint32_t j = 0; j < LS_R; ++j) {
      const uint32_t ly = rg * LS_R + j;
      const uint32_t gx = (uint32_t)x0 + x, gy = (uint32_t)y0 + ly;
      if (gx < W && gy < H) {
        const LossPixel p = loss_ssim_pixel(st[0][j], st[1][j], st[2][j], st[3][j], st[4][j]);
        const uint32_t at = (ly + LOSS_HALO) * LS_PS + x + LOSS_HALO;
        sum_m += p.m;
        sum_l1 += fabsf(sa[c][at] - sb[c][at]);
        if (MAPS) {
          const size_t px = (size_t)gy * W + gx;
          maps[(size_t)(c * 3 + 0) * plane + px] = p.d_mu1;
          maps[(size_t)(c * 3 + 1) * plane + px] = p.d_s1;
          maps[(size_t)(c * 3 + 2) * plane + px] = p.d_s12;
        }
      }
    }
    __syncthreads();  // (the next channel's x pass overwrites sh)
  }
  double d_l1 = (double)sum_l1, d_m = (double)sum_m;
  ls_tree_sum(red, d_l1, d_m);
  if (t == 0) {
    const size_t wg = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partials[2 * wg] = d_l1;
    partials[2 * wg + 1] = d_m;
  }
}

template <int C>
__global__ __launch_bounds__(LS_WG) void gs_loss_grad_kernel(const float* __restrict__ image,
                                                            const float* __restrict__ target, uint32_t W, uint32_t H,
                                                            bool vec_image, bool vec_target, bool vec_grad,
                                                            const float* __restrict__ maps, float k1, float k2,
                                                            float* __restrict__ grad) {
  __shared__ float sm[3][LS_S * LS_PS];
  __shared__ float sh[3][LS_S * LS_PH];
  const uint32_t t = threadIdx.x;
  const int x0 = (int)(blockIdx.x * LS_T), y0 = (int)(blockIdx.y * LS_T);
  const uint32_t x = t & (LS_T - 1), rg = t / LS_T;
  const uint32_t gx = (uint32_t)x0 + x;
  const size_t plane = (size_t)W * H;
  LsRgb a[LS_R], b[LS_R];
  float out[LS_R][3];
#pragma unroll
  for (uint32_t j = 0; j < LS_R; ++j) {
    const uint32_t gy = (uint32_t)y0 + rg * LS_R + j;
    a[j] = b[j] = LsRgb{{0.0f, 0.0f, 0.0f}};
    if (gx < W && gy < H) {
      const size_t p = (size_t)gy * W + gx;
      a[j] = ls_load_rgb(image, p, 4, vec_image);
      b[j] = ls_load_rgb(target, p, C, C == 4 && vec_target);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    {  // (loads first, as in the statistics kernel)
      float v[LS_STAGE][3];
#pragma unroll
      for (uint32_t it = 0; it < LS_STAGE; ++it) {
        const uint32_t i = t + it * LS_WG, ly = i / LS_S, lx = i - ly * LS_S;
        const int sx = x0 + (int)lx - LOSS_HALO, sy = y0 + (int)ly - LOSS_HALO;
        v[it][0] = v[it][1] = v[it][2] = 0.0f;
        if (i < LS_S * LS_S && sx >= 0 && sy >= 0 && sx < (int)W && sy < (int)H) {
          const size_t p = (size_t)sy * W + (size_t)sx;
#pragma unroll
          for (int k = 0; k < 3; ++k) v[it][k] = maps[(size_t)(c * 3 + k) * plane + p];
        }
      }
#pragma unroll
      for (uint32_t it = 0; it < LS_STAGE; ++it) {
        const uint32_t i = t + it * LS_WG, ly = i / LS_S, lx = i - ly * LS_S;
        if (i < LS_S * LS_S) {
#pragma unroll
          for (int k = 0; k < 3; ++k) sm[k][ly * LS_PS + lx] = v[it][k];
        }
      }
    }
    __syncthreads();
    for (uint32_t i = t; i < 3 * LS_ITEMS; i += LS_WG) {
      const uint32_t k = i / LS_ITEMS, ii = i - k * LS_ITEMS;
      const uint32_t cg = ii / LS_S, r = ii - cg * LS_S;
      const float* ps = &sm[k][r * LS_PS + cg * LS_R];
      float v[LS_N];
#pragma unroll
      for (uint32_t q = 0; q < LS_N; ++q) v[q] = ps[q];
      const uint32_t o = r * LS_PH + cg * LS_R;
#pragma unroll
      for (uint32_t j = 0; j < LS_R; ++j) sh[k][o + j] = loss_tap11(v + j);
    }
    __syncthreads();  // (also orders this channel's reads of sm before the next channel's staging)
    float g[3][LS_R];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float v[LS_N];
#pragma unroll
      for (uint32_t q = 0; q < LS_N; ++q) v[q] = sh[k][(rg * LS_R + q) * LS_PH + x];
#pragma unroll
      for (uint32_t j = 0; j < LS_R; ++j) g[k][j] = loss_tap11(v + j);
    }
#pragma unroll
    for (uint32_t j = 0; j < LS_R; ++j) {
      const float G = fmaf(b[j].c[c], g[2][j], fmaf(2.0f * a[j].c[c], g[1][j], g[0][j]));
      out[j][c] = k1 * loss_sign(a[j].c[c] - b[j].c[c]) - k2 * G;
    }
    // (sh is next written after the following channel's staging barrier, which every work-item reaches only
    // after these reads)
  }
#pragma unroll
  for (uint32_t j = 0; j < LS_R; ++j) {
    const uint32_t gy = (uint32_t)y0 + rg * LS_R + j;
    if (gx < W && gy < H) {
      const size_t p = (size_t)gy * W + gx;
      if (vec_grad) {
        reinterpret_cast<float4*>(grad)[p] = make_float4(out[j][0], out[j][1], out[j][2], 0.0f);
      } else {
        grad[4 * p] = out[j][0];
        grad[4 * p + 1] = out[j][1];
        grad[4 * p + 2] = out[j][2];
        grad[4 * p + 3] = 0.0f;
      }
    }
  }
}

__global__ __launch_bounds__(LS_WG) void gs_loss_final_kernel(const double* __restrict__ partials, uint32_t nwg,
                                                             double inv_n, float lambda, float* __restrict__ loss_out) {
  __shared__ double red[2][LS_WG];
  const uint32_t t = threadIdx.x;
  double s_l1 = 0.0, s_m = 0.0;
  for (uint32_t c0 = 0; c0 < nwg; c0 += LS_STEP) {
    const uint32_t w = c0 + t;
    if (w < nwg) {
      s_l1 += partials[2 * (size_t)w];
      s_m += partials[2 * (size_t)w + 1];
    }
  }
  ls_tree_sum(red, s_l1, s_m);
  if (t == 0) {
    const double l1 = s_l1 * inv_n, ssim = s_m * inv_n, lam = (double)lambda;
    loss_out[0] = (float)((1.0 - lam) * l1 + lam * (1.0 - ssim));
    loss_out[1] = (float)l1;
    loss_out[2] = (float)ssim;
    loss_out[3] = 0.0f;
  }
}
static_assert(LS_STEP == LS_WG, "the final sum's step is its workgroup");

bool ls_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The inverse-depth L1 (ptgs_image_loss_invdepth_l1). A workgroup owns LD_PER consecutive pixels, a work-item
// LD_PER / LS_WG of them, LS_WG apart (coalesced). term = |D - 1.0f / t| in f32 (IEEE divide, no contraction)
// where t > 0 (+inf included: 1 / t = 0), 0 where t <= 0 or t is NaN; the terms and the supervised count are
// summed in f64, per work-item in pixel order, then by the fixed tree: one (sum, count) pair per workgroup.
constexpr uint32_t LD_PER = 4 * LS_WG;

__global__ __launch_bounds__(LS_WG) void gs_loss_invdepth_kernel(const float* __restrict__ invdepth,
                                                                const float* __restrict__ target, size_t pixels,
                                                                float k, float* __restrict__ grad,
                                                                double* __restrict__ partials) {
  __shared__ double red[2][LS_WG];
  const uint32_t t = threadIdx.x;
  double sum = 0.0, count = 0.0;
  for (uint32_t it = 0; it < LD_PER / LS_WG; ++it) {
    const size_t p = (size_t)blockIdx.x * LD_PER + it * LS_WG + t;
    if (p < pixels) {
      const float tz = target[p];
      float g = 0.0f;
      if (tz > 0.0f) {  // (false for NaN)
        const float diff = invdepth[p] - 1.0f / tz;
        sum += (double)fabsf(diff);
        count += 1.0;
        g = k * loss_sign(diff);
      }
      if (grad) grad[p] = g;
    }
  }
  ls_tree_sum(red, sum, count);
  if (t == 0) {
    partials[2 * (size_t)blockIdx.x] = sum;
    partials[2 * (size_t)blockIdx.x + 1] = count;
  }
}

__global__ __launch_bounds__(LS_WG) void gs_loss_invdepth_final_kernel(const double* __restrict__ partials,
                                                                      uint32_t nwg, double pixels, float weight,
                                                                      float* __restrict__ terms) {
  __shared__ double red[2][LS_WG];
  const uint32_t t = threadIdx.x;
  double sum = 0.0, count = 0.0;
  for (uint32_t c0 = 0; c0 < nwg; c0 += LS_STEP) {
    const uint32_t w = c0 + t;
    if (w < nwg) {
      sum += partials[2 * (size_t)w];
      count += partials[2 * (size_t)w + 1];
    }
  }
  ls_tree_sum(red, sum, count);
  if (t == 0) {
    const double mean = sum / pixels;
    terms[0] = (float)((double)weight * mean);
    terms[1] = (float)mean;
    terms[2] = (float)count;
    terms[3] = 0.0f;
  }
}

}  // namespace

struct LossWorkspace {
  DevBuf maps;            // float: LS_MAPS planes of W x H
  DevBuf partials;        // double: (sum |a - b|, sum m) per workgroup
  DevBuf depth_partials;  // double: (sum |D - 1/t|, supervised pixels) per workgroup of the inverse-depth L1
};

LossWorkspace* loss_workspace_create() { return new LossWorkspace(); }

void loss_workspace_destroy(LossWorkspace* ws) { delete ws; }

hipError_t image_loss_l1_dssim(LossWorkspace* ws, const float* image, const float* target, uint32_t channels,
                               uint32_t W, uint32_t H, float lambda, float grad_scale, float* loss_out, float* grad,
                               hipStream_t s) {
  if (W == 0 || H == 0 || W > LOSS_MAX_SIDE || H > LOSS_MAX_SIDE || (channels != 3 && channels != 4))
    return hipErrorInvalidValue;
  const dim3 grid((W + LS_T - 1) / LS_T, (H + LS_T - 1) / LS_T);
  const uint32_t nwg = grid.x * grid.y;  // (<= 512 * 512)
  const size_t pixels = (size_t)W * H;
  hipError_t e;
  // (grown to the exact size: no slack)
  if ((e = ws->partials.ensure(2 * (size_t)nwg * sizeof(double), 0)) != hipSuccess) return e;
  if (grad && (e = ws->maps.ensure(LS_MAPS * pixels * sizeof(float), 0)) != hipSuccess) return e;
  float* const maps = ws->maps.as<float>();
  double* const partials = ws->partials.as<double>();
  const bool vi = ls_aligned16(image), vt = ls_aligned16(target);
  if (grad) {
    if (channels == 4)
      gs_loss_stats_kernel<4, true><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, maps, partials);
    else
      gs_loss_stats_kernel<3, true><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, maps, partials);
  } else {
    if (channels == 4)
      gs_loss_stats_kernel<4, false><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, nullptr, partials);
    else
      gs_loss_stats_kernel<3, false><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, nullptr, partials);
  }
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const double n = 3.0 * (double)pixels;
  if (grad) {
    const float k1 = (float)((double)grad_scale * (1.0 - (double)lambda) / n);
    const float k2 = (float)((double)grad_scale * (double)lambda / n);
    if (channels == 4)
      gs_loss_grad_kernel<4><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, ls_aligned16(grad), maps, k1, k2,
                                                    grad);
    else
      gs_loss_grad_kernel<3><<<grid, LS_WG, 0, s>>>(image, target, W, H, vi, vt, ls_aligned16(grad), maps, k1, k2,
                                                    grad);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  gs_loss_final_kernel<<<1, LS_WG, 0, s>>>(partials, nwg, 1.0 / n, lambda, loss_out);
  return hipGetLastError();
}

hipError_t image_loss_invdepth_l1(LossWorkspace* ws, const float* invdepth, const float* target_depth, uint32_t W,
                                  uint32_t H, float weight, float grad_scale, float* terms, float* grad, hipStream_t s) {
  if (W == 0 || H == 0 || W > LOSS_MAX_SIDE || H > LOSS_MAX_SIDE) return hipErrorInvalidValue;
  const size_t pixels = (size_t)W * H;
  const uint32_t nwg = (uint32_t)((pixels + LD_PER - 1) / LD_PER);  // (<= 2^18)
  hipError_t e;
  if ((e = ws->depth_partials.ensure(2 * (size_t)nwg * sizeof(double), 0)) != hipSuccess) return e;
  double* const partials = ws->depth_partials.as<double>();
  const float k = (float)((double)weight * (double)grad_scale / (double)pixels);
  gs_loss_invdepth_kernel<<<nwg, LS_WG, 0, s>>>(invdepth, target_depth, pixels, k, grad, partials);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  gs_loss_invdepth_final_kernel<<<1, LS_WG, 0, s>>>(partials, nwg, (double)pixels, weight, terms);
  return hipGetLastError();
}

}  // namespace ptgs
