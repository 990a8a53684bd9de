// splat_sh.hip — what a trained 3DGS checkpoint (Kerbl et al. 2023, point_cloud.ply) needs before the
// rasterizer of splat.hip can draw it: view-dependent colours from spherical-harmonic coefficients,
// the activations of the stored scales / opacities, and the SH rows of a reordered copy. The
// rasterizer itself is untouched: it keeps reading ptgs_gaussians.colors, which gs_sh_colors_kernel
// writes on the frame's stream before the splat call.
//
// Colour (computeColorFromSH of the original rasterizer's forward.cu, per channel c, f32, no FMA,
// evaluated left to right as written; sh[k] = the k-th coefficient of the Gaussian's row):
//   d = mean - camera_pos; len = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z); (x, y, z) = len > 0 ? d / len : 0
//   res = C0 * sh[0]
//   degree >= 1:  res = res - C1*y*sh[1] + C1*z*sh[2] - C1*x*sh[3]
//   degree >= 2:  xx = x*x, yy = y*y, zz = z*z, xy = x*y, yz = y*z, xz = x*z
//                 res = res + C2[0]*xy*sh[4] + C2[1]*yz*sh[5] + C2[2]*(2*zz - xx - yy)*sh[6]
//                           + C2[3]*xz*sh[7] + C2[4]*(xx - yy)*sh[8]
//   degree >= 3:  res = res + C3[0]*y*(3*xx - yy)*sh[9] + C3[1]*xy*z*sh[10] + C3[2]*y*(4*zz - xx - yy)*sh[11]
//                           + C3[3]*z*(2*zz - 3*xx - 3*yy)*sh[12] + C3[4]*x*(4*zz - xx - yy)*sh[13]
//                           + C3[5]*z*(xx - yy)*sh[14] + C3[6]*x*(3*xx - yy)*sh[15]
//   color = fmaxx(res + 0.5, 0)
// A product a*b*s is (a*b)*s, a*b*(e)*s is ((a*b)*(e))*s, and a sum adds its terms one by one in index
// order, so the factor in front of sh[k] depends on the direction only and is computed once for the
// three channels.
//
// Memory: the kernel is a stream (12 B mean + 12 K B coefficients in, 12 B out per Gaussian, K =
// (degree + 1)^2). A degree-3 row is 192 B: work-items that each walk their own row give every load
// instruction 64 rows to touch. So a workgroup of 256 work-items loads the contiguous block of its 256
// rows with lane-contiguous loads (16 B per lane; 4 B per lane when the base is not 16-B aligned),
// stages it in LDS and each work-item reads its coefficients from there. The LDS row stride is the row
// length made odd (13 / 27 / 49 dwords): 32 lanes reading coefficient j of 32 consecutive rows then
// hit 32 different banks. Degree 0 has one coefficient per channel and reads it directly.
// -DPTGS_SH_ROWWISE builds the row-per-work-item form (no staging) for the A/B of DESIGN.md.
//
// Training: gs_sh_colors_backward_kernel and gs_activate_backward_kernel differentiate the two (contracts in
// ptgs.h). The colour's backward is the same stream with a second wide array going out (dL/d sh, 12 K B per
// Gaussian): the block is staged in as above, each work-item writes its dL/d sh row over its own LDS row, and
// the block is stored with lane-contiguous stores. The per-Gaussian math of both directions is in
// splat_sh_math.h (host / device).
#include "splat_sh.h"

#include "splat_partial_sum.h"
#include "splat_sh_math.h"

namespace ptgs {
namespace {

constexpr int SH_WG = 256;  // Gaussians per workgroup (the forward pass's chunk granule, splat_plan.h)
constexpr int SH_BATCH = 4;  // staging loads in flight per work-item

// Stage the block's nfl floats (rows of R, contiguous at src) into LDS rows of stride S with lane-contiguous
// loads: float4 plus a dword tail when VEC (src 16-B aligned), dwords otherwise. Nothing at or past src + nfl
// is read. SH_BATCH loads per work-item are issued before the first is stored, to keep bytes in flight.
template <uint32_t R, uint32_t S, bool VEC>
__device__ __forceinline__ void sh_stage_in(float* rows, const float* __restrict__ src, uint32_t nfl, uint32_t t) {
  auto put = [&](uint32_t f, float v) { rows[f + (f / R) * (S - R)] = v; };
  uint32_t done = 0;
  if (VEC) {
    const uint32_t nv = nfl >> 2;
    for (uint32_t q0 = t; q0 < nv; q0 += SH_BATCH * SH_WG) {
      float4 v[SH_BATCH];
#pragma unroll
      for (int j = 0; j < SH_BATCH; ++j)
        if (q0 + j * SH_WG < nv) v[j] = reinterpret_cast<const float4*>(src)[q0 + j * SH_WG];
#pragma unroll
      for (int j = 0; j < SH_BATCH; ++j) {
        const uint32_t q = q0 + j * SH_WG;
        if (q < nv) {
          put(4 * q, v[j].x);
          put(4 * q + 1, v[j].y);
          put(4 * q + 2, v[j].z);
          put(4 * q + 3, v[j].w);
        }
      }
    }
    done = nv << 2;  // (at most 3 floats are left)
  }
  for (uint32_t f0 = done + t; f0 < nfl; f0 += SH_BATCH * SH_WG) {
    float v[SH_BATCH];
#pragma unroll
    for (int j = 0; j < SH_BATCH; ++j)
      if (f0 + j * SH_WG < nfl) v[j] = src[f0 + j * SH_WG];
#pragma unroll
    for (int j = 0; j < SH_BATCH; ++j)
      if (f0 + j * SH_WG < nfl) put(f0 + j * SH_WG, v[j]);
  }
}

// The way back: the block's nfl floats from the LDS rows to dst, lane-contiguous float4 stores plus a dword
// tail when VEC (dst 16-B aligned), dword stores otherwise. Nothing at or past dst + nfl is written.
template <uint32_t R, uint32_t S, bool VEC>
__device__ __forceinline__ void sh_stage_out(const float* rows, float* __restrict__ dst, uint32_t nfl, uint32_t t) {
  auto get = [&](uint32_t f) { return rows[f + (f / R) * (S - R)]; };
  uint32_t done = 0;
  if (VEC) {
    const uint32_t nv = nfl >> 2;
    for (uint32_t q = t; q < nv; q += SH_WG)
      reinterpret_cast<float4*>(dst)[q] = make_float4(get(4 * q), get(4 * q + 1), get(4 * q + 2), get(4 * q + 3));
    done = nv << 2;
  }
  for (uint32_t f = done + t; f < nfl; f += SH_WG) dst[f] = get(f);
}

// One workgroup: Gaussians [256 b, 256 b + 256) ∩ [0, count). VEC: sh is 16-B aligned (a block starts
// 256 rows = a multiple of 16 B after it), so the block is loaded as float4 plus a dword tail.
template <int DEG, bool VEC>
__global__ __launch_bounds__(SH_WG) void gs_sh_colors_kernel(const float* __restrict__ means,
                                                            const float* __restrict__ sh, uint32_t count,
                                                            uint32_t active, v3 cam, float* __restrict__ colors) {
  constexpr uint32_t R = sh_row(DEG);  // floats per row
  constexpr uint32_t S = R | 1u;       // LDS row stride
  const uint32_t first = blockIdx.x * (uint32_t)SH_WG, t = threadIdx.x;
  const uint32_t left = count - first, nrows = left < (uint32_t)SH_WG ? left : (uint32_t)SH_WG;
  const float* src = sh + (size_t)first * R;
#if defined(PTGS_SH_ROWWISE)
  const float* row = src + (size_t)t * R;
#else
  __shared__ float rows[DEG == 0 ? 1 : SH_WG * S];
  const float* row = DEG == 0 ? src + (size_t)t * R : rows + t * S;
  if (DEG > 0) {
    sh_stage_in<R, S, VEC>(rows, src, nrows * R, t);
    __syncthreads();
  }
#endif
  if (t >= nrows) return;
  const size_t i3 = (size_t)(first + t) * 3;
  float len;
  const v3 dir = sh_dir(means + i3, cam, &len);
  float rgb[3];
  sh_eval<DEG>(row, active, dir, rgb);
  colors[i3] = rgb[0];
  colors[i3 + 1] = rgb[1];
  colors[i3 + 2] = rgb[2];
}

__global__ __launch_bounds__(256) void gs_activate_kernel(const float* log_scales, const float* logits, uint32_t count,
                                                         float* scales, float* opacities) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)count * 3) scales[i] = expx(log_scales[i]);
  if (i < count) opacities[i] = 1.0f / (1.0f + expx(-logits[i]));
}

// The backward of gs_sh_colors_kernel, one workgroup per the same 256 rows: the block of coefficients comes in
// through LDS as there, each work-item overwrites its own LDS row with its row of dL/d(sh) (sh_backward_one
// reads the row completely first), and the block goes out with lane-contiguous stores. VIN / VOUT: sh / dsh
// are 16-B aligned. dmeans: NULL (the direction part is skipped), or dL/d(mean) is added to it, each Gaussian
// by its own work-item: no atomics.
// EYE (ptgs_gaussians_sh_colors_backward_eye): the workgroup also leaves the sum of what its Gaussians add to
// dL/d(mean) (formed with dmeans NULL too) in eye_partials[3 blockIdx.x ..]: over the wave in DPP, over the four
// waves through LDS, three plain stores; gs_sh_eye_finish_kernel adds the rows and negates. The EYE = false
// instantiations are the kernels as they were.
template <int DEG, bool VIN, bool VOUT, bool EYE>
__global__ __launch_bounds__(SH_WG) void gs_sh_colors_backward_kernel(const float* __restrict__ means,
                                                                     const float* __restrict__ sh, uint32_t count,
                                                                     uint32_t active, v3 cam,
                                                                     const float* __restrict__ dcolors,
                                                                     float* __restrict__ dsh, float* dmeans,
                                                                     float* __restrict__ eye_partials) {
  constexpr uint32_t R = sh_row(DEG);  // floats per row
  constexpr uint32_t S = R | 1u;       // LDS row stride
  const uint32_t first = blockIdx.x * (uint32_t)SH_WG, t = threadIdx.x;
  const uint32_t left = count - first, nrows = left < (uint32_t)SH_WG ? left : (uint32_t)SH_WG;
  const float* src = sh + (size_t)first * R;
  float* dst = dsh + (size_t)first * R;
#if defined(PTGS_SH_ROWWISE)
  const float* row = src + (size_t)t * R;
  float* drow = dst + (size_t)t * R;
#else
  __shared__ float rows[DEG == 0 ? 1 : SH_WG * S];
  const float* row = DEG == 0 ? src + (size_t)t * R : rows + t * S;
  float* drow = DEG == 0 ? dst + (size_t)t * R : rows + t * S;
  if (DEG > 0) {
    sh_stage_in<R, S, VIN>(rows, src, nrows * R, t);
    __syncthreads();
  }
#endif
  float dm[3] = {0.0f, 0.0f, 0.0f};  // (EYE) what this Gaussian adds to dL/d(mean)
  if (t < nrows) {
    const size_t i3 = (size_t)(first + t) * 3;
    float len = 0.0f;
    v3 dir = mk3(0.0f);
    if (DEG > 0 && active > 0) dir = sh_dir(means + i3, cam, &len);  // (the DC band does not see the direction)
    const float dcol[3] = {dcolors[i3], dcolors[i3 + 1], dcolors[i3 + 2]};
    sh_backward_one<DEG>(row, active, dir, len, dcol, drow, dmeans ? dmeans + i3 : nullptr, EYE ? dm : nullptr);
  }
#if !defined(PTGS_SH_ROWWISE)
  if (DEG > 0) {
    __syncthreads();
    sh_stage_out<R, S, VOUT>(rows, dst, nrows * R, t);
  }
#endif
  if (EYE) {  // (every work-item of the workgroup is here; those past nrows add zeros)
    __shared__ float s_eye[SH_WG / 64][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float s = gb_wave_sum(dm[k]);
      if ((t & 63u) == 63u) s_eye[t >> 6][k] = s;
    }
    __syncthreads();
    if (t < 3) eye_partials[(size_t)blockIdx.x * 3 + t] = (s_eye[0][t] + s_eye[1][t]) + (s_eye[2][t] + s_eye[3][t]);
  }
}

// The second stage of dL/d(camera_pos): one workgroup adds the `rows` partial rows of this call in float64, in a
// fixed order (splat_partial_sum.h); the eye moves against the means, hence the sign.
__global__ __launch_bounds__(GS_PSUM_BLOCK_EYE) void gs_sh_eye_finish_kernel(const float* __restrict__ partials,
                                                                              uint32_t rows,
                                                                              float* __restrict__ deye) {
  __shared__ double s_seg[3 * GS_PSUM_BLOCK_EYE];
  const double sum = gs_sum_partial_rows<3, GS_PSUM_BLOCK_EYE>(partials, rows, s_seg);
  if (threadIdx.x < 3) deye[threadIdx.x] = (float)(-sum);
}

// no __restrict__: an output may be its upstream gradient (in place)
__global__ __launch_bounds__(256) void gs_activate_backward_kernel(const float* scales, const float* opacities,
                                                                  uint32_t count, const float* dscales,
                                                                  const float* dopacities, float* dlog_scales,
                                                                  float* dlogits) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)count * 3) dlog_scales[i] = sh_dlog_scale(dscales[i], scales[i]);
  if (i < count) dlogits[i] = sh_dlogit(dopacities[i], opacities[i]);
}

// one work-item per output float: contiguous writes, reads contiguous within a row
__global__ __launch_bounds__(256) void gs_permute_sh_kernel(const float* __restrict__ sh, uint32_t R,
                                                           const uint32_t* __restrict__ ids, uint32_t count,
                                                           float* __restrict__ out) {
  const size_t f = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t)count * R) return;
  const uint32_t i = (uint32_t)(f / R), col = (uint32_t)(f - (size_t)i * R);
  const uint32_t id = ids[i];
  out[f] = id < count ? sh[(size_t)id * R + col] : 0.0f;
}

template <int DEG>
hipError_t launch_sh(const float* means, const float* sh, uint32_t count, uint32_t active, v3 cam, float* colors,
                     hipStream_t s) {
  const uint32_t blocks = (uint32_t)(((uint64_t)count + SH_WG - 1) / SH_WG);
  if constexpr (DEG > 0) {  // (degree 0 stages nothing)
    if (((uintptr_t)sh & 15u) == 0) {
      gs_sh_colors_kernel<DEG, true><<<blocks, SH_WG, 0, s>>>(means, sh, count, active, cam, colors);
      return hipGetLastError();
    }
  }
  gs_sh_colors_kernel<DEG, false><<<blocks, SH_WG, 0, s>>>(means, sh, count, active, cam, colors);
  return hipGetLastError();
}

template <int DEG, bool EYE>
hipError_t launch_sh_backward(const float* means, const float* sh, uint32_t count, uint32_t active, v3 cam,
                              const float* dcolors, float* dsh, float* dmeans, float* eye_partials, hipStream_t s) {
  const uint32_t blocks = (uint32_t)(((uint64_t)count + SH_WG - 1) / SH_WG);
#define PTGS_SH_BWD(VIN, VOUT)                                                                                  \
  gs_sh_colors_backward_kernel<DEG, VIN, VOUT, EYE><<<blocks, SH_WG, 0, s>>>(means, sh, count, active, cam, dcolors, \
                                                                             dsh, dmeans, eye_partials)
  const bool vin = ((uintptr_t)sh & 15u) == 0, vout = ((uintptr_t)dsh & 15u) == 0;
  if constexpr (DEG == 0) {  // (degree 0 stages nothing)
    PTGS_SH_BWD(false, false);
  } else if (vin && vout) {
    PTGS_SH_BWD(true, true);
  } else if (vin) {
    PTGS_SH_BWD(true, false);
  } else if (vout) {
    PTGS_SH_BWD(false, true);
  } else {
    PTGS_SH_BWD(false, false);
  }
#undef PTGS_SH_BWD
  return hipGetLastError();
}

}  // namespace

hipError_t splat_sh_colors(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                           uint32_t active_degree, const float cam[3], float* colors, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const v3 c = mk3(cam[0], cam[1], cam[2]);
  switch (sh_degree) {
    case 0: return launch_sh<0>(means, sh, count, active_degree, c, colors, s);
    case 1: return launch_sh<1>(means, sh, count, active_degree, c, colors, s);
    case 2: return launch_sh<2>(means, sh, count, active_degree, c, colors, s);
    case 3: return launch_sh<3>(means, sh, count, active_degree, c, colors, s);
  }
  return hipErrorInvalidValue;
}

hipError_t splat_sh_colors_backward(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                                    uint32_t active_degree, const float cam[3], const float* dcolors, float* dsh,
                                    float* dmeans, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const v3 c = mk3(cam[0], cam[1], cam[2]);
  if (sh_degree == 0 || active_degree == 0) dmeans = nullptr;  // no direction part: neither read nor written
  switch (sh_degree) {
    case 0: return launch_sh_backward<0, false>(means, sh, count, active_degree, c, dcolors, dsh, dmeans, nullptr, s);
    case 1: return launch_sh_backward<1, false>(means, sh, count, active_degree, c, dcolors, dsh, dmeans, nullptr, s);
    case 2: return launch_sh_backward<2, false>(means, sh, count, active_degree, c, dcolors, dsh, dmeans, nullptr, s);
    case 3: return launch_sh_backward<3, false>(means, sh, count, active_degree, c, dcolors, dsh, dmeans, nullptr, s);
  }
  return hipErrorInvalidValue;
}

hipError_t splat_sh_colors_backward_eye(const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                                        uint32_t active_degree, const float cam[3], const float* dcolors, float* dsh,
                                        float* dmeans, float* eye_partials, float* deye, hipStream_t s) {
  if (sh_degree > 3) return hipErrorInvalidValue;
  if (count == 0 || sh_degree == 0 || active_degree == 0) {  // no direction part: the eye gets exact zeros
    const hipError_t e = hipMemsetAsync(deye, 0, 3 * sizeof(float), s);
    return e ? e : splat_sh_colors_backward(means, sh, count, sh_degree, active_degree, cam, dcolors, dsh, dmeans, s);
  }
  const v3 c = mk3(cam[0], cam[1], cam[2]);
  const uint32_t act = active_degree;
  hipError_t e = hipErrorInvalidValue;
  if (sh_degree == 1) e = launch_sh_backward<1, true>(means, sh, count, act, c, dcolors, dsh, dmeans, eye_partials, s);
  if (sh_degree == 2) e = launch_sh_backward<2, true>(means, sh, count, act, c, dcolors, dsh, dmeans, eye_partials, s);
  if (sh_degree == 3) e = launch_sh_backward<3, true>(means, sh, count, act, c, dcolors, dsh, dmeans, eye_partials, s);
  if (e) return e;
  // every row the finish reads was written by the launch above
  gs_sh_eye_finish_kernel<<<1, GS_PSUM_BLOCK_EYE, 0, s>>>(eye_partials, splat_sh_eye_rows(count), deye);
  return hipGetLastError();
}

hipError_t splat_sh_activate(const float* log_scales, const float* logits, uint32_t count, float* scales,
                             float* opacities, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const uint32_t blocks = (uint32_t)(((uint64_t)count * 3 + 255) / 256);
  gs_activate_kernel<<<blocks, 256, 0, s>>>(log_scales, logits, count, scales, opacities);
  return hipGetLastError();
}

hipError_t splat_sh_activate_backward(const float* scales, const float* opacities, uint32_t count,
                                      const float* dscales, const float* dopacities, float* dlog_scales,
                                      float* dlogits, hipStream_t s) {
  if (count == 0) return hipSuccess;
  const uint32_t blocks = (uint32_t)(((uint64_t)count * 3 + 255) / 256);
  gs_activate_backward_kernel<<<blocks, 256, 0, s>>>(scales, opacities, count, dscales, dopacities, dlog_scales,
                                                     dlogits);
  return hipGetLastError();
}

hipError_t splat_sh_permute(const float* sh, uint32_t sh_degree, const uint32_t* ids, uint32_t count, float* out,
                            hipStream_t s) {
  if (count == 0) return hipSuccess;
  const uint32_t R = (uint32_t)sh_row((int)sh_degree);
  const uint64_t blocks = ((uint64_t)count * R + 255) / 256;
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  gs_permute_sh_kernel<<<(uint32_t)blocks, 256, 0, s>>>(sh, R, ids, count, out);
  return hipGetLastError();
}

}  // namespace ptgs
