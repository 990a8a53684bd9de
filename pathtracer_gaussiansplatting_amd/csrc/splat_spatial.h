// splat_spatial.h — scene preparation, not part of a frame: the spatial (Morton) order of a Gaussian set
// (ptgs_gaussians_sort_spatial) and the per-chunk bounds (ptgs_gaussians_chunk_bounds), kernels and host
// functions. Relies on gs_chunks256 (splat_plan.h) and the declarations of splat.h.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>

#include "../../include/ptgs/ptgs.h"
#include "splat.h"
#include "splat_plan.h"

namespace ptgs {

// ---- spatial order (ptgs_gaussians_sort_spatial) ---------------------------------------------------
__device__ __forceinline__ uint32_t gs_f2ord(float f) {  // order-preserving float -> uint
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gs_ord2f(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }
__device__ __forceinline__ uint32_t gs_spread3(uint32_t v) {  // 10 bits -> every 3rd bit
  v = (v * 0x00010001u) & 0xFF0000FFu;
  v = (v * 0x00000101u) & 0x0F00F00Fu;
  v = (v * 0x00000011u) & 0xC30C30C3u;
  v = (v * 0x00000005u) & 0x49249249u;
  return v;
}

__global__ __launch_bounds__(256) void gs_means_bounds_kernel(const float* __restrict__ means, uint32_t n,
                                                              uint32_t* __restrict__ b) {  // b: lo[3], hi[3]
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n)
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = means[3 * i + a];
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; ++a) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], off));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off));
    }
  if ((threadIdx.x & 63u) == 0)
    for (int a = 0; a < 3; ++a) {
      atomicMin(b + a, gs_f2ord(lo[a]));
      atomicMax(b + 3 + a, gs_f2ord(hi[a]));
    }
}

__global__ __launch_bounds__(256) void gs_means_morton_kernel(const float* __restrict__ means, uint32_t n,
                                                              const uint32_t* __restrict__ b,
                                                              unsigned long long* __restrict__ keys) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t q[3];
  for (int a = 0; a < 3; ++a) {
    const float lo = gs_ord2f(b[a]), ext = gs_ord2f(b[3 + a]) - lo;
    const float u = ext > 0.0f ? (means[3 * i + a] - lo) / ext : 0.0f;
    q[a] = (uint32_t)fminf(fmaxf(u * 1024.0f, 0.0f), 1023.0f);
  }
  const uint32_t code = (gs_spread3(q[0]) << 2) | (gs_spread3(q[1]) << 1) | gs_spread3(q[2]);
  keys[i] = ((unsigned long long)code << 32) | i;
}

__global__ __launch_bounds__(256) void gs_gather_sorted_kernel(const unsigned long long* __restrict__ keys, uint32_t n,
                                                               ptgs_gaussians g, float* __restrict__ means,
                                                               float* __restrict__ scales, float* __restrict__ rots,
                                                               float* __restrict__ opac, float* __restrict__ colors,
                                                               uint32_t* __restrict__ ids) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint32_t j = (uint32_t)keys[i];
  for (int a = 0; a < 3; ++a) {
    means[3 * i + a] = g.means[3 * j + a];
    scales[3 * i + a] = g.scales[3 * j + a];
    colors[3 * i + a] = g.colors[3 * j + a];
  }
  for (int a = 0; a < 4; ++a) rots[4 * i + a] = g.rotations[4 * j + a];
  opac[i] = g.opacities[j];
  ids[i] = g.ids ? g.ids[j] : j;
}

hipError_t splat_sort_spatial(const ptgs_gaussians* g, float* means, float* scales, float* rots, float* opac,
                              float* colors, uint32_t* ids, hipStream_t s) {
  const uint32_t n = g->count;
  if (n == 0) return hipSuccess;
  hipError_t e;
  uint32_t* b = nullptr;
  unsigned long long *k0 = nullptr, *k1 = nullptr;
  void* tmp = nullptr;
  size_t tmp_bytes = 0;
  const uint32_t init[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u, 0u};
  const dim3 grid((n + 255) / 256);
  auto done = [&](hipError_t r) {
    (void)hipStreamSynchronize(s);
    if (b) (void)hipFree(b);
    if (k0) (void)hipFree(k0);
    if (k1) (void)hipFree(k1);
    if (tmp) (void)hipFree(tmp);
    return r;
  };
  if ((e = hipMalloc(&b, 32)) || (e = hipMalloc(&k0, (size_t)n * 8)) || (e = hipMalloc(&k1, (size_t)n * 8))) return done(e);
  if ((e = hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, k0, k1, (int)n, 0, 62, s))) return done(e);
  if ((e = hipMalloc(&tmp, tmp_bytes))) return done(e);
  if ((e = hipMemcpyAsync(b, init, sizeof(init), hipMemcpyHostToDevice, s))) return done(e);
  hipLaunchKernelGGL(gs_means_bounds_kernel, grid, dim3(256), 0, s, g->means, n, b);
  hipLaunchKernelGGL(gs_means_morton_kernel, grid, dim3(256), 0, s, g->means, n, (const uint32_t*)b, k0);
  if ((e = hipGetLastError())) return done(e);
  if ((e = hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, k0, k1, (int)n, 0, 62, s))) return done(e);
  hipLaunchKernelGGL(gs_gather_sorted_kernel, grid, dim3(256), 0, s, (const unsigned long long*)k1, n, *g, means, scales,
                     rots, opac, colors, ids);
  return done(hipGetLastError());
}

// ---- chunk bounds (ptgs_gaussians_chunk_bounds) -----------------------------------------------------
// chunk c = Gaussians [256 c, 256 c + 256): (min x, min y, min z, max |scale|), (max x, max y, max z, 0)
__global__ __launch_bounds__(256) void gs_chunk_bounds_kernel(const float* __restrict__ means,
                                                              const float* __restrict__ scales, uint32_t n,
                                                              float4* __restrict__ out) {
  __shared__ float s_b[7][4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  float b[7] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY, 0.0f};
  if (i < n) {
    for (int a = 0; a < 3; ++a) b[a] = b[3 + a] = means[3 * i + a];
    b[6] = fmaxf(fabsf(scales[3 * i]), fmaxf(fabsf(scales[3 * i + 1]), fabsf(scales[3 * i + 2])));
  }
  for (int off = 32; off > 0; off >>= 1)
    for (int a = 0; a < 3; ++a) {
      b[a] = fminf(b[a], __shfl_xor(b[a], off));
      b[3 + a] = fmaxf(b[3 + a], __shfl_xor(b[3 + a], off));
    }
  for (int off = 32; off > 0; off >>= 1) b[6] = fmaxf(b[6], __shfl_xor(b[6], off));
  if ((threadIdx.x & 63u) == 0)
    for (int a = 0; a < 7; ++a) s_b[a][threadIdx.x >> 6] = b[a];
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      for (int a = 0; a < 3; ++a) {
        b[a] = fminf(b[a], s_b[a][w]);
        b[3 + a] = fmaxf(b[3 + a], s_b[3 + a][w]);
      }
      b[6] = fmaxf(b[6], s_b[6][w]);
    }
    out[2 * blockIdx.x] = make_float4(b[0], b[1], b[2], b[6]);
    out[2 * blockIdx.x + 1] = make_float4(b[3], b[4], b[5], 0.0f);
  }
}

hipError_t splat_chunk_bounds(const ptgs_gaussians* g, float* bounds, hipStream_t s) {
  if (g->count == 0) return hipSuccess;
  hipLaunchKernelGGL(gs_chunk_bounds_kernel, dim3(gs_chunks256(g->count)), dim3(256), 0, s, g->means, g->scales,
                     g->count, (float4*)bounds);
  return hipGetLastError();
}

}  // namespace ptgs
