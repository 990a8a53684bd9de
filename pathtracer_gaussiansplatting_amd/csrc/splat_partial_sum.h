// splat_partial_sum.h — the second stage of a two-stage sum over Gaussians (the camera gradients of
// splat_backward.hip and splat_sh.hip). The first stage leaves one row of K floats per workgroup, written with
// plain vector stores; gs_sum_partial_rows adds the rows in ONE workgroup of BLOCK work-items, in float64 and in a
// fixed order: work-item t adds the rows t, t + BLOCK, t + 2 BLOCK, ... in index order (consecutive work-items read
// consecutive rows, and the loads of GS_PSUM_BATCH rows are issued before their adds: a work-item that waited for
// each row in turn took 0.5 us per row, 30 us over the 15 625 rows of 4M Gaussians), then the BLOCK sums are added
// by a halving tree. No atomics: two runs give the same bits. The launch boundary between the stages is the
// grid-wide barrier; there is nothing to overlap with it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptgs {

#define GS_PSUM_BLOCK 256  // the pose finish (12 columns: 24 KiB of LDS)
#define GS_PSUM_BLOCK_EYE 1024  // the eye finish (3 columns: 24 KiB), 1M Gaussians and more per call

// Wave64 float sum in DPP (row_shr 1/2/4/8 inside rows of 16, then row_bcast 15 / 31): lane 63 ends with
// the sum of all 64, returned wave-uniform. Every lane of the wave must be active.
__device__ __forceinline__ float gb_wave_sum(float v) {
  auto step = [](float x, int y) { return x + __int_as_float(y); };
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x111, 0xF, 0xF, false));  // row_shr:1
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x112, 0xF, 0xF, false));  // row_shr:2
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x114, 0xF, 0xF, false));  // row_shr:4
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x118, 0xF, 0xF, false));  // row_shr:8
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false));  // row_bcast:15
  v = step(v, __builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, false));  // row_bcast:31
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

#define GS_PSUM_BATCH 4

// s_seg: K * BLOCK doubles of LDS; BLOCK: the workgroup's size, a power of two. Every work-item of the workgroup
// calls it; work-item k < K returns the sum of column k (the others return 0).
template <uint32_t K, uint32_t BLOCK>
__device__ __forceinline__ double gs_sum_partial_rows(const float* __restrict__ partials, uint32_t rows,
                                                      double* s_seg) {
  static_assert((BLOCK & (BLOCK - 1u)) == 0 && K <= BLOCK, "a halving tree over the work-items' sums");
  const uint32_t t = threadIdx.x;
  double acc[K];
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) acc[k] = 0.0;
  for (uint32_t r0 = t; r0 < rows; r0 += GS_PSUM_BATCH * BLOCK) {
    float v[GS_PSUM_BATCH][K];
#pragma unroll
    for (uint32_t j = 0; j < GS_PSUM_BATCH; ++j) {
      const uint32_t r = r0 + j * BLOCK;
#pragma unroll
      for (uint32_t k = 0; k < K; ++k) v[j][k] = r < rows ? partials[(size_t)r * K + k] : 0.0f;  // (+ 0: exact)
    }
#pragma unroll
    for (uint32_t j = 0; j < GS_PSUM_BATCH; ++j) {
#pragma unroll
      for (uint32_t k = 0; k < K; ++k) acc[k] += (double)v[j][k];
    }
  }
#pragma unroll
  for (uint32_t k = 0; k < K; ++k) s_seg[k * BLOCK + t] = acc[k];
  __syncthreads();
  for (uint32_t half = BLOCK / 2u; half > 0u; half >>= 1) {
    if (t < half) {
#pragma unroll
      for (uint32_t k = 0; k < K; ++k) s_seg[k * BLOCK + t] += s_seg[k * BLOCK + t + half];
    }
    __syncthreads();
  }
  return t < K ? s_seg[t * BLOCK] : 0.0;
}

}  // namespace ptgs
