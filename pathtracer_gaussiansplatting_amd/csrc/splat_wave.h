// splat_wave.h — wave64 and workgroup primitives with no splatting in them: DPP scan / reduce, lane
// exchanges without LDS, the 64-key register sort of a wave, the workgroup's bitonic network. Used by the
// binning, fused, radix sort, spill and blend stages; relies on no other header of the rasterizer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ptgs {

// Inclusive wave64 prefix sum in DPP (row_shr 1/2/4/8 inside rows of 16, then row_bcast 15 / 31
// across rows): six VALU adds instead of six ds_bpermute round trips.
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t x) {
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true);  // row_shr:1
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true);  // row_shr:2
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true);  // row_shr:4
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true);  // row_shr:8
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
  x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
  return x;
}

// Wave64 min / max / sum in DPP (the scan pattern of wave_incl_scan: lane 63 ends with the reduction of
// all 64) and broadcast from lane 63: six VALU steps with no LDS round trip, where the __shfl_xor
// butterfly is six dependent ds_bpermute round trips.
template <int OP>  // 0 min, 1 max, 2 sum
__device__ __forceinline__ uint32_t wave_reduce(uint32_t x) {
  const int id = OP == 0 ? -1 : 0;  // (0xFFFFFFFF: the identity of an unsigned min)
  auto f = [](uint32_t a, uint32_t b) { return OP == 0 ? min(a, b) : OP == 1 ? max(a, b) : a + b; };
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x111, 0xF, 0xF, false));  // row_shr:1
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x112, 0xF, 0xF, false));  // row_shr:2
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x114, 0xF, 0xF, false));  // row_shr:4
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x118, 0xF, 0xF, false));  // row_shr:8
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x142, 0xA, 0xF, false));  // row_bcast:15
  x = f(x, (uint32_t)__builtin_amdgcn_update_dpp(id, (int)x, 0x143, 0xC, 0xF, false));  // row_bcast:31
  return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

// x of lane ^ J without LDS: DPP inside rows of 16 (quad_perm for 1 / 2; half-row / row mirrors composed
// with them for 4 / 8) and the gfx950 permlane swaps across rows (16) and halves (32)
template <uint32_t J>
__device__ __forceinline__ uint32_t lane_xor(uint32_t x, uint32_t lane) {
  if (J == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, false);  // quad_perm 1,0,3,2
  if (J == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, false);  // quad_perm 2,3,0,1
  if (J == 4) {  // (i ^ 7) ^ 3
    const int t = __builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, false);  // row_half_mirror
    return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x1B, 0xF, 0xF, false);     // quad_perm 3,2,1,0
  }
  if (J == 8) {  // (i ^ 15) ^ 7
    const int t = __builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, false);  // row_mirror
    return (uint32_t)__builtin_amdgcn_update_dpp(0, t, 0x141, 0xF, 0xF, false);    // row_half_mirror
  }
  if (J == 16) {  // odd rows of the first result, even rows of the second (the rows as a constant lane mask)
    const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false);
    return __builtin_amdgcn_inverse_ballot_w64(0xFFFF0000FFFF0000ull) ? r[0] : r[1];
  }
  const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);  // J == 32
  return __builtin_amdgcn_inverse_ballot_w64(0xFFFFFFFF00000000ull) ? r[0] : r[1];
}
template <uint32_t J>
__device__ __forceinline__ unsigned long long lane_xor64(unsigned long long x, uint32_t lane) {
  return ((unsigned long long)lane_xor<J>((uint32_t)(x >> 32), lane) << 32) | lane_xor<J>((uint32_t)x, lane);
}

// ascending bitonic sort ("flip" network: every comparator puts the min at the lower index) over
// n elements; indices >= n act as +inf and are never touched, so n need not be a power of two.
template <typename Swap>
__device__ __forceinline__ void bitonic_flip_sort(uint32_t n, Swap swap_if) {
  uint32_t npad = 1;
  while (npad < n) npad <<= 1;
  const uint32_t half = npad >> 1;
  for (uint32_t lk = 1; (1u << lk) <= npad; ++lk) {  // k = 2^lk; all strides are powers of two
    const uint32_t k = 1u << lk, lhk = lk - 1;
    for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
      uint32_t blk = i >> lhk, off = i & ((1u << lhk) - 1u);
      uint32_t a = blk * k + off, b = blk * k + k - 1 - off;
      if (b < n) swap_if(a, b);
    }
    __syncthreads();
    for (int lj = (int)lk - 2; lj >= 0; --lj) {
      const uint32_t j = 1u << lj;
      for (uint32_t i = threadIdx.x; i < half; i += blockDim.x) {
        uint32_t a = ((i >> lj) << (lj + 1)) + (i & (j - 1u)), b = a + j;
        if (b < n) swap_if(a, b);
      }
      __syncthreads();
    }
  }
}

// The 64-key register sort of a wave (the blend's merge ranking, splat_blend.h).
// (the exchanges through DPP and the gfx950 permlane swaps: no LDS round trip per step)
// the lanes of a bitonic step (K, J) that keep the smaller key: ascending blocks' low halves and descending
// blocks' high halves (a compile-time lane mask)
template <uint32_t K, uint32_t J>
__host__ __device__ constexpr unsigned long long gs_keep_min_mask() {
  unsigned long long m = 0;
  for (uint32_t l = 0; l < 64u; ++l)
    if (((l & K) == 0u) == ((l & J) == 0u)) m |= 1ull << l;
  return m;
}
// one compare-exchange step: a lane takes its partner's key iff (partner < own) equals "keeps the
// minimum" — one 64-bit compare, the lane mask applied to its result in SGPRs, two selects (the min / max
// form compared twice and selected three times: 21 steps x ~6 VALU more per wave sort, ~0.7 M VALU per
// C2 frame)
template <uint32_t K, uint32_t J>
__device__ __forceinline__ unsigned long long gs_sort_step(unsigned long long x, uint32_t lane) {
  const unsigned long long y = lane_xor64<J>(x, lane);
  const unsigned long long take = ~(__builtin_amdgcn_ballot_w64(y < x) ^ gs_keep_min_mask<K, J>());
  return __builtin_amdgcn_inverse_ballot_w64(take) ? y : x;
}
__device__ __forceinline__ unsigned long long gs_wave_sort64(unsigned long long x, uint32_t lane) {
  x = gs_sort_step<2, 1>(x, lane);
  x = gs_sort_step<4, 2>(x, lane); x = gs_sort_step<4, 1>(x, lane);
  x = gs_sort_step<8, 4>(x, lane); x = gs_sort_step<8, 2>(x, lane); x = gs_sort_step<8, 1>(x, lane);
  x = gs_sort_step<16, 8>(x, lane); x = gs_sort_step<16, 4>(x, lane); x = gs_sort_step<16, 2>(x, lane);
  x = gs_sort_step<16, 1>(x, lane);
  x = gs_sort_step<32, 16>(x, lane); x = gs_sort_step<32, 8>(x, lane); x = gs_sort_step<32, 4>(x, lane);
  x = gs_sort_step<32, 2>(x, lane); x = gs_sort_step<32, 1>(x, lane);
  x = gs_sort_step<64, 32>(x, lane); x = gs_sort_step<64, 16>(x, lane); x = gs_sort_step<64, 8>(x, lane);
  x = gs_sort_step<64, 4>(x, lane); x = gs_sort_step<64, 2>(x, lane); x = gs_sort_step<64, 1>(x, lane);
  return x;
}

}  // namespace ptgs
