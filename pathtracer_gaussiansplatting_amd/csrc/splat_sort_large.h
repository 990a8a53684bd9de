// splat_sort_large.h — stage: the radix sort of the tiles above GS_MID pairs, before the blend. Relies on
// GsFused (splat_fused.h), the counter words (splat_words.h), the wave scan and the bitonic network
// (splat_wave.h) and GS_SORT_THREADS / GS_RADIX_MAXR (splat_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "splat_fused.h"
#include "splat_plan.h"
#include "splat_probe.h"
#include "splat_wave.h"
#include "splat_words.h"

namespace ptgs {

// ---- large tiles: radix sort ----------------------------------------------------------------------
// Tiles of more than GS_MID pairs are listed by the colscan and sorted here, before the blend, by
// 256-work-item workgroups striding over the list:
//  load     the segment's depths (u32) and positions (u16) into LDS (tiles of up to 256 * rmax
//           pairs; rmax follows the previous frame's largest tile) or, above that, into a global
//           scratch at the tile's pair offset (10M Gaussians at 4K: ~28k-pair tiles, L2-resident)
//  passes   stable LSD radix sort on the depth minus the tile's minimum, 4-bit digits over the bits
//           of the depth range (C2's 4..12 depths: 24 bits, 6 passes); work-item t owns positions
//           [t R, t R + R) (R odd: bank-conflict free in LDS): per-digit counts in packed byte
//           registers, a (digit, work-item) scan of the 16 x 256 u16 counters in LDS, then each item
//           goes to (its digit's scanned base) + (earlier items of that digit in the work-item)
//  ties     equal depths are put in gaussian order (odd-even transposition inside equal-depth runs;
//           rare: the order of a stable global sort of (tile, depth) keys over gaussian indices)
//  publish  keys_out = tile << 32 | depth, vals_out = gaussian (the blend streams these)
// A 16-byte-per-comparator LDS bitonic network measured ~5 MB of LDS traffic per 2.6k-pair tile
// (LDS-bandwidth bound: ~130 us of the 1M-Gaussian frame); the radix moves ~0.2 MB.
// (GS_SORT_THREADS, GS_RADIX_MAXR: splat_plan.h)
#define GS_RADIX_MAXN 65535u  // u16 positions: global bitonic above (never met by the configs)

__host__ __device__ constexpr size_t gs_radix_lds(uint32_t rmax) {
  return (size_t)GS_SORT_THREADS * rmax * 12u + 16u * GS_SORT_THREADS * 2u;
}

// Sort positions [0, n) of (dep[0], slot[0]) (dep[1] / slot[1]: the other half of the ping-pong) by
// depth; returns the half that holds the result. DEP / SLOT are LDS or global arrays (inlined per
// call site, so the address spaces are known); s_cnt and s_red are LDS.
__device__ __forceinline__ uint32_t gs_radix_tile(uint32_t* dep0, uint32_t* dep1, uint16_t* slot0, uint16_t* slot1,
                                                  uint16_t* s_cnt, uint32_t (*s_red)[GS_SORT_THREADS / 64],
                                                  const uint32_t* segw, uint32_t n, uint32_t R) {
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t vmin = ~0u, vmax = 0u;
  for (uint32_t k0 = tid; k0 < n; k0 += 8 * GS_SORT_THREADS) {  // 8 loads in flight per work-item
    uint32_t d[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k0 + j * GS_SORT_THREADS;
      d[j] = k < n ? segw[2 * k + 1] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k0 + j * GS_SORT_THREADS;
      if (k < n) {
        vmin = min(vmin, d[j]);
        vmax = max(vmax, d[j]);
        dep0[k] = d[j];
        slot0[k] = (uint16_t)k;
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    vmin = min(vmin, (uint32_t)__shfl_xor((int)vmin, off));
    vmax = max(vmax, (uint32_t)__shfl_xor((int)vmax, off));
  }
  if (lane == 0) {
    s_red[0][wave] = vmin;
    s_red[1][wave] = vmax;
  }
  __syncthreads();
#pragma unroll
  for (int w = 0; w < GS_SORT_THREADS / 64; ++w) {
    vmin = min(vmin, s_red[0][w]);
    vmax = max(vmax, s_red[1][w]);
  }
  // depth bits of positive floats order like the floats: sort (d - min) over the bits of max - min
  vmin = (uint32_t)__builtin_amdgcn_readfirstlane((int)vmin);
  vmax = (uint32_t)__builtin_amdgcn_readfirstlane((int)vmax);
  const uint32_t nbits = vmax > vmin ? 32u - (uint32_t)__builtin_clz(vmax - vmin) : 0u;
  const uint32_t p0 = tid * R, p1 = min(n, p0 + R);  // this work-item's positions
  uint32_t cur = 0;
  for (uint32_t sh = 0; sh < nbits; sh += 4) {
    const uint32_t* sd = cur ? dep1 : dep0;
    const uint16_t* ss = cur ? slot1 : slot0;
    uint32_t* dd = cur ? dep0 : dep1;
    uint16_t* ds = cur ? slot0 : slot1;
    // counts: bytes of c0 (digits 0-7) and c1 (digits 8-15); R < 256
    unsigned long long c0 = 0, c1 = 0;
#pragma unroll 8
    for (uint32_t p = p0; p < p1; ++p) {
      const uint32_t d = ((sd[p] - vmin) >> sh) & 15u;
      const unsigned long long inc = 1ull << ((d & 7u) * 8u);
      c0 += d < 8u ? inc : 0ull;
      c1 += d < 8u ? 0ull : inc;
    }
#pragma unroll
    for (uint32_t d = 0; d < 8; ++d) {
      s_cnt[d * GS_SORT_THREADS + tid] = (uint16_t)((c0 >> (8u * d)) & 0xFFu);
      s_cnt[(d + 8) * GS_SORT_THREADS + tid] = (uint16_t)((c1 >> (8u * d)) & 0xFFu);
    }
    __syncthreads();
    // exclusive scan of the counters in (digit, work-item) order: work-item t holds entries [16t, 16t+16)
    uint4* cw = reinterpret_cast<uint4*>(s_cnt + 16u * tid);
    const uint4 a0 = cw[0], a1 = cw[1];
    uint32_t v[16] = {a0.x & 0xFFFFu, a0.x >> 16, a0.y & 0xFFFFu, a0.y >> 16, a0.z & 0xFFFFu, a0.z >> 16,
                      a0.w & 0xFFFFu, a0.w >> 16, a1.x & 0xFFFFu, a1.x >> 16, a1.y & 0xFFFFu, a1.y >> 16,
                      a1.z & 0xFFFFu, a1.z >> 16, a1.w & 0xFFFFu, a1.w >> 16};
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const uint32_t x = v[k];
      v[k] = sum;
      sum += x;
    }
    const uint32_t incl = wave_incl_scan(sum);
    if (lane == 63) s_red[0][wave] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (uint32_t w = 0; w < wave; ++w) base += s_red[0][w];
    cw[0] = make_uint4((v[0] + base) | ((v[1] + base) << 16), (v[2] + base) | ((v[3] + base) << 16),
                       (v[4] + base) | ((v[5] + base) << 16), (v[6] + base) | ((v[7] + base) << 16));
    cw[1] = make_uint4((v[8] + base) | ((v[9] + base) << 16), (v[10] + base) | ((v[11] + base) << 16),
                       (v[12] + base) | ((v[13] + base) << 16), (v[14] + base) | ((v[15] + base) << 16));
    __syncthreads();
    // scatter, stable inside the work-item (running byte counters) and across work-items (the scan);
    // batches of 8: a batch's loads issue before its stores (which the compiler may not reorder
    // across: every array can alias)
    c0 = 0;
    c1 = 0;
    for (uint32_t q0 = p0; q0 < p1; q0 += 8) {
      uint32_t dv[8], sv[8], dst[8];
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t p = min(q0 + j, p1 - 1);
        dv[j] = sd[p];
        sv[j] = ss[p];
      }
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t d = ((dv[j] - vmin) >> sh) & 15u;
        const uint32_t bit = (d & 7u) * 8u;
        const unsigned long long cc = d < 8u ? c0 : c1;
        const uint32_t local = (uint32_t)(cc >> bit) & 0xFFu;
        const bool ok = q0 + j < p1;
        c0 += (ok && d < 8u) ? (1ull << bit) : 0ull;
        c1 += (ok && d >= 8u) ? (1ull << bit) : 0ull;
        dst[j] = (uint32_t)s_cnt[d * GS_SORT_THREADS + tid] + local;
      }
#pragma unroll
      for (uint32_t j = 0; j < 8; ++j)
        if (q0 + j < p1) {
          dd[dst[j]] = dv[j];
          ds[dst[j]] = (uint16_t)sv[j];
        }
    }
    __syncthreads();
    cur ^= 1u;
  }
  return cur;
}

// ties (equal depths in gaussian order) and publish of one sorted tile
__device__ __forceinline__ void gs_radix_publish(const uint32_t* sd, uint16_t* ss, const uint32_t* segw, uint32_t n,
                                                 unsigned long long tbits, unsigned long long* keys_out,
                                                 uint32_t* vals_out) {
  const uint32_t tid = threadIdx.x;
  int tie = 0;
  for (uint32_t k = tid; k + 1 < n; k += GS_SORT_THREADS) tie |= sd[k] == sd[k + 1];
  if (__syncthreads_or(tie)) {
    int changed;
    do {
      changed = 0;
      for (uint32_t ph = 0; ph < 2; ++ph) {
        for (uint32_t k = 2 * tid + ph; k + 1 < n; k += 2 * GS_SORT_THREADS)
          if (sd[k] == sd[k + 1]) {
            const uint16_t x = ss[k], y = ss[k + 1];
            if (segw[2 * (uint32_t)y] < segw[2 * (uint32_t)x]) {
              ss[k] = y;
              ss[k + 1] = x;
              changed = 1;
            }
          }
        __syncthreads();
      }
    } while (__syncthreads_or(changed));
  }
  for (uint32_t k0 = tid; k0 < n; k0 += 8 * GS_SORT_THREADS) {  // 8 gathers in flight per work-item
    uint32_t g[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k0 + j * GS_SORT_THREADS;
      g[j] = k < n ? segw[2 * (uint32_t)ss[k]] : 0u;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint32_t k = k0 + j * GS_SORT_THREADS;
      if (k < n) {
        if (keys_out) keys_out[k] = tbits | sd[k];  // (keys: only for a published frame)
        vals_out[k] = g[j];
      }
    }
  }
}

__global__ __launch_bounds__(GS_SORT_THREADS) void gs_sort_large_kernel(
    const uint2* __restrict__ ranges, unsigned long long* __restrict__ pairs,
    const unsigned long long* __restrict__ tile_slots, const uint32_t* __restrict__ large,
    const uint32_t* __restrict__ large_ctr, unsigned long long* __restrict__ keys_out, uint32_t* __restrict__ vals_out,
    const uint32_t* __restrict__ total, uint32_t cap, uint32_t rmax, uint32_t* __restrict__ g_dep,
    uint16_t* __restrict__ g_slot, uint32_t g_cap, GsFused fu, uint32_t ntiles) {
  // LDS: one array per field, halves at offsets (an array of LDS pointers indexed at run time would
  // turn every access into a FLAT one)
  extern __shared__ __attribute__((aligned(16))) char s_arena[];
  const uint32_t capn = GS_SORT_THREADS * rmax;
  uint32_t* s_dep = reinterpret_cast<uint32_t*>(s_arena);           // [2][capn]
  uint16_t* s_slot = reinterpret_cast<uint16_t*>(s_dep + 2 * capn);  // [2][capn]
  uint16_t* s_cnt = s_slot + 2 * capn;                                // [16 digits][256 work-items]
  __shared__ uint32_t s_red[2][GS_SORT_THREADS / 64];
  __shared__ uint32_t s_list[GS_SORT_THREADS + 1];  // fused: this block's large tiles
  const uint32_t tid = threadIdx.x;
  uint32_t count;
  if (fu.scap) {
    // fused front end: no tile list; block b checks tiles b, b + grid, ... (<= 256 of them: the host
    // sizes the grid) by their cursors and sorts those above GS_MID pairs that fit their rows (a
    // spilled tile, above scap, is gathered and sorted by its blend workgroup: gs_spill_tile)
    if (tid == 0) s_list[GS_SORT_THREADS] = 0;
    __syncthreads();
    const uint32_t t = blockIdx.x + tid * gridDim.x;
    if (t < ntiles) {
      const uint32_t c = fu.cursor[t];
      if (c > GS_MID && c <= fu.scap) s_list[atomicAdd(&s_list[GS_SORT_THREADS], 1u)] = t;
    }
    __syncthreads();
    count = s_list[GS_SORT_THREADS];
  } else {
    count = large_ctr[GS_LC_COUNT];
  }
  // static striding over the list (a shared work counter serialises: ~30 ns per contended atomic,
  // 210 us for the 1M-Gaussian frame's 7k claims)
  for (uint32_t li = fu.scap ? 0 : blockIdx.x; li < count; li += fu.scap ? 1 : gridDim.x) {
    const uint32_t tile = fu.scap ? s_list[li] : large[li];
    const uint2 range = fu.scap ? make_uint2(tile * fu.scap, tile * fu.scap + fu.cursor[tile]) : ranges[tile];
    if (!fu.scap && range.y > cap) continue;  // segment beyond the pair buffer: spilled (gs_spill_tile)
    const uint32_t n = range.y - range.x;
    unsigned long long* seg = fu.scap ? const_cast<unsigned long long*>(tile_slots) + range.x
                            : n <= GS_TILE_SLOTS ? const_cast<unsigned long long*>(tile_slots) + (size_t)tile * GS_TILE_SLOTS
                                                 : pairs + range.x;
    const uint32_t* segw = reinterpret_cast<const uint32_t*>(seg);  // (gaussian, depth) word pairs
    const unsigned long long tbits = (unsigned long long)tile << 32;
    const uint32_t R = ((n + GS_SORT_THREADS - 1) / GS_SORT_THREADS) | 1u;
    if (R <= rmax) {
      const uint32_t h = gs_radix_tile(s_dep, s_dep + capn, s_slot, s_slot + capn, s_cnt, s_red, segw, n, R);
      gs_radix_publish(s_dep + h * capn, s_slot + h * capn, segw, n, tbits, keys_out ? keys_out + range.x : nullptr,
                       vals_out + range.x);
    } else if (g_dep && n <= GS_RADIX_MAXN && range.y <= g_cap) {
      // global scratch at the tile's pair offset: [2][g_cap] depths, [2][g_cap] positions
      uint32_t* d0 = g_dep + range.x;
      uint16_t* s0 = g_slot + range.x;
      const uint32_t h = gs_radix_tile(d0, d0 + g_cap, s0, s0 + g_cap, s_cnt, s_red, segw, n, R);
      gs_radix_publish(h ? d0 + g_cap : d0, h ? s0 + g_cap : s0, segw, n, tbits,
                       keys_out ? keys_out + range.x : nullptr, vals_out + range.x);
    } else {  // bitonic network in global memory (a frame whose tiles outgrew the scratch)
      bitonic_flip_sort(n, [&](uint32_t a, uint32_t b) {
        unsigned long long x = seg[a], y = seg[b];
        if (y < x) { seg[a] = y; seg[b] = x; }
      });
      for (uint32_t k = tid; k < n; k += GS_SORT_THREADS) {
        const unsigned long long v = seg[k];
        if (keys_out) keys_out[range.x + k] = tbits | (v >> 32);
        vals_out[range.x + k] = (uint32_t)v;
      }
    }
    __syncthreads();  // LDS reused by the next tile
  }
}

}  // namespace ptgs
