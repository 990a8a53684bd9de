// splat_bin.h — stage: the three-launch front end (count / colscan / scatter) and what the fused front end
// shares with it: the band / expand / clip / chunk walks, the blend's tile order, the spill re-arm. Relies on
// PreArgs and gs_preprocess_one (splat_preprocess.h), BinGrid (splat_plan.h), the counter words
// (splat_words.h), the wave primitives (splat_wave.h) and the stamps (splat_probe.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "splat_plan.h"
#include "splat_preprocess.h"
#include "splat_probe.h"
#include "splat_wave.h"
#include "splat_words.h"

namespace ptgs {

// ---- binning --------------------------------------------------------------------------------------
// No global atomics per pair (contended scattered atomics measured 100 us for C2's 617k pairs). The
// grid is (bands, chunks): a band is a run of band_rows tile rows (as many as fit GS_BAND_TILES: the
// whole 1080p frame is one band, 4K takes 4), a chunk a contiguous range of Gaussians.
//  count    block (band, c) preprocesses chunk c (band-0 blocks store the per-Gaussian outputs, the
//           others only recompute the rects) and counts the chunk's pairs in its band into an LDS
//           histogram (ds_add), written to hist[c][t].
//  colscan  one block per 64 tiles: hist[c][t] -> exclusive prefix over the chunks (in place), the
//           tile totals, their exclusive scan inside the 64-tile group and the group totals; K and
//           the largest tile go to pinned host memory (last block).
//  scatter  block (band, c): tile starts = scan of the group totals + in-group offset; re-walks chunk
//           c and places each pair at start[t] + hist[c][t] + (LDS cursor). Chunk-0 blocks publish
//           the ranges.
// Order inside a tile's segment depends on LDS atomic order and is fixed by the blend's per-tile sort.
#define GS_BIN_THREADS 1024
#ifndef GS_COUNT_THREADS
#define GS_COUNT_THREADS 1024  // the count's workgroup (the scatter keeps GS_BIN_THREADS)
#endif
// (GS_MAX_CHUNKS, GS_CHUNK_MIN, GS_BAND_TILES, GS_TILE_SLOTS, GS_MID, GS_MAX_GROUPS: splat_plan.h)

// The bands cover the frame's tile rows [row0, row1) only (a tile-row shard bins its own rows: one band of
// up to GS_MAX_CHUNKS chunks instead of the whole frame's bands); the 64-tile groups start at row0's first
// tile. hist, tile_info and ranges keep the frame's global tile ids (tiles = grid_x * grid_y).
__device__ __forceinline__ void gs_band(const BinGrid& bg, uint32_t& ty0, uint32_t& ty1) {
  ty0 = bg.row0 + blockIdx.x * bg.band_rows;
  ty1 = min(bg.row1, ty0 + bg.band_rows);
}

// Pairs of one wave's 64 entries (gaussian g, x0 | w << 16, y0 | h << 16; h = 0: none), walked 64 per
// step: a shuffle scan of the rect areas; lane q's pair belongs to the first entry whose inclusive
// sum exceeds q (6-step binary search over shuffles), its tile is (x0 + r % w, y0 + r / w) for its
// rank r inside that rect. Every lane works on every step but the last (a per-Gaussian rect loop
// idles the lanes of the smaller rects: C2's rects hold 1 to ~100 tiles). f(g, x, y, depth).
template <bool WANT_DEPTH, typename F>
__device__ __forceinline__ void gs_expand(uint32_t lane, uint32_t eg, uint32_t exw, uint32_t eyh, float dep, F f) {
  const uint32_t a = (exw >> 16) * (eyh >> 16);
  const uint32_t incl = wave_incl_scan(a);
  const uint32_t total = (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(incl, 63));
  const uint32_t excl = incl - a;
  for (uint32_t p = 0; p < total; p += 64) {
    const uint32_t qi = p + lane;
    uint32_t lo = 0;
#pragma unroll
    for (uint32_t step = 32; step; step >>= 1) lo = __shfl(incl, (int)(lo + step - 1)) <= qi ? lo + step : lo;
    const uint32_t og = __shfl(eg, (int)lo), oxw = __shfl(exw, (int)lo), oy = __shfl(eyh, (int)lo);
    const uint32_t oex = __shfl(excl, (int)lo);
    const float od = WANT_DEPTH ? __shfl(dep, (int)lo) : 0.0f;
    if (qi < total) {
      const uint32_t r = qi - oex, ow = oxw >> 16;
      uint32_t row = (uint32_t)((float)r * __builtin_amdgcn_rcpf((float)ow));  // r < 2^13: off by <= 1
      row = row * ow > r ? row - 1 : row;
      row = (row + 1) * ow <= r ? row + 1 : row;
      f(og, (oxw & 0xFFFFu) + (r - row * ow), (oy & 0xFFFFu) + row, od);
    }
  }
}

__device__ __forceinline__ void gs_clip(const ushort4& rc, uint32_t ty0, uint32_t ty1, uint32_t& xw, uint32_t& yh) {
  const uint32_t y0 = max((uint32_t)rc.y, ty0), y1 = min((uint32_t)rc.w, ty1);
  const bool hit = y0 < y1 && rc.x < rc.z;  // culled Gaussians hold the empty rect
  xw = (uint32_t)rc.x | ((uint32_t)(rc.z - rc.x) << 16);
  yh = hit ? (y0 | ((y1 - y0) << 16)) : 0u;
}

// Scatter's walk of chunk blockIdx.y inside the band: with several bands most rects miss the band, so
// each wave first filters (64 rects per step, GS_WALK_PF steps in flight; ballot + mbcnt append the
// hits to its GS_WQ-entry LDS ring) and expands 64 queued entries at a time (depths gathered then).
#define GS_WQ 128
#define GS_WALK_PF 4
template <typename F>
__device__ __forceinline__ void gs_walk_chunk(const BinGrid& bg, const ushort4* __restrict__ rects,
                                              const float* __restrict__ depths, const uint32_t* __restrict__ ids,
                                              uint32_t n, uint32_t ty0, uint32_t ty1, uint4* s_q, F f) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t b0 = blockIdx.y * bg.chunk, b1 = min(n, b0 + bg.chunk);
  const ushort4 zero = make_ushort4(0, 0, 0, 0);
  uint4* q = s_q + wave * GS_WQ;
  uint32_t base = b0 + wave * 64u;
  ushort4 pf[GS_WALK_PF];
#pragma unroll
  for (int k = 0; k < GS_WALK_PF; ++k) {  // (if/else: a ?: of two ushort4 lvalues selects addresses -> FLAT)
    const uint32_t i = base + k * GS_BIN_THREADS + lane;
    pf[k] = zero;
    if (i < b1) pf[k] = rects[i];
  }
  uint32_t head = 0, cnt = 0;  // wave-uniform ring state
  for (;;) {
    while (cnt < 64u && base < b1) {
      const ushort4 rc = pf[0];
#pragma unroll
      for (int k = 0; k < GS_WALK_PF - 1; ++k) pf[k] = pf[k + 1];
      {
        const uint32_t i = base + GS_WALK_PF * GS_BIN_THREADS + lane;
        pf[GS_WALK_PF - 1] = zero;
        if (i < b1) pf[GS_WALK_PF - 1] = rects[i];
      }
      uint32_t xw, yh;
      gs_clip(rc, ty0, ty1, xw, yh);
      const unsigned long long bal = __ballot(yh != 0u);
      if (bal) {
        if (yh) {
          const uint32_t pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
          q[(head + cnt + pos) & (GS_WQ - 1u)] = make_uint4(base + lane, xw, yh, ids ? ids[base + lane] : base + lane);
        }
        cnt += (uint32_t)__popcll(bal);
      }
      base += GS_BIN_THREADS;
    }
    if (cnt == 0) break;
    const uint32_t take = min(64u, cnt);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint4 e = lane < take ? q[(head + lane) & (GS_WQ - 1u)] : make_uint4(0u, 0u, 0u, 0u);
    head += take;
    cnt -= take;
    const float dep = lane < take ? depths[e.x] : 0.0f;
    gs_expand<true>(lane, e.w, e.y, e.z, dep, f);  // (e.w: the caller's index for the key)
  }
}

// The blend's tile order, built by one extra workgroup of the front end's first launch (fused or
// count) while the others bin: the tiles [tb, te) by the previous frame's pair count, heaviest first (a counting
// sort on min(255, n / 2), descending; the order inside a bucket is the LDS atomics'). The blend's
// workgroups are dispatched in index order, so its long-running tiles start first and the kernel's
// ramp-down runs light tiles only. Any permutation renders the same image: the previous frame's
// counts (ranges[t].y - .x, whatever path wrote them) only steer the schedule.
#define GS_ORDER_B 4u  // previous tile counts in flight per work-item (16: 104 VGPRs in the front-end kernels)
// (order[b] = the tile. Carrying the previous frame's count of the tile in the word, so the blend loads
// only that much of the key row with the tile, measured slower: C2 0.0594 vs 0.0588 ms)
__device__ __forceinline__ uint32_t gs_order_bucket_n(uint32_t n) {
  return GS_ORDER_BUCKETS - 1u - min(GS_ORDER_BUCKETS - 1u, n >> 1);
}
__device__ __forceinline__ uint32_t gs_order_bucket(uint2 r) { return gs_order_bucket_n(r.y > r.x ? r.y - r.x : 0u); }
// (COUNTS: prev holds one u32 pair count per tile, the fused front end's cursors of the frame itself)
template <bool COUNTS = false>
__device__ __forceinline__ uint32_t gs_order_bucket_at(const void* prev, uint32_t t) {
  return COUNTS ? gs_order_bucket_n(static_cast<const uint32_t*>(prev)[t]) : gs_order_bucket(static_cast<const uint2*>(prev)[t]);
}
template <bool COUNTS = false>
__device__ void gs_tile_order(const void* __restrict__ prev, uint32_t* __restrict__ order, uint32_t tb, uint32_t te,
                              uint32_t* s_h /* >= GS_ORDER_BUCKETS */) {
  // (the previous counts are loaded GS_ORDER_B per work-item at a time, all in flight before the first
  // is used: a loop of one load and one LDS atomic per iteration waited for every load, 16 dependent
  // round trips per pass at 1080p on the front end's critical path)
  const uint32_t tid = threadIdx.x, lane = tid & 63u, nth = blockDim.x;  // (>= 64)
  for (uint32_t b = tid; b < GS_ORDER_BUCKETS; b += nth) s_h[b] = 0;
  __syncthreads();
  for (uint32_t t0 = tb + tid; t0 < te; t0 += GS_ORDER_B * nth) {
    uint32_t bk[GS_ORDER_B];
#pragma unroll
    for (uint32_t j = 0; j < GS_ORDER_B; ++j) {
      const uint32_t t = t0 + j * nth;
      bk[j] = t < te ? gs_order_bucket_at<COUNTS>(prev, t) : GS_ORDER_BUCKETS;
    }
#pragma unroll
    for (uint32_t j = 0; j < GS_ORDER_B; ++j)
      if (bk[j] < GS_ORDER_BUCKETS) atomicAdd(s_h + bk[j], 1u);
  }
  __syncthreads();
  if (tid < 64) {  // exclusive scan of the buckets: one wave, four per lane
    const uint32_t c0 = s_h[4 * lane], c1 = s_h[4 * lane + 1], c2 = s_h[4 * lane + 2], c3 = s_h[4 * lane + 3];
    const uint32_t sum = (c0 + c1) + (c2 + c3);
    const uint32_t ex = wave_incl_scan(sum) - sum;
    s_h[4 * lane] = ex;
    s_h[4 * lane + 1] = ex + c0;
    s_h[4 * lane + 2] = ex + c0 + c1;
    s_h[4 * lane + 3] = ex + c0 + c1 + c2;
  }
  __syncthreads();
  for (uint32_t t0 = tb + tid; t0 < te; t0 += GS_ORDER_B * nth) {
    uint32_t bk[GS_ORDER_B];
#pragma unroll
    for (uint32_t j = 0; j < GS_ORDER_B; ++j) {
      const uint32_t t = t0 + j * nth;
      bk[j] = t < te ? gs_order_bucket_at<COUNTS>(prev, t) : GS_ORDER_BUCKETS;
    }
#pragma unroll
    for (uint32_t j = 0; j < GS_ORDER_B; ++j)
      if (bk[j] < GS_ORDER_BUCKETS) order[atomicAdd(s_h + bk[j], 1u)] = t0 + j * nth;
  }
}

// The tile order of an overlapped fused frame (SplatOverlap::own_order), from the frame's OWN pair counts
// (the cursors its front end has just reserved): it runs on the front-end stream behind the front end,
// off the caller's stream, where the blend of the previous frame hides it; the in-kernel order
// workgroup of a serial frame can only use the previous frame's counts.
// Up to GS_ORDER_R * GS_ORDER_THREADS tiles (1080p: 8 160) each work-item keeps its tiles' buckets in
// registers (one load round) and the histogram has GS_ORDER_COLS columns per bucket, one per lane & 15:
// the LDS atomics of a wave's lanes on one bucket (most light tiles share a few buckets) meet 4-way
// instead of 64-way (a single-column histogram serialised ~8k same-address atomics per pass, ~3.5 us).
// Larger grids (4K) take the generic two-pass order.
#ifndef GS_ORDER_THREADS
#define GS_ORDER_THREADS 1024
#endif
#define GS_ORDER_COLS 16u
#define GS_ORDER_R ((8192u + GS_ORDER_THREADS - 1u) / GS_ORDER_THREADS)
#define GS_ORDER_E (GS_ORDER_BUCKETS * GS_ORDER_COLS / GS_ORDER_THREADS)  // scanned entries per work-item
static_assert(GS_ORDER_E * GS_ORDER_THREADS == GS_ORDER_BUCKETS * GS_ORDER_COLS, "the order scan's split");
__global__ __launch_bounds__(GS_ORDER_THREADS) void gs_tile_order_kernel(const uint32_t* __restrict__ counts,
                                                                         uint32_t* __restrict__ order, uint32_t tb,
                                                                         uint32_t te) {
  __shared__ uint32_t s_h[GS_ORDER_BUCKETS * GS_ORDER_COLS];
  __shared__ uint32_t s_part[GS_ORDER_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, col = lane & (GS_ORDER_COLS - 1u);
  if (te - tb > GS_ORDER_R * GS_ORDER_THREADS) {
    gs_tile_order<true>(counts, order, tb, te, s_h);
    return;
  }
  uint32_t bk[GS_ORDER_R];
#pragma unroll
  for (uint32_t j = 0; j < GS_ORDER_R; ++j) {
    const uint32_t t = tb + tid + j * GS_ORDER_THREADS;
    bk[j] = t < te ? gs_order_bucket_n(counts[t]) : GS_ORDER_BUCKETS;
  }
  for (uint32_t k = tid; k < GS_ORDER_BUCKETS * GS_ORDER_COLS; k += GS_ORDER_THREADS) s_h[k] = 0;
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < GS_ORDER_R; ++j)
    if (bk[j] < GS_ORDER_BUCKETS) atomicAdd(s_h + bk[j] * GS_ORDER_COLS + col, 1u);
  __syncthreads();
  // exclusive scan of the (bucket, column) counts in bucket-major order
  uint32_t v[GS_ORDER_E], sum = 0;
#pragma unroll
  for (uint32_t e = 0; e < GS_ORDER_E; ++e) {
    v[e] = s_h[tid * GS_ORDER_E + e];
    sum += v[e];
  }
  const uint32_t incl = wave_incl_scan(sum);
  if (lane == 63u) s_part[wave] = incl;
  __syncthreads();
  uint32_t ex = incl - sum;
  for (uint32_t w = 0; w < wave; ++w) ex += s_part[w];
#pragma unroll
  for (uint32_t e = 0; e < GS_ORDER_E; ++e) {
    s_h[tid * GS_ORDER_E + e] = ex;
    ex += v[e];
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < GS_ORDER_R; ++j)
    if (bk[j] < GS_ORDER_BUCKETS) order[atomicAdd(s_h + bk[j] * GS_ORDER_COLS + col, 1u)] = tb + tid + j * GS_ORDER_THREADS;
}

// Spill accounting (see gs_spill_tile), run by the first front-end launch's block (0, 0): the previous
// frame's spill demand (GS_FZ_POOL_CURSOR, which its spilled tiles advanced; that frame's blend has
// finished: stream order) goes to the host (GS_KH_SPILL_DEMAND, the pool's next size) and the running
// maximum (GS_FZ_MAX_DEMAND); the cursor restarts at 0 for this frame's blend.
__device__ __forceinline__ void gs_spill_rearm(uint32_t* fz, uint32_t* k_host) {
  const uint32_t d = fz[GS_FZ_POOL_CURSOR];
  __atomic_store_n(k_host + GS_KH_SPILL_DEMAND, d, __ATOMIC_RELAXED);
  if (d > fz[GS_FZ_MAX_DEMAND]) fz[GS_FZ_MAX_DEMAND] = d;
  fz[GS_FZ_POOL_CURSOR] = 0;  // (the demand reaches the host with the blend's system fence: no fence here)
}

// Bounding tile rect (x0, y0, x1, y1) of one front-end workgroup's clipped Gaussian rects, reduced over
// the workgroup (every work-item passes its running bounds; s_r: 4 x waves words of LDS); work-item 0
// stores it (empty: x0 > x1). A spilled tile's blend workgroup looks only at the chunks whose rect
// holds it.
template <uint32_t NT>
__device__ __forceinline__ void gs_store_chunk_rect(uint32_t bx0, uint32_t by0, uint32_t bx1, uint32_t by1,
                                                    uint32_t (*s_r)[NT / 64], ushort4* crect, uint32_t wg) {
  for (int off = 32; off > 0; off >>= 1) {
    bx0 = min(bx0, (uint32_t)__shfl_xor((int)bx0, off));
    by0 = min(by0, (uint32_t)__shfl_xor((int)by0, off));
    bx1 = max(bx1, (uint32_t)__shfl_xor((int)bx1, off));
    by1 = max(by1, (uint32_t)__shfl_xor((int)by1, off));
  }
  if ((threadIdx.x & 63u) == 0) {
    s_r[0][threadIdx.x >> 6] = bx0;
    s_r[1][threadIdx.x >> 6] = by0;
    s_r[2][threadIdx.x >> 6] = bx1;
    s_r[3][threadIdx.x >> 6] = by1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (uint32_t w = 1; w < NT / 64; ++w) {
      bx0 = min(bx0, s_r[0][w]);
      by0 = min(by0, s_r[1][w]);
      bx1 = max(bx1, s_r[2][w]);
      by1 = max(by1, s_r[3][w]);
    }
    crect[wg] = bx0 < bx1 ? make_ushort4((unsigned short)bx0, (unsigned short)by0, (unsigned short)bx1, (unsigned short)by1)
                          : make_ushort4(1, 1, 0, 0);
  }
}

// preprocess + count. Block (0, 0) also re-arms the frame's counters.
template <bool ROWCULL>
__global__ __launch_bounds__(GS_COUNT_THREADS, 4) void gs_bin_count_kernel(SplatCam cam, PreArgs A, BinGrid bg,
                                                                      uint32_t* __restrict__ hist,
                                                                      uint32_t* __restrict__ total,
                                                                      uint32_t* __restrict__ large_ctr,
                                                                      uint32_t* k_host, uint32_t* __restrict__ nzbuf,
                                                                      const uint2* __restrict__ prev_ranges,
                                                                      uint32_t* __restrict__ order, uint32_t order_tb,
                                                                      uint32_t order_te, uint32_t* __restrict__ fz,
                                                                      ushort4* __restrict__ crect) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];  // band_rows * grid_x (>= GS_ORDER_BUCKETS)
  if (order && blockIdx.y == gridDim.y - 1) {  // the extra row of blocks: the blend's tile order
    if (blockIdx.x == 0) gs_tile_order(prev_ranges, order, order_tb, order_te, s_hist);
    return;
  }
  uint32_t ty0, ty1;
  gs_band(bg, ty0, ty1);
  const uint32_t nt = (ty1 - ty0) * bg.grid_x;
  for (uint32_t k = threadIdx.x; k < nt; k += GS_COUNT_THREADS) s_hist[k] = 0;
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    total[GS_TOT_MAX_TILE] = 0;  // (colscan's atomicMax; the scatter hands it to the host)
    large_ctr[GS_LC_COUNT] = 0;  // (colscan's list)
    gs_spill_rearm(fz, k_host);
  }
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t b0 = blockIdx.y * bg.chunk, b1 = min(A.n, b0 + bg.chunk);
  uint32_t bx0 = 0xFFFFu, by0 = 0xFFFFu, bx1 = 0u, by1 = 0u;  // the chunk's rect in the band (gs_spill_tile)
  for (uint32_t base = b0 + wave * 64u; base < b1; base += GS_COUNT_THREADS) {
    const uint32_t i = base + lane;
    ushort4 rc = make_ushort4(0, 0, 0, 0);
    // (tile-row shard with chunk bounds: a 256-Gaussian chunk whose bound misses the rows is skipped
    // before its Gaussians are loaded; a wave's 64 lie in at most two chunks)
    const bool skip = cam.cull && i < b1 && A.cskip[i >> 8];
    if (i < b1 && !skip)
      rc = blockIdx.x == 0 ? gs_preprocess_one<true, ROWCULL>(cam, A, i) : gs_preprocess_one<false, ROWCULL>(cam, A, i);
    else if (i < b1 && blockIdx.x == 0) gs_store_skipped(A, i);
    uint32_t xw, yh;
    gs_clip(rc, ty0, ty1, xw, yh);
    if (yh) {
      bx0 = min(bx0, xw & 0xFFFFu);
      bx1 = max(bx1, (xw & 0xFFFFu) + (xw >> 16));
      by0 = min(by0, yh & 0xFFFFu);
      by1 = max(by1, (yh & 0xFFFFu) + (yh >> 16));
    }
    if (__ballot(yh != 0u))
      gs_expand<false>(lane, i, xw, yh, 0.0f, [&](uint32_t, uint32_t x, uint32_t y, float) {
        atomicAdd(s_hist + (y - ty0) * bg.grid_x + x, 1u);
      });
  }
  __syncthreads();
  uint32_t* row = hist + (size_t)blockIdx.y * bg.tiles + ty0 * bg.grid_x;
  uint32_t nz = 0;
  for (uint32_t k = threadIdx.x; k < nt; k += GS_COUNT_THREADS) {
    const uint32_t c = s_hist[k];
    row[k] = c;
    nz += c != 0u;
  }
  // touched (chunk, tile) entries, the front-end policy's measure of spatial coherence (the fused
  // path would reserve each with an atomic), per workgroup; the scatter's block (0, 0) sums them for
  // the host (GS_KH_RUNS)
  for (int off = 32; off > 0; off >>= 1) nz += (uint32_t)__shfl_xor((int)nz, off);
  __shared__ uint32_t s_nz[GS_COUNT_THREADS / 64];
  if ((threadIdx.x & 63u) == 0) s_nz[threadIdx.x >> 6] = nz;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (uint32_t w = 0; w < GS_COUNT_THREADS / 64; ++w) t += s_nz[w];
    nzbuf[blockIdx.y * gridDim.x + blockIdx.x] = t;  // (summed by the scatter's block (0, 0): no fan-in atomics)
  }
  __shared__ uint32_t s_rr[4][GS_COUNT_THREADS / 64];
  gs_store_chunk_rect<GS_COUNT_THREADS>(bx0, by0, bx1, by1, s_rr, crect, blockIdx.y * gridDim.x + blockIdx.x);
}

// One 256-work-item block per 64-tile group g: wave w sums chunks [w*cpw, (w+1)*cpw) of the group's
// 64 tiles (lane = tile: coalesced rows), then rewrites hist[c][t] as the exclusive prefix over c.
// Outputs per tile (offset inside the group, total), per group its total, atomicMax of the largest
// tile into GS_TOT_MAX_TILE, and the tiles of more than `thr` pairs appended to the large-tile list.
#ifndef GS_COLSCAN_WAVES
#define GS_COLSCAN_WAVES 16
#endif
#define GS_COLSCAN_THREADS (64 * GS_COLSCAN_WAVES)
#define GS_CS_REG 16u  // chunk rows per colscan wave kept in registers
static_assert(GS_MAX_CHUNKS <= GS_COLSCAN_WAVES * 64, "colscan: at most 64 chunk rows per wave");
__global__ __launch_bounds__(GS_COLSCAN_THREADS) void gs_bin_colscan_kernel(BinGrid bg, uint32_t* __restrict__ hist,
                                                             uint2* __restrict__ tile_info,
                                                             uint32_t* __restrict__ group_total,
                                                             uint32_t* __restrict__ total, uint32_t thr,
                                                             uint32_t* __restrict__ large,
                                                             uint32_t* __restrict__ large_ctr) {
  __shared__ uint32_t s_ws[GS_COLSCAN_WAVES][64];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t t = bg.row0 * bg.grid_x + blockIdx.x * 64u + lane;
  const bool ok = t < bg.row1 * bg.grid_x;
  const uint32_t cpw = (bg.chunks + GS_COLSCAN_WAVES - 1u) / GS_COLSCAN_WAVES, c0 = wave * cpw,
                 c1 = min(bg.chunks, c0 + cpw);
  // the wave's first GS_CS_REG rows in flight at once and kept in registers (fully unrolled: every
  // frame of up to 256 chunks); rows beyond them (more chunks: 10M Gaussians at 4K, single-band tile-row
  // shards of large sets) in batches of GS_CS_REG, read again for the rewrite
  uint32_t h[GS_CS_REG];
  uint32_t sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < GS_CS_REG; ++k) {
    h[k] = (ok && c0 + k < c1) ? hist[(size_t)(c0 + k) * bg.tiles + t] : 0u;
    sum += h[k];
  }
  for (uint32_t k0 = GS_CS_REG; k0 < cpw; k0 += GS_CS_REG) {
    uint32_t x[GS_CS_REG];
#pragma unroll
    for (uint32_t k = 0; k < GS_CS_REG; ++k) x[k] = (ok && c0 + k0 + k < c1) ? hist[(size_t)(c0 + k0 + k) * bg.tiles + t] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < GS_CS_REG; ++k) sum += x[k];
  }
  s_ws[wave][lane] = sum;
  __syncthreads();
  uint32_t run = 0;
  for (uint32_t w = 0; w < wave; ++w) run += s_ws[w][lane];
#pragma unroll
  for (uint32_t k = 0; k < GS_CS_REG; ++k)
    if (ok && c0 + k < c1) {
      hist[(size_t)(c0 + k) * bg.tiles + t] = run;
      run += h[k];
    }
  for (uint32_t k0 = GS_CS_REG; k0 < cpw; k0 += GS_CS_REG) {
    uint32_t x[GS_CS_REG];
#pragma unroll
    for (uint32_t k = 0; k < GS_CS_REG; ++k) x[k] = (ok && c0 + k0 + k < c1) ? hist[(size_t)(c0 + k0 + k) * bg.tiles + t] : 0u;
#pragma unroll
    for (uint32_t k = 0; k < GS_CS_REG; ++k)
      if (ok && c0 + k0 + k < c1) {
        hist[(size_t)(c0 + k0 + k) * bg.tiles + t] = run;
        run += x[k];
      }
  }
  if (wave != 0) return;
  uint32_t tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < GS_COLSCAN_WAVES; ++w) tot += s_ws[w][lane];
  const uint32_t incl = wave_incl_scan(tot);
  if (ok) tile_info[t] = make_uint2(incl - tot, tot);  // (offset inside the group, tile total)
  const bool big = ok && tot > thr;
  const unsigned long long bal = __ballot(big);
  if (bal) {
    uint32_t at = 0;
    if (lane == 0) at = atomicAdd(large_ctr + GS_LC_COUNT, (uint32_t)__popcll(bal));
    at = (uint32_t)__shfl((int)at, 0);
    if (big) large[at + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = t;
  }
  uint32_t mx = tot;
  for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off));
  const uint32_t gsum = __shfl(incl, 63);
  if (lane == 0) {
    group_total[blockIdx.x] = gsum;
    if (mx) atomicMax(total + GS_TOT_MAX_TILE, mx);
  }
}

// K = the sum of the group totals (every block scans them all); block (0, 0) publishes it to GS_TOT_PAIRS
// and, with the frame's other hints, to pinned host memory (GsHostWord). A pair is written only where it
// fits the pair buffer (the host sizes it from the previous K and, with stats, re-runs scatter + blend
// after growing it when it did not: see splat_gaussians).
__global__ __launch_bounds__(GS_BIN_THREADS) void gs_bin_scatter_kernel(
    BinGrid bg, const ushort4* __restrict__ rects, const float* __restrict__ depths, const uint32_t* __restrict__ ids,
    uint32_t n,
    const uint32_t* __restrict__ hist, const uint2* __restrict__ tile_info, const uint32_t* __restrict__ group_total,
    uint32_t* __restrict__ total, const uint32_t* __restrict__ large_ctr, uint32_t* k_host,
    const uint32_t* __restrict__ nzbuf, uint32_t nzn, uint32_t cap,
    uint2* __restrict__ ranges,
    unsigned long long* __restrict__ pairs, unsigned long long* __restrict__ tile_slots) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cur[];  // 2 * band_rows * grid_x + groups
  __shared__ uint4 s_q[GS_BIN_THREADS / 64 * GS_WQ];
  __shared__ uint32_t s_part[GS_BIN_THREADS / 64];
  uint32_t ty0, ty1;
  gs_band(bg, ty0, ty1);
  const uint32_t nt = (ty1 - ty0) * bg.grid_x, t0 = ty0 * bg.grid_x;
  uint32_t* s_tot = s_cur + bg.band_rows * bg.grid_x;
  uint32_t* s_gpre = s_tot + bg.band_rows * bg.grid_x;
  const uint32_t c = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  // exclusive scan of the group totals
  const uint32_t gend = bg.groups;
  uint32_t carry = 0;
  for (uint32_t g0 = 0; g0 < gend; g0 += GS_BIN_THREADS) {
    const uint32_t g = g0 + tid;
    const uint32_t v = g < gend ? group_total[g] : 0u;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63) s_part[wv] = incl;
    __syncthreads();
    uint32_t woff = carry, all = carry;
    for (uint32_t w = 0; w < GS_BIN_THREADS / 64; ++w) {
      woff += w < wv ? s_part[w] : 0u;
      all += s_part[w];
    }
    if (g < gend) s_gpre[g] = woff + incl - v;
    carry = all;
    __syncthreads();
  }
  uint32_t nzsum = 0;
  if (blockIdx.x == 0 && blockIdx.y == 0) {  // the count's touched entries (per workgroup)
    for (uint32_t k = tid; k < nzn; k += GS_BIN_THREADS) nzsum += nzbuf[k];
    for (int off = 32; off > 0; off >>= 1) nzsum += (uint32_t)__shfl_xor((int)nzsum, off);
    if (lane == 0) s_part[wv] = nzsum;
    __syncthreads();
    nzsum = 0;
    for (uint32_t w = 0; w < GS_BIN_THREADS / 64; ++w) nzsum += s_part[w];
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
    total[GS_TOT_PAIRS] = carry;
    __atomic_store_n(k_host + GS_KH_MAX_TILE, total[GS_TOT_MAX_TILE], __ATOMIC_RELAXED);  // (the next sort's LDS size)
    __atomic_store_n(k_host + GS_KH_LARGE_TILES, large_ctr[GS_LC_COUNT], __ATOMIC_RELAXED);  // (the next sort grid)
    __atomic_store_n(k_host + GS_KH_RUNS, nzsum, __ATOMIC_RELAXED);  // touched (chunk, tile) entries
    __atomic_store_n(k_host + GS_KH_OVER_SCAP, 0u, __ATOMIC_RELAXED);
    __atomic_store_n(k_host + GS_KH_PUBLISHED_BY, 2u, __ATOMIC_RELAXED);  // three launches
    __atomic_store_n(k_host + GS_KH_PAIRS, carry, __ATOMIC_RELAXED);  // the host's K read-back
    if (carry > total[GS_TOT_MAX_K]) total[GS_TOT_MAX_K] = carry;  // (fused frames: GS_FZ_MAX_K)
    __atomic_store_n(k_host + GS_KH_MAX_K_THREE, total[GS_TOT_MAX_K], __ATOMIC_RELAXED);
    __threadfence_system();  // visible to the host before the kernel ends (the K event has no system fence)
  }
  if (blockIdx.x == 0 && blockIdx.y == 0 && (bg.row0 > 0 || bg.row1 < bg.grid_y)) {
    // a tile-row frame's bands cover its rows only: the other tiles' ranges are empty (as the oracle's)
    const uint32_t tb = bg.row0 * bg.grid_x, te = bg.row1 * bg.grid_x;
    for (uint32_t t = tid; t < bg.tiles; t += GS_BIN_THREADS)
      if (t < tb || t >= te) ranges[t] = make_uint2(0u, 0u);
  }
  // (K above the pair buffer: the tiles whose segment ends beyond it keep none of their pairs here and
  // are rendered by the blend through gs_spill_tile; the fixed rows of small tiles always fit)
  for (uint32_t k = tid; k < nt; k += GS_BIN_THREADS) {
    const uint32_t t = t0 + k;
    const uint2 ti = tile_info[t];
    const uint32_t start = s_gpre[(t - bg.row0 * bg.grid_x) >> 6] + ti.x;
    s_cur[k] = hist[(size_t)c * bg.tiles + t];
    // where the tile's pairs go: its fixed GS_TILE_SLOTS-slot row when they fit (the blend then
    // loads keys without waiting for the range), else its segment of the pair buffer (flag bit 31)
    s_tot[k] = ti.y <= GS_TILE_SLOTS ? t * GS_TILE_SLOTS : (start | 0x80000000u);
    if (c == 0) ranges[t] = ti.y ? make_uint2(start, start + ti.y) : make_uint2(0u, 0u);
  }
  __syncthreads();
  auto put = [&](uint32_t i, uint32_t x, uint32_t y, float d) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | i;
    const uint32_t k = (y - ty0) * bg.grid_x + x;
    const uint32_t rel = atomicAdd(s_cur + k, 1u), dst = s_tot[k];
    if (dst & 0x80000000u) {
      const uint32_t at = (dst & 0x7FFFFFFFu) + rel;
      if (at < cap) pairs[at] = key;
    } else {
      tile_slots[dst + rel] = key;
    }
  };
  if (bg.bands == 1) {  // one band: every rect meets it, so no filtering ring (one Gaussian per lane, as the count;
                        // -0.4 us at C2, kernel trace)
    const uint32_t b0 = c * bg.chunk, b1 = min(n, b0 + bg.chunk);
    for (uint32_t base = b0 + wv * 64u; base < b1; base += GS_BIN_THREADS) {
      const uint32_t i = base + lane;
      ushort4 rc = make_ushort4(0, 0, 0, 0);
      float d = 0.0f;
      if (i < b1) {
        rc = rects[i];
        d = depths[i];
      }
      uint32_t xw, yh;
      gs_clip(rc, ty0, ty1, xw, yh);
      if (__ballot(yh != 0u)) gs_expand<true>(lane, ids && i < b1 ? ids[i] : i, xw, yh, d, put);
    }
    return;
  }
  gs_walk_chunk(bg, rects, depths, ids, n, ty0, ty1, s_q, put);
}

}  // namespace ptgs
