// splat_blend.h — stage: the per-tile sort and blend (one workgroup per 16x16 tile) and the two publish
// kernels of a fused frame. Relies on GsFused (splat_fused.h), GsSpill and gs_spill_tile (splat_spill.h),
// the wave sort and scan (splat_wave.h), the counter words (splat_words.h), SplatCam and the tile
// constants (splat_plan.h), gs_st4_nt (splat_preprocess.h) and the stamps / probes (splat_probe.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "splat_fused.h"
#include "splat_plan.h"
#include "splat_preprocess.h"
#include "splat_probe.h"
#include "splat_spill.h"
#include "splat_wave.h"
#include "splat_words.h"

namespace ptgs {

// ---- blend ----------------------------------------------------------------------------------------
// Merge ranking (tiles of more than GS_MERGE_MIN pairs): every wave sorts its 64 keys in registers
// (bitonic network over the lanes, ascending), the sorted runs go to LDS, and a key's rank is its lane
// plus, for every other run, the count of that run's keys below it (a binary search of 7 LDS reads):
// ~200 VALU per key for 2-4 runs and ~400 for 8 instead of n / 4 compares against every key (the
// counting below): keys are unique, so the ranks are the same.
// (the wave's sort: gs_wave_sort64, splat_wave.h)

// keys below x in the sorted 64-key runs [0, m) of s_key except run `self` (m <= R): the binary searches
// of every run advance in lockstep, so each step's R LDS reads are in flight together (one round trip
// per step instead of one per step and run); runs >= m are read but not counted
template <uint32_t R>
__device__ __forceinline__ uint32_t gs_runs_below(const unsigned long long* s_key, uint32_t m, uint32_t self,
                                                  unsigned long long x) {
  uint32_t pos[R];
#pragma unroll
  for (uint32_t q = 0; q < R; ++q) pos[q] = 0;
#pragma unroll
  for (uint32_t step = 32; step; step >>= 1) {
    unsigned long long v[R];
#pragma unroll
    for (uint32_t q = 0; q < R; ++q) v[q] = s_key[64u * q + pos[q] + step - 1u];
#pragma unroll
    for (uint32_t q = 0; q < R; ++q) pos[q] += (q < m && q != self && v[q] < x) ? step : 0u;
  }
  uint32_t r = 0;
  unsigned long long v[R];
#pragma unroll
  for (uint32_t q = 0; q < R; ++q) v[q] = s_key[64u * q + pos[q]];
#pragma unroll
  for (uint32_t q = 0; q < R; ++q) r += (q < m && q != self) ? pos[q] + (v[q] < x ? 1u : 0u) : 0u;
  return r;
}
// keys of the sorted 64-key run b below x
__device__ __forceinline__ uint32_t gs_run_below(const unsigned long long* b, unsigned long long x) {
  uint32_t pos = 0;
#pragma unroll
  for (uint32_t step = 32; step; step >>= 1)
    if (b[pos + step - 1] < x) pos += step;
  return pos + (b[pos] < x ? 1u : 0u);
}
#ifndef GS_MERGE_MIN
#define GS_MERGE_MIN 96u  // (counting is cheaper for up to ~1.5 runs)
#endif
#define GS_ARENA (48 * (GS_BLOCK + 1) + 4 * (GS_BLOCK + 4) * 4)  // staged records + per-quadrant lists

struct GStage {  // one staged blend record (see gs_preprocess_one)
  float4 a, b, c;
};

static_assert(GS_ARENA >= 8u * GS_SPILL_LDS + 4u * (GS_SPILL_CAND + 3u), "gs_spill_tile's keys, candidates and counters fit the arena");

// One 256-work-item workgroup per 16x16 tile (a persistent, software-pipelined variant that loads
// the next tile's keys during the current one measured slower: static tile assignment loses to the
// dispatcher's dynamic balancing, 103 vs 72 us at C2; a tile-pair workgroup shading two pixels per
// lane in packed f32 measured 133 vs 104 us per frame: the per-pixel done / valid bookkeeping of the
// pair and the strip lists cost more than the packing saved).
//  sort     tiles of <= 256 pairs: one key per work-item; up to GS_MERGE_MIN pairs ranked by counting
//           against all n keys in LDS, above that by merge ranking (gs_wave_sort64 + gs_run_below);
//           while it runs, the blend records of the unsorted keys are already in flight, and the
//           staging slot of sorted position r is recorded; then publish the sorted keys (tile << 32 |
//           depth) / values (gaussian). Tiles of (256, GS_MID] pairs are merge-ranked two keys per
//           work-item. Larger tiles were sorted and published by gs_sort_large_kernel: their values
//           are streamed in batches of 256, the records of batch b + 1 (and the values of b + 2) in
//           flight while batch b blends.
//  blend    wave w shades the 8x8 quadrant q = w of the tile (x half w & 1, y half w >> 1), one pixel
//           per lane. Each staged Gaussian's alpha box is tested against the four quadrants (a 4-bit
//           mask in LDS; small tiles add the exact per-quadrant test, stage_rec); every wave ballots
//           bit w over the batch's masks in sorted order into its own list (no cross-wave counts: one
//           barrier per batch), so a wave iterates only the Gaussians that can touch its 64 pixels.
//           alpha = min(0.99, 2^z) with the hardware exp2 (within 1e-4 relative L2 of the oracle's exp,
//           test_raster_gpu.py); front to back, stop before the Gaussian that would take T below 1e-4
//           (the reference's rule).
// OVER (hybrid composite): per-pixel depth limit and an "under" image instead of the background colour
// Measured and rejected here: per-4x4-sub-block lists, one per ds_read_b128 lane group of a wave (each
// group reads its own list's record in the cycle a broadcast takes, 16% fewer evaluation steps at C2):
// 0.0596 vs 0.0564 ms, the u16 lists' unpacking, four ballots per compaction round and the sub-block
// masks cost more than the steps saved (the machinery alone with quadrant lists: 0.0620 ms); and (git
// history: round 4) records read by one lane and broadcast with
// readfirstlane (C2 0.0784 vs 0.0565 ms), alphas of several entries computed ahead of the transmittance
// chain, the termination applied without its wave-uniform branch, an XCD-aware tile mapping, loading the
// key row only up to the previous frame's count, non-temporal records / key rows.
#define GS_DONE_EVERY 4u  // list entries between the wave's all-pixels-done tests (a power of two >= 4)
// (the termination as two selects per entry instead of the wave-uniform branch: 2 spilled VGPRs, C2 serial
// 0.0607 vs 0.0563 ms, round 6)
// (Measured and rejected, round 6: the quadratic as three packed v_pk_mul / v_pk_fma_f32 over the record's
// (A, C) (B, D) (E, F) pairs plus one add, and red / green as one packed FMA: 13 VALU per entry instead of
// 15, but C2 0.0574 vs 0.0558 ms: the packed ops' dependency stalls (s_nop) lengthen each wave's chain.)
#ifndef GS_BLEND_MIN_BLOCKS
#define GS_BLEND_MIN_BLOCKS 8  // 64 VGPRs: 8 waves per SIMD (vs 7 at 70 VGPRs): +3% at C2
#endif
template <bool OVER>
__global__ __launch_bounds__(GS_BLOCK, GS_BLEND_MIN_BLOCKS) void gs_sort_blend_kernel(SplatCam cam, const uint2* __restrict__ ranges,
                                                                 unsigned long long* __restrict__ pairs,
                                                                 uint32_t sorted_above,
                                                                 unsigned long long* __restrict__ keys_out,
                                                                 uint32_t* __restrict__ vals_out,
                                                                 const float4* __restrict__ rec, float bg_r,
                                                                 float bg_g, float bg_b,
                                                                 uint32_t cap, uint32_t slot_keys,
                                                                 const unsigned long long* __restrict__ tile_slots,
                                                                 const float* __restrict__ depth_lim,
                                                                 const float4* __restrict__ under,
                                                                 float4* __restrict__ out, GsFused fu, GsSpill sp) {
  // staged records of the current batch; slot GS_BLOCK is a null Gaussian (alpha = 0) that pads the
  // per-quadrant lists to a multiple of 4.
  __shared__ __attribute__((aligned(16))) char s_arena[GS_ARENA];
  GStage* s_stage = reinterpret_cast<GStage*>(s_arena);
  uint32_t(*s_list)[GS_BLOCK + 4] = reinterpret_cast<uint32_t(*)[GS_BLOCK + 4]>(s_arena + sizeof(GStage) * (GS_BLOCK + 1));
  // the merge ranks' sorted runs and a mid tile's ranked keys alias the arena: records are staged only
  // after the last read of either (behind a barrier)
  unsigned long long* s_key = reinterpret_cast<unsigned long long*>(s_arena);
  __shared__ uint8_t s_mask[GS_BLOCK];
  __shared__ uint8_t s_sslot[GS_BLOCK];  // small tiles: staging slot of sorted position p
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  STAMP(1, 0);
  if (fu.seq_flag && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0)  // (this blend has started: SplatSeq)
    __hip_atomic_store(fu.seq_flag, fu.seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  if (fu.scap) {
    // fused front end: block (0, 0) hands the frame's counters to the host and re-arms them (the
    // fused kernel that produced them has finished; no other blend block reads them)
    uint32_t fp = 0, fr = 0;  // the front end's pairs and reservations (block (0, 0) sums the partials)
    if (blockIdx.x == 0 && blockIdx.y == 0) {
      for (uint32_t k = tid; k < fu.nwg; k += GS_BLOCK) {
        fp += fu.fzp[2 * k];
        fr += fu.fzp[2 * k + 1];
      }
      for (int off = 32; off > 0; off >>= 1) {
        fp += (uint32_t)__shfl_xor((int)fp, off);
        fr += (uint32_t)__shfl_xor((int)fr, off);
      }
      uint32_t* s_r = reinterpret_cast<uint32_t*>(s_arena);  // (before any other use of the arena)
      if (lane == 0) {
        s_r[wave] = fp;
        s_r[4 + wave] = fr;
      }
      __syncthreads();
      fp = (s_r[0] + s_r[1]) + (s_r[2] + s_r[3]);
      fr = (s_r[4] + s_r[5]) + (s_r[6] + s_r[7]);
      __syncthreads();
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) {
      const uint32_t big = fu.fz[GS_FZ_MAX_TILE];
      __atomic_store_n(fu.k_host + GS_KH_MAX_TILE, big > 256u ? big : 256u, __ATOMIC_RELAXED);  // (a bound)
      __atomic_store_n(fu.k_host + GS_KH_LARGE_TILES, fu.fz[GS_FZ_ABOVE_MID], __ATOMIC_RELAXED);
      __atomic_store_n(fu.k_host + GS_KH_RUNS, fr, __ATOMIC_RELAXED);  // reservations
      __atomic_store_n(fu.k_host + GS_KH_OVER_SCAP, fu.fz[GS_FZ_OVER_SCAP], __ATOMIC_RELAXED);  // (spilled)
      __atomic_store_n(fu.k_host + GS_KH_PUBLISHED_BY, 1u, __ATOMIC_RELAXED);  // fused
      __atomic_store_n(fu.k_host + GS_KH_PAIRS, fp, __ATOMIC_RELAXED);
      if (fp > fu.fz[GS_FZ_MAX_K]) fu.fz[GS_FZ_MAX_K] = fp;  // (three-launch frames: GS_TOT_MAX_K)
      __atomic_store_n(fu.k_host + GS_KH_MAX_K_FUSED, fu.fz[GS_FZ_MAX_K], __ATOMIC_RELAXED);
      fu.fz[GS_FZ_MAX_TILE] = 0;
      fu.fz[GS_FZ_ABOVE_MID] = 0;
      fu.fz[GS_FZ_OVER_SCAP] = 0;
      __threadfence_system();
    }
    if (blockIdx.x == 0 && blockIdx.y == 0) {  // the slice queue of the front end back to empty
      const uint32_t used = min(fu.fz[GS_FZ_Q_ENTRIES], fu.fsq_cap);
      for (uint32_t k = tid; k < used; k += GS_BLOCK) fu.fsq[k] = make_uint2(0u, 0u);
      if (tid == 0) {
        __atomic_store_n(fu.k_host + GS_KH_QUEUED, fu.fz[GS_FZ_Q_ENTRIES], __ATOMIC_RELAXED);  // (the helper count)
        fu.fz[GS_FZ_Q_CLAIMS] = 0;
        fu.fz[GS_FZ_Q_ENTRIES] = 0;
        fu.fz[GS_FZ_Q_OWNERS] = 0;
      }
    }
  }
  uint32_t tile_x = blockIdx.x, tile_y = cam.row_begin + blockIdx.y;
  uint32_t tile = tile_y * cam.grid_x + tile_x;
  if (fu.order) {  // heavy tiles first (gs_tile_order)
    tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)fu.order[blockIdx.y * gridDim.x + blockIdx.x]);
    tile_y = tile / cam.grid_x;
    tile_x = tile - tile_y * cam.grid_x;
  }
  STAMP(1, 4);
  const float tx0 = (float)(tile_x * GS_BLOCK_X), ty0 = (float)(tile_y * GS_BLOCK_Y);
  // Stage a record with its 2D mean in tile-local pixel coordinates (gx, gy): the blend evaluates
  // z = A dx^2 + B dx dy + C dy^2 + log2 o from (dx, dy) = pixel - mean, the form in which ptgs.h states the
  // function. (Until tests/test_splat_forward_gpu.py the record held the quadratic expanded in (ux, uy),
  // A ux^2 + B ux uy + C uy^2 + D ux + E uy + F, five FMAs instead of seven operations: for a Gaussian that is all
  // dilation, conic 1 / 0.3, F and D ux reach 1 200 inside the tile and cancel to a z of a few units, up to 1e-4
  // in z and 5e-5 in a pixel; the expansion now serves the exact quadrant test below alone, whose 0.02 margin
  // covers that.) Return the quadrant mask of its alpha box: bit q = (x half q & 1, y half q >> 1), the box tested
  // in tile-local coordinates against the quadrants' pixel ranges [0, 7] / [8, 15] (immediates: no
  // register holds a tile bound across the batch loop; the box's 1% + 0.01 px margin covers the
  // rounding of the local shift). exact: also the exact quadrant test (small tiles; the large-tile batch
  // loop keeps the box test: its copy of the test spilled 2 VGPRs).
  auto stage_rec = [&](uint32_t slot, const float4& ga, const float4& gb, const float4& gc, bool exact) -> uint32_t {
    const float gx = ga.x - tx0, gy = ga.y - ty0, A = ga.z, B = ga.w, C = gb.x;
    const float D = -2.0f * A * gx - B * gy, E = -B * gx - 2.0f * C * gy;
    const float F = ((A * gx * gx + B * gx * gy) + C * gy * gy) + gb.y;
    s_stage[slot].a = make_float4(A, B, C, gx);
    s_stage[slot].b = make_float4(gy, gb.y, gb.z, gb.w);
    s_stage[slot].c = gc;
    const float x0 = gx - gc.y, x1 = gx + gc.y, y0 = gy - gc.z, y1 = gy + gc.z;
    const bool xl = x0 <= 7.0f && x1 >= 0.0f, xr = x0 <= 15.0f && x1 >= 8.0f;
    const bool yt = y0 <= 7.0f && y1 >= 0.0f, yb = y0 <= 15.0f && y1 >= 8.0f;
    uint32_t qm = (uint32_t)(xl && yt) | ((uint32_t)(xr && yt) << 1) | ((uint32_t)(xl && yb) << 2) |
                  ((uint32_t)(xr && yb) << 3);
    if (exact) {
      // exact quadrant test (C2 0.0585 -> 0.0577 ms, bit-exact): the largest z over a quadrant's pixel
      // square (z concave: A, C < 0) is at the centre when the centre lies inside, else on an edge, each
      // edge's a clamped 1D parabola. A quadrant whose largest z is below log2(1/255) (minus a 0.02
      // margin for the rounding of the staged form) has no pixel with alpha >= 1/255: the entry would be
      // evaluated to nothing by every lane of its wave.
      // the vertex u* = -q / (2p) = q * (-1 / (2p)) (an approximate reciprocal: the value at a point near
      // the vertex is within the margin of the maximum)
      const float i2a = -0.5f * __builtin_amdgcn_rcpf(A), i2c = -0.5f * __builtin_amdgcn_rcpf(C);
      auto vmax = [](float p, float q, float r, float inv, float u0, float u1) {
        const float u = fminf(fmaxf(q * inv, u0), u1);
        return __builtin_fmaf(__builtin_fmaf(p, u, q), u, r);
      };
      const float zk = -7.9943534f - 0.02f;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float lo_x = (q & 1) ? 8.0f : 0.0f, lo_y = (q >> 1) ? 8.0f : 0.0f;
        const float hi_x = lo_x + 7.0f, hi_y = lo_y + 7.0f;
        const bool inside = gx >= lo_x && gx <= hi_x && gy >= lo_y && gy <= hi_y;
        // x = lo_x / hi_x over y in [lo_y, hi_y]; y = lo_y / hi_y over x in [lo_x, hi_x]
        const float m0 = vmax(C, __builtin_fmaf(B, lo_x, E), __builtin_fmaf(__builtin_fmaf(A, lo_x, D), lo_x, F), i2c, lo_y, hi_y);
        const float m1 = vmax(C, __builtin_fmaf(B, hi_x, E), __builtin_fmaf(__builtin_fmaf(A, hi_x, D), hi_x, F), i2c, lo_y, hi_y);
        const float m2 = vmax(A, __builtin_fmaf(B, lo_y, D), __builtin_fmaf(__builtin_fmaf(C, lo_y, E), lo_y, F), i2a, lo_x, hi_x);
        const float m3 = vmax(A, __builtin_fmaf(B, hi_y, D), __builtin_fmaf(__builtin_fmaf(C, hi_y, E), hi_y, F), i2a, lo_x, hi_x);
        const float m = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        if (!inside && !(m >= zk)) qm &= ~(1u << q);
      }
    }
    return qm;
  };
  // the tile's slot row is loaded together with its count (no dependent round trip for small tiles;
  // every work-item loads its slot whatever the count)
  const uint32_t srow = fu.scap ? fu.scap : GS_TILE_SLOTS;
  const unsigned long long k_slot = tile_slots[(size_t)tile * srow + tid];
  uint2 range;
  if (fu.scap) {
    const uint32_t c = fu.cursor[tile];
    range = make_uint2(tile * fu.scap, tile * fu.scap + c);
  } else {
    range = ranges[tile];
  }
  uint32_t n = range.y - range.x;
  STAMP_WAITED(1, 5);  // (the slot row and the count have arrived)
  const uint32_t n_front = n;  // (the front end's count: n becomes the completed count of a spilled tile)
  const bool small = slot_keys && n <= GS_BLOCK;
  if (fu.scap && tid == 0) fu.ranges[tile] = range;
  // a tile whose pairs were not all stored (fused: above its row's capacity; three launches: its
  // segment ends beyond the pair buffer) is gathered and sorted here: its sorted gaussians come from
  // the spill pool (nullptr: pool exhausted, the tile stays at the background; counted)
  const bool spilled = fu.scap ? n > fu.scap : (n > GS_TILE_SLOTS && range.y > cap);
  const uint32_t* vsrc = vals_out + range.x;
  if (spilled) {
    vsrc = gs_spill_tile(sp, tile_x, tile_y, n, s_arena);
    if (!vsrc) n = 0;
  }
  const bool mid = !small && !spilled && n <= sorted_above;  // not sorted by gs_sort_large_kernel: sorted here
  // publish (PTGS_FLAG_SPLAT_PUBLISH) only where the tile's range fits the buffers: a three-launch frame
  // above the pair buffer is re-run by the host after growing them (the published layout is that run's)
  const bool pub = keys_out && (fu.scap || range.y <= cap);
  const bool mid_lds = mid && n <= GS_MID;
  const unsigned long long tbits = (unsigned long long)tile << 32;
  float4 ra, rb, rc;     // records in flight: the unsorted keys' (small) / batch b + 1's (large)
  uint32_t g_next = 0;   // large tiles: gaussian of batch b + 2
  unsigned long long key = ~0ull;
  if (small && tid < n) {
    const unsigned long long k_cur = k_slot;
    const uint32_t g = (uint32_t)k_cur;
    if (GS_PROBE(GS_PROBE_NO_REC)) {
      ra = rb = rc = make_float4((float)g, 0.f, 0.f, 0.f);
    } else {
      ra = rec[3 * g];
      rb = rec[3 * g + 1];
      rc = rec[3 * g + 2];
    }
    key = (k_cur & 0xFFFFFFFF00000000ull) | ((unsigned long long)g << 8) | tid;  // g < 2^24 (slot_keys)
  }
  if (small) STAMP_WAITED(1, 6);  // (wave 0's records have arrived)
  if (small && n > GS_MERGE_MIN) {
    // merge ranking: the wave's sorted run in LDS, ranks by binary searches of the other runs; the
    // work-item holding a sorted key (its slot in the low 8 bits) records slot and published key
    const uint32_t m = (n + 63u) >> 6;  // runs holding keys (uniform)
    unsigned long long sk = ~0ull;
    if (wave < m) {
      sk = GS_PROBE(GS_PROBE_NO_MERGE) ? key : gs_wave_sort64(key, lane);
      s_key[tid] = sk;
    }
    __syncthreads();
    uint32_t r = GS_PROBE(GS_PROBE_NO_MERGE) ? tid : lane;
    if (wave < m && !GS_PROBE(GS_PROBE_NO_MERGE)) r += gs_runs_below<GS_BLOCK / 64>(s_key, m, wave, sk);
    __syncthreads();  // every read of the keys is done before records overwrite them
    if (tid < n) s_mask[tid] = (uint8_t)stage_rec(tid, ra, rb, rc, !GS_PROBE(GS_PROBE_NO_EXACT));
    if (sk != ~0ull) {
      if (pub) {
        keys_out[range.x + r] = tbits | (sk >> 32);
        vals_out[range.x + r] = (uint32_t)(sk >> 8) & 0xFFFFFFu;
      }
      s_sslot[r] = (uint8_t)(sk & 0xFFu);
    }
  } else if (small) {
    // rank counting (keys are unique): every work-item of a wave holding keys counts the keys below
    // its own over all n in LDS (uniform reads, eight keys per step, no barrier in the loop) and
    // records its staging slot at that rank
    s_key[tid] = key;  // ~0 above n
    __syncthreads();
    uint32_t r = GS_PROBE(GS_PROBE_NO_RANK) ? tid : 0u;
    if (wave * 64u < n && !GS_PROBE(GS_PROBE_NO_RANK)) {
      // four uniform reads in flight (entries n .. 255 hold ~0: never below a key)
      const uint32_t nu = (uint32_t)__builtin_amdgcn_readfirstlane((int)n);
      for (uint32_t j = 0; j < nu; j += 8) {
        const ulonglong2 x0 = *reinterpret_cast<const ulonglong2*>(s_key + j);
        const ulonglong2 x1 = *reinterpret_cast<const ulonglong2*>(s_key + j + 2);
        const ulonglong2 x2 = *reinterpret_cast<const ulonglong2*>(s_key + j + 4);
        const ulonglong2 x3 = *reinterpret_cast<const ulonglong2*>(s_key + j + 6);
        r += ((uint32_t)(x0.x < key) + (uint32_t)(x0.y < key)) + ((uint32_t)(x1.x < key) + (uint32_t)(x1.y < key)) +
             ((uint32_t)(x2.x < key) + (uint32_t)(x2.y < key)) + ((uint32_t)(x3.x < key) + (uint32_t)(x3.y < key));
      }
    }
    __syncthreads();  // every read of the keys is done before records overwrite them
    if (tid < n) {
      s_mask[tid] = (uint8_t)stage_rec(tid, ra, rb, rc, !GS_PROBE(GS_PROBE_NO_EXACT));
      if (pub) {
        keys_out[range.x + r] = tbits | (key >> 32);
        vals_out[range.x + r] = (uint32_t)(key >> 8) & 0xFFFFFFu;
      }
      s_sslot[r] = (uint8_t)tid;
    }
  } else {
    if (mid) {
      unsigned long long* seg = fu.scap ? const_cast<unsigned long long*>(tile_slots) + range.x
                              : n <= GS_TILE_SLOTS ? const_cast<unsigned long long*>(tile_slots) + (size_t)tile * GS_TILE_SLOTS
                                                   : pairs + range.x;
      if (mid_lds) {
        // merge ranking (above), two keys per work-item: wave w sorts runs w and w + 4 (slots tid and
        // tid + 256), then writes both keys to their ranks (keys are unique: the gaussian is in the
        // low word)
        unsigned long long k0 = tid < n ? seg[tid] : ~0ull;
        unsigned long long k1 = tid + GS_BLOCK < n ? seg[tid + GS_BLOCK] : ~0ull;
        const uint32_t m = (n + 63u) >> 6;  // runs holding keys: 5 .. 8 (uniform)
        k0 = gs_wave_sort64(k0, lane);
        if (wave + 4u < m) k1 = gs_wave_sort64(k1, lane);
        s_key[tid] = k0;
        s_key[tid + GS_BLOCK] = k1;
        __syncthreads();
        uint32_t r0 = lane, r1 = lane;
        for (uint32_t q = 0; q < m; ++q) {  // (8 runs in lockstep for two keys would spill at 64 VGPRs)
          const unsigned long long* run = s_key + 64u * q;
          if (q != wave) r0 += gs_run_below(run, k0);
          if (q != wave + 4u && wave + 4u < m) r1 += gs_run_below(run, k1);
        }
        __syncthreads();
        if (k0 != ~0ull) s_key[r0] = k0;  // (the slots below n hold exactly the keys other than ~0)
        if (k1 != ~0ull) s_key[r1] = k1;
        __syncthreads();
        if (pub)
          for (uint32_t k = tid; k < n; k += GS_BLOCK) {
            const unsigned long long v = s_key[k];
            keys_out[range.x + k] = tbits | (v >> 32);
            vals_out[range.x + k] = (uint32_t)v;
          }
      } else {  // beyond GS_MID without the sort kernel (a frame whose tiles outgrew the previous one's)
        bitonic_flip_sort(n, [&](uint32_t a, uint32_t b) {
          unsigned long long x = seg[a], y = seg[b];
          if (y < x) { seg[a] = y; seg[b] = x; }
        });
        for (uint32_t k = tid; k < n; k += GS_BLOCK) {
          const unsigned long long v = seg[k];
          if (pub) keys_out[range.x + k] = tbits | (v >> 32);
          vals_out[range.x + k] = (uint32_t)v;
        }
        __syncthreads();
      }
    }
    // sorted values (LDS for mid tiles, else vals_out): batch 0's records and batch 1's values in flight
    if (tid < n) {
      const uint32_t g = mid_lds ? (uint32_t)s_key[tid] : vsrc[tid];
      ra = rec[3 * g];
      rb = rec[3 * g + 1];
      rc = rec[3 * g + 2];
    }
    if (tid + GS_BLOCK < n) g_next = mid_lds ? (uint32_t)s_key[tid + GS_BLOCK] : vsrc[tid + GS_BLOCK];
  }
  if (tid == 0) {  // the null record (alpha 0) that pads the per-quadrant lists
    s_stage[GS_BLOCK].a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s_stage[GS_BLOCK].b = make_float4(0.0f, -__builtin_huge_valf(), 0.0f, 0.0f);
    s_stage[GS_BLOCK].c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  }

  const uint32_t px = tile_x * GS_BLOCK_X + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t py = tile_y * GS_BLOCK_Y + (wave >> 1) * 8u + (lane >> 3);
  const bool inside = px < cam.W && py < cam.H;
  // the wave's finished pixels as a lane mask in SGPRs (set: outside the image, saturated, or behind the mesh):
  // the per-entry validity and the every-4-entries all-done test read it without moving it into a VGPR
  unsigned long long done = __builtin_amdgcn_ballot_w64(!inside);
  const float pfx = (float)px, pfy = (float)py;
  const float ux = pfx - tx0, uy = pfy - ty0;
  const float lim = (OVER && inside) ? depth_lim[(size_t)py * cam.W + px] : 0.0f;
  float T = 1.0f;
  float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
  const char* stage = reinterpret_cast<const char*>(s_stage);
  int todo = (int)n;
  STAMP(1, 1);
  for (uint32_t base = 0; todo > 0; base += GS_BLOCK, todo -= GS_BLOCK) {
    // (small tiles: the barrier also publishes the records, masks and sorted slots staged after the
    // sort; large tiles: every wave is done with the previous batch.) The first batch: done = !inside,
    // and every tile holds a pixel inside the image: a plain barrier instead of the counting one, which
    // reduces through LDS behind a second barrier.
    if (base == 0) __syncthreads();
    else if (__syncthreads_count(__builtin_amdgcn_inverse_ballot_w64(done)) == GS_BLOCK) break;
    const uint32_t idx = base + tid;
    if (!small) {
      if (idx < n) {
        s_mask[tid] = (uint8_t)stage_rec(tid, ra, rb, rc, false);  // (large tiles: the box test only)
      }
      // next batch: its records (values loaded a batch ago) and the values of the one after
      if (idx + GS_BLOCK < n) {
        const uint32_t g = g_next;
        ra = rec[3 * g];
        rb = rec[3 * g + 1];
        rc = rec[3 * g + 2];
      }
      if (idx + 2 * GS_BLOCK < n) g_next = vsrc[idx + 2 * GS_BLOCK];
      __syncthreads();  // the batch's records and masks are staged
    }
    // each wave compacts its own quadrant's list from every staged mask, in sorted order (no
    // cross-wave counts: one barrier per batch fewer, two fewer for a small tile)
    const uint32_t nb = min((uint32_t)GS_BLOCK, n - base);
    const uint32_t nbu = (uint32_t)__builtin_amdgcn_readfirstlane((int)nb);
    uint32_t cnt = 0;
#pragma unroll
    for (uint32_t k = 0; k < GS_BLOCK / 64; ++k) {
      if (k * 64u >= nbu) break;  // (uniform: only the rounds that hold staged entries)
      const uint32_t p = k * 64u + lane;
      const uint32_t slot = small ? (uint32_t)s_sslot[p] : p;
      const bool bit = p < nb && ((s_mask[slot] >> wave) & 1u);
      const unsigned long long bal = __ballot(bit);
      if (bit)
        s_list[wave][cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] =
            slot * (uint32_t)sizeof(GStage);
      cnt += (uint32_t)__popcll(bal);
    }
    if (GS_PROBE(GS_PROBE_NO_EVAL)) cnt = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // wave-uniform trip count; the list is padded with the null Gaussian up to a multiple of 4
    const uint32_t cntu = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt);
    if (lane < 4) s_list[wave][cntu + lane] = GS_BLOCK * (uint32_t)sizeof(GStage);
    const uint32_t* list = s_list[wave];
    for (uint32_t j = 0; j < cntu; j += 4) {
      // (the all-done test every GS_DONE_EVERY entries: scalar, every lane of the wave is active here)
      if ((j & (GS_DONE_EVERY - 1u)) == 0u && done == __builtin_amdgcn_read_exec()) break;
      const uint4 o4 = *reinterpret_cast<const uint4*>(list + j);  // 4 list entries
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const uint32_t o = u == 0 ? o4.x : u == 1 ? o4.y : u == 2 ? o4.z : o4.w;
        const float4 a = *reinterpret_cast<const float4*>(stage + o);
        const float4 b = *reinterpret_cast<const float4*>(stage + o + 16);
        const float cb = *reinterpret_cast<const float*>(stage + o + 32);
        if (OVER) {  // sorted by depth: the first Gaussian at or behind the mesh ends the pixel
          const float gd = *reinterpret_cast<const float*>(stage + o + 44);
          done |= __builtin_amdgcn_ballot_w64(!(gd < lim));
        }
        // z = A dx^2 + B dx dy + C dy^2 + log2 o at (dx, dy) = pixel - mean, both tile-local: two subtractions,
        // two multiplies, three FMAs. (The reference's power > 0 skip is not tested: the conic is positive
        // definite (+0.3 low-pass), so power <= 0 up to rounding at power ~ 0.)
        const float dx = ux - a.w, dy = uy - b.x;
        const float z = __builtin_fmaf(__builtin_fmaf(a.x, dx, a.y * dy), dx, __builtin_fmaf(a.z * dy, dy, b.y));
        // alpha >= 1/255: z >= log2(1/255)
        const bool valid = __builtin_amdgcn_inverse_ballot_w64(__builtin_amdgcn_ballot_w64(z >= -7.9943534f) & ~done);
        const float alpha = valid ? fminf(0.99f, __builtin_amdgcn_exp2f(z)) : 0.0f;
        float wgt = alpha * T;
        float test_T = T - wgt;
        const unsigned long long term = __builtin_amdgcn_ballot_w64(test_T < 0.0001f);  // (only a valid pair)
        if (term) {  // rare: this Gaussian would saturate the pixel -> stop before it
          done |= term;
          const bool t = __builtin_amdgcn_inverse_ballot_w64(term);
          wgt = t ? 0.0f : wgt;
          test_T = t ? T : test_T;
        }
        C0 = __builtin_fmaf(b.z, wgt, C0);
        C1 = __builtin_fmaf(b.w, wgt, C1);
        C2 = __builtin_fmaf(cb, wgt, C2);
        T = test_T;
      }
    }
  }
  STAMP(1, 2);
  if (fu.scap && tid == 0 && n_front) fu.cursor[tile] = 0;  // (n > 0: every wave passed a barrier after reading it)
  if (inside) {
    // the pixel index is recomputed here from a laundered thread id, so that the one computed before
    // the batch loop is not kept (spilled) across it
    uint32_t t2 = tid;
    asm volatile("" : "+v"(t2));
    const uint32_t px2 = tile_x * GS_BLOCK_X + ((t2 >> 6) & 1u) * 8u + (t2 & 7u);
    const uint32_t py2 = tile_y * GS_BLOCK_Y + (t2 >> 7) * 8u + ((t2 & 63u) >> 3);
    const size_t pix = (size_t)py2 * cam.W + px2;
    if (OVER) {
      const float4 u4 = under[pix];
      gs_st4_nt(out + pix, make_float4(C0 + T * u4.x, C1 + T * u4.y, C2 + T * u4.z, (1.0f - T) + T * u4.w));
    } else {
      gs_st4_nt(out + pix, make_float4(C0 + T * bg_r, C1 + T * bg_g, C2 + T * bg_b, 1.0f - T));
    }
  }
  STAMP_SYNC();
  STAMP(1, 3);
}

// Published frame of the fused front end (PTGS_FLAG_SPLAT_PUBLISH, tests): the blend wrote each tile's
// sorted keys / values at t * scap; these two launches compact them into the three-launch layout
// (exclusive scan of the tile counts -> ranges, empty tiles (0, 0)) so both paths publish alike.
// Unpublished fused frames leave ranges[t] = (t * scap, t * scap + n): end - begin is the count.
#define GS_PUB_THREADS 1024
// (a spilled tile's count exceeds its row: only the row's scap keys are copied; a published frame with
// spilled tiles is re-run through the three-launch path by the host)
__global__ __launch_bounds__(GS_PUB_THREADS) void gs_publish_scan_kernel(const uint2* __restrict__ fr, uint32_t ntiles,
                                                                         uint32_t t_begin, uint32_t t_end, uint32_t scap,
                                                                         uint32_t* __restrict__ offs) {
  __shared__ uint32_t s_part[GS_PUB_THREADS / 64];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  const uint32_t per = (ntiles + GS_PUB_THREADS - 1) / GS_PUB_THREADS, a = tid * per, b = min(ntiles, a + per);
  uint32_t sum = 0;
  for (uint32_t t = a; t < b; ++t) sum += (t >= t_begin && t < t_end) ? min(scap, fr[t].y - fr[t].x) : 0u;
  const uint32_t incl = wave_incl_scan(sum);
  if (lane == 63) s_part[wv] = incl;
  __syncthreads();
  uint32_t run = incl - sum;
  for (uint32_t w = 0; w < wv; ++w) run += s_part[w];
  for (uint32_t t = a; t < b; ++t) {
    offs[t] = run;
    run += (t >= t_begin && t < t_end) ? min(scap, fr[t].y - fr[t].x) : 0u;
  }
}

__global__ __launch_bounds__(256) void gs_publish_copy_kernel(const uint2* __restrict__ fr, const uint32_t* __restrict__ offs,
                                                              uint32_t t_begin, uint32_t t_end, uint32_t scap,
                                                              const unsigned long long* __restrict__ keys_in,
                                                              const uint32_t* __restrict__ vals_in,
                                                              unsigned long long* __restrict__ keys_out,
                                                              uint32_t* __restrict__ vals_out, uint2* __restrict__ ranges) {
  const uint32_t t = blockIdx.x;
  const bool in = t >= t_begin && t < t_end;
  const uint2 r = in ? fr[t] : make_uint2(0u, 0u);
  const uint32_t n = min(scap, r.y - r.x), o = offs[t];
  __syncthreads();  // (ranges may be fr itself: every work-item has read fr[t])
  if (threadIdx.x == 0) ranges[t] = n ? make_uint2(o, o + n) : make_uint2(0u, 0u);
  for (uint32_t k = threadIdx.x; k < n; k += 256) {
    keys_out[o + k] = keys_in[r.x + k];
    vals_out[o + k] = vals_in[r.x + k];
  }
}

}  // namespace ptgs
