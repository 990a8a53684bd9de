// splat_fused.h — stage: the fused front end (preprocess, count, reserve and scatter in one launch over
// fixed-capacity tile rows) and GsFused, the later stages' view of such a frame. Relies on the walks, the
// tile order and the spill re-arm of splat_bin.h, gs_preprocess_one (splat_preprocess.h), GsFusedShape
// (splat_plan.h), the counter words (splat_words.h) and the wave primitives (splat_wave.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "splat_bin.h"
#include "splat_plan.h"
#include "splat_preprocess.h"
#include "splat_probe.h"
#include "splat_wave.h"
#include "splat_words.h"

namespace ptgs {

// ---- fused front end ------------------------------------------------------------------------------
// One launch instead of count + colscan + scatter: per-tile slot rows of a fixed capacity `scap`
// (a power of two >= the largest tile of recent frames) replace the exact tile segments, so a tile's
// pairs need no global prefix: block (band, c) preprocesses chunk c (one Gaussian per work-item,
// kept in registers), counts its pairs per tile in LDS, reserves each touched tile's run with one
// returning atomicAdd on the tile's cursor, then walks its pairs again and writes each key to
// tile_slots[t * scap + base + LDS rank]. The order inside a row depends on the atomics' order and is
// fixed by the per-tile sort (keys are unique), so keys / values / image equal the three-launch path.
// The blend reads the tile's count from its cursor and zeroes it (cursors are zero between frames).
// A tile whose count exceeds scap keeps its first scap keys only: the blend renders it through
// gs_spill_tile (its pairs gathered again from the per-Gaussian rects / depths band 0 stores here and
// the per-workgroup chunk rects), so the frame is complete; the next frame sizes its rows from it.
// Counters: fz (GS_FZ_MAX_TILE, GS_FZ_ABOVE_MID, GS_FZ_OVER_SCAP) and per workgroup fzp: (pairs,
// reservations); published to the host by the blend's block (0, 0).
// (GS_FUSED_OWN_CULL, GS_FUSED_THREADS, GS_FUSED_WG, GS_FUSED_WG_OV, GsFusedShape: splat_plan.h)
struct GsFused {  // the sort's and the blend's view of a fused-front-end frame (scap == 0: three-launch path)
  uint32_t scap;
  uint32_t* cursor;   // per-tile pair counts (zeroed again by the blend)
  uint32_t* fz;       // counters (GsFzWord)
  uint32_t* k_host;   // pinned host words (GsHostWord; published by blend block (0, 0))
  uint2* ranges;      // the tile ranges the blend writes (t * scap, t * scap + n)
  uint32_t* fzp;      // per front-end workgroup: (pairs, reservations)
  uint32_t nwg;
  const uint32_t* order;  // blend workgroup -> tile (heavy tiles first; null: row-major)
  uint2* fsq;             // the front end's slice queue (re-armed by block (0, 0): entries and GS_FZ_Q_*)
  uint32_t fsq_cap;
  unsigned long long* seq_flag;  // frames in flight: the blend's first workgroup stores `seq` here (SplatSeq)
  unsigned long long seq;
};

// The count walk of one slice [p0, p1) of a chunk's pairs (at most GS_FUSED_QREG per work-item): the
// chunk's rects (s_e: x0 | w << 16, y0 | h << 16, key index, depth bits) and the inclusive scan of
// their areas (s_incl) are in LDS; work-item t takes the contiguous pairs [p0 + t q, p0 + t q + q)
// (q = ceil((p1 - p0) / WG)): one binary search for its first pair, then it steps through the
// rects (a heavy Gaussian's pairs are spread over the whole workgroup instead of one wave). Returning
// LDS atomics give each pair its rank among the slice's pairs of its tile, kept in registers with the
// pair, packed as k | rank << 13 | j << 21 (k: tile in the chunk's rect, < 8192 = GS_BAND_TILES; rank
// < 256: one pair per Gaussian and tile; j: Gaussian in the chunk, < 256). The scatter then writes each
// kept pair at its run's base + rank without walking the rects again or touching an LDS atomic.
// Returns the work-item's pair count.
#ifndef GS_FUSED_QREG
#define GS_FUSED_QREG 8  // pairs per work-item of a slice (GsFusedShape<WG>::slice / WG; C2 needs <= 7)
#endif
#define GS_KEEP_RB (GS_FUSED_THREADS <= 256 ? 8u : 9u)  // bits of rank and of j (< GS_FUSED_THREADS)
static_assert(GS_FUSED_THREADS <= 512 && GS_BAND_TILES <= 8192, "gs_wg_count_keep's packing");
#define GS_PK_NONE 0xFFFFFFFFu  // a walked pair outside the histogram window (kept by another window's walk)
template <uint32_t WG>
__device__ __forceinline__ uint32_t gs_wg_count_keep(const uint32_t* s_incl, const uint4* s_e, uint32_t ng, uint32_t p0,
                                                     uint32_t p1, uint32_t* s_hist, uint32_t bx0, uint32_t by0,
                                                     uint32_t rw, uint32_t kw, uint32_t kcap,
                                                     uint32_t (&pk)[GS_FUSED_QREG]) {
  const uint32_t q = (p1 - p0 + WG - 1) / WG;
  uint32_t p = p0 + threadIdx.x * q;
  const uint32_t pe = min(p1, p + q);
  if (p >= pe) return 0;
  const uint32_t cnt = pe - p;
  uint32_t lo = 0, hi = ng - 1;  // first j with incl[j] > p
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (s_incl[mid] > p) hi = mid;
    else lo = mid + 1;
  }
  uint32_t j = lo;
  uint4 e = s_e[j];
  uint32_t w = e.x >> 16, r = p - (s_incl[j] - w * (e.y >> 16));
  uint32_t ry = r / w, rx = r - ry * w;
#pragma unroll
  for (uint32_t c = 0; c < GS_FUSED_QREG; ++c) {
    if (c < cnt) {
      // (the tile's index in the rect, relative to the histogram window [kw, kw + kcap))
      const uint32_t k = ((e.y & 0xFFFFu) + ry - by0) * rw + ((e.x & 0xFFFFu) + rx - bx0) - kw;
      if (k < kcap) {
        const uint32_t rank = atomicAdd(s_hist + k, 1u);
        pk[c] = k | (rank << 13) | (j << (13u + GS_KEEP_RB));
      } else {
        pk[c] = GS_PK_NONE;
      }
      if (c + 1 < cnt && ++rx == w) {
        rx = 0;
        if (++ry == (e.y >> 16)) {  // next rect with pairs
          do {
            e = s_e[++j];
          } while ((e.y >> 16) == 0u || (e.x >> 16) == 0u);
          w = e.x >> 16;
          ry = 0;
        }
      }
    }
  }
  return cnt;
}

// Load balance. A chunk's pairs are walked in slices of at most GsFusedShape<WG>::slice pairs. The owner (the
// chunk's workgroup) walks slice 0 and publishes the others to a queue (fsq, entries (owner + 1, j));
// helper workgroups (the rows after the owners) claim queued slices, rebuild the chunk's rects (the
// same preprocess, no stores) and walk them: every (slice, tile) run reserves its own range, so a
// chunk that holds many times the mean pairs (Gaussians close to a moving camera) no longer sets the
// kernel's length alone. After its slice 0 an owner claims its own still-queued slices (it never
// waits), so no slice depends on a helper: a helper waits only for owners that have not published yet
// (owners precede helpers in dispatch order), and gives up after ~100 us (a slice it would have taken
// is then its owner's). Queue words: GS_FZ_Q_CLAIMS (helpers), GS_FZ_Q_ENTRIES, GS_FZ_Q_OWNERS (done);
// entries are 0 (not written), owner + 1 (open), GS_FSQ_TAKEN; the blend's block (0, 0) re-arms them.
// (GS_FUSED_HELPERS, helper workgroups per band, one queued slice each: splat_plan.h)
#define GS_FSQ_TAKEN 0xFFFFFFFFu
// waves per SIMD: 512 work-items 6 (3 workgroups per CU; 8 forced SGPR spills), 256 work-items 8 (64 VGPRs)
#define GS_FUSED_WAVES(WG) ((WG) == 512 ? 6 : 8)
static_assert(GsFusedShape<512>::slice <= 512u * GS_FUSED_QREG && GsFusedShape<256>::slice <= 256u * GS_FUSED_QREG,
              "a slice's pairs are kept in registers");
// chunk skip flags (cskip) and chunk bounds are per 256 Gaussians (ptgs_gaussians_chunk_bounds): the fused
// workgroups index them by their own chunk, so a fused chunk must be exactly that
static_assert(GS_FUSED_THREADS == 256, "the fused chunk is the chunk-bounds granule (256 Gaussians)");


template <bool ROWCULL, uint32_t WG>
__global__ __launch_bounds__(WG, GS_FUSED_WAVES(WG)) void gs_bin_fused_kernel(SplatCam cam, PreArgs A, BinGrid bg,
                                                                         uint32_t scap,
                                                                         uint32_t* __restrict__ cursor,
                                                                         uint32_t* __restrict__ fz,
                                                                         uint32_t* __restrict__ fzp,
                                                                         unsigned long long* __restrict__ tile_slots,
                                                                         const uint2* __restrict__ prev_ranges,
                                                                         uint32_t* __restrict__ order,
                                                                         uint32_t order_tb, uint32_t order_te,
                                                                         ushort4* __restrict__ crect,
                                                                         ushort4* __restrict__ rects_out,
                                                                         float* __restrict__ depths_out,
                                                                         uint32_t* k_host, uint2* __restrict__ fsq,
                                                                         uint32_t fsq_cap, uint32_t kcap) {
  // the histogram window: kcap entries (<= band_rows * grid_x); a chunk whose bounding tile rect holds
  // more tiles walks its slice once per window of kcap tiles (each walk counts, reserves and scatters
  // only its window's pairs), so the dynamic LDS need not cover a whole band
  extern __shared__ __attribute__((aligned(16))) uint32_t s_hist[];
  __shared__ uint32_t s_red[4][WG / 64];
  __shared__ uint32_t s_tot[WG / 64];
  __shared__ uint32_t s_incl[GS_FUSED_THREADS];
  __shared__ uint4 s_e[GS_FUSED_THREADS];
  __shared__ uint32_t s_job[4];  // helpers: (owner, slice) claimed; owners: queue base of their slices
  static_assert(GS_FUSED_THREADS >= GS_ORDER_BUCKETS, "gs_tile_order's buckets live in s_incl");
  if (order && blockIdx.y == gridDim.y - 1) {  // the extra row of blocks: the blend's tile order
    if (blockIdx.x == 0) {
      STAMP(0, 0);
      gs_tile_order(prev_ranges, order, order_tb, order_te, s_incl);
      STAMP_SYNC();
      STAMP(0, 5);
    }
    return;
  }
  STAMP(0, 0);
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t nown = bg.chunks * gridDim.x;  // owner workgroups
  const bool owner = blockIdx.y < bg.chunks;
  if (owner && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) gs_spill_rearm(fz, k_host);
  uint32_t acc_pairs = 0, acc_res = 0;  // this workgroup's reservations over all its slices (per work-item)
  uint32_t wg = blockIdx.y * gridDim.x + blockIdx.x;  // the owner whose chunk is processed
  uint32_t slice = 0;
  {  // helpers claim one queued slice (one per helper: no loop keeps the camera's registers live)
    if (!owner) {
      if (threadIdx.x == 0) {
        // (owner, slice) in two words: an owner index is bands x chunks, beyond any packing's bits at 8K
        // with tens of millions of Gaussians
        uint32_t job = 0xFFFFFFFFu, jslice = 0, hidx = 0, spins = 0;
        for (;;) {
          if (!hidx) hidx = atomicAdd(fz + GS_FZ_Q_CLAIMS, 1u) + 1u;  // (1-based: 0 = none claimed)
          const uint32_t idx = hidx - 1u;
          if (idx >= fsq_cap) break;
          // (the entry as one 64-bit word: owner + 1 and slice arrive together, no fence needed)
          const unsigned long long ev = __hip_atomic_load(reinterpret_cast<unsigned long long*>(fsq + idx),
                                                          __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const uint32_t v = (uint32_t)ev;
          if (v == 0u) {  // not written yet: done when every owner has published and this index is past the end
            const uint32_t done = __hip_atomic_load(fz + GS_FZ_Q_OWNERS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const uint32_t tail = __hip_atomic_load(fz + GS_FZ_Q_ENTRIES, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((done >= nown && idx >= tail) || ++spins > 200u) break;
            // (a few hundred helpers polling: every ~3 us, or their loads crowd out the owners' memory
            // traffic; measured 3x slower owner phases at ~0.05 us per poll)
            __builtin_amdgcn_s_sleep(127);
            continue;
          }
          hidx = 0;  // this index is settled: the next iteration claims another
          if (v != GS_FSQ_TAKEN && atomicCAS(&fsq[idx].x, v, GS_FSQ_TAKEN) == v) {
            job = v - 1u;
            jslice = (uint32_t)(ev >> 32);
            break;
          }
        }
        s_job[0] = job;
        s_job[3] = jslice;
      }
      __syncthreads();
      const uint32_t job = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_job[0]);
      if (job == 0xFFFFFFFFu) {
        if (threadIdx.x == 0) {
          const uint32_t fw = blockIdx.y * gridDim.x + blockIdx.x;
          fzp[2 * fw] = 0;
          fzp[2 * fw + 1] = 0;
        }
        return;
      }
      wg = job;
      slice = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_job[3]);
    }
    const uint32_t band = wg % gridDim.x, chunk = wg / gridDim.x;
    const uint32_t ty0 = bg.row0 + band * bg.band_rows, ty1 = min(bg.row1, ty0 + bg.band_rows);
    const uint32_t i = chunk * bg.chunk + threadIdx.x;  // chunk <= GS_FUSED_THREADS (host)
    const bool own = threadIdx.x < bg.chunk && i < A.n;
    const bool store = owner && band == 0;
    ushort4 rc = make_ushort4(0, 0, 0, 0);
    const uint32_t o = own && A.ids ? A.ids[i] : i;  // the key's index (the caller's)
    float d = 0.0f;  // view depth (every band's blocks need it for the keys; only band 0 stores it)
    // (tile-row shard with chunk bounds: a chunk whose bound misses the rows is skipped before its
    // Gaussians are loaded; it goes through the rest with no pairs)
    const bool skip = cam.cull && (A.cbounds ? gs_chunk_misses(cam, A.cbounds[2 * chunk], A.cbounds[2 * chunk + 1])
                                             : A.cskip[chunk] != 0);
    if (owner && skip) {
      // a culled chunk leaves at once (a tile-row shard of a large set culls most of its ~N / 256
      // workgroups): what it owes is the empty chunk rect (gs_spill_tile then never reads its Gaussians),
      // its published zeros, its arrival at the slice queue's owner count and zero partials
      if (own && store) gs_store_skipped(A, i);
      if (threadIdx.x == 0) {
        crect[wg] = make_ushort4(1, 1, 0, 0);
        atomicAdd(fz + GS_FZ_Q_OWNERS, 1u);
        fzp[2 * wg] = 0;
        fzp[2 * wg + 1] = 0;
      }
      return;
    }
    if (own && !skip)
      rc = store ? gs_preprocess_one<true, ROWCULL>(cam, A, i, &d) : gs_preprocess_one<false, ROWCULL>(cam, A, i, &d);
    else if (own && store) gs_store_skipped(A, i);
    if (own && store) {  // for gs_spill_tile: the rect (empty: culled) and depth in walk order
      rects_out[i] = rc;
      depths_out[i] = d;
    }
    STAMP_WAITED(0, 6);  // (wave 0's preprocess, loads included)
    uint32_t xw, yh;
    gs_clip(rc, ty0, ty1, xw, yh);
    // the chunk's bounding tile rect (within the band): the LDS histogram covers only it, so zeroing
    // and the reservation scan touch ~100 entries for a spatially coherent chunk instead of the band's
    uint32_t bx0 = 0xFFFFu, by0 = 0xFFFFu, bx1 = 0u, by1 = 0u;
    if (yh) {
      bx0 = xw & 0xFFFFu;
      bx1 = bx0 + (xw >> 16);
      by0 = yh & 0xFFFFu;
      by1 = by0 + (yh >> 16);
    }
    bx0 = wave_reduce<0>(bx0);
    by0 = wave_reduce<0>(by0);
    bx1 = wave_reduce<1>(bx1);
    by1 = wave_reduce<1>(by1);
    // the rects and the inclusive scan of their areas for the workgroup walk: the per-wave partials of
    // both (rect bounds, area totals) meet behind one barrier
    const uint32_t area = yh ? (xw >> 16) * (yh >> 16) : 0u;
    const uint32_t incl = wave_incl_scan(area);
    if (lane == 0) {
      s_red[0][wave] = bx0;
      s_red[1][wave] = by0;
      s_red[2][wave] = bx1;
      s_red[3][wave] = by1;
    }
    if (lane == 63) s_tot[wave] = incl;
    if (threadIdx.x < GS_FUSED_THREADS) s_e[threadIdx.x] = make_uint4(xw, yh, o, __float_as_uint(d));
    __syncthreads();
    STAMP(0, 7);
    uint32_t run = incl, P = 0;
#pragma unroll
    for (uint32_t w = 0; w < WG / 64; ++w) {
      bx0 = min(bx0, s_red[0][w]);
      by0 = min(by0, s_red[1][w]);
      bx1 = max(bx1, s_red[2][w]);
      by1 = max(by1, s_red[3][w]);
      const uint32_t tw = s_tot[w];
      run += w < wave ? tw : 0u;
      P += tw;
    }
    if (threadIdx.x < GS_FUSED_THREADS) s_incl[threadIdx.x] = run;
    // (uniform: in SGPRs, the registers the slice loop keeps)
    bx0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bx0);
    by0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)by0);
    bx1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)bx1);
    by1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)by1);
    P = (uint32_t)__builtin_amdgcn_readfirstlane((int)P);
    const uint32_t rw = bx1 > bx0 ? bx1 - bx0 : 0u, rh = by1 > by0 ? by1 - by0 : 0u, nt = rw * rh;
    const uint32_t nsl = (P + GsFusedShape<WG>::slice - 1u) / GsFusedShape<WG>::slice;  // slices of this chunk (uniform)
    if (owner) {
      if (threadIdx.x == 0) {  // the workgroup's bounding rect (gs_spill_tile; empty: x0 > x1)
        crect[wg] = nt ? make_ushort4((unsigned short)bx0, (unsigned short)by0, (unsigned short)bx1, (unsigned short)by1)
                       : make_ushort4(1, 1, 0, 0);
        // slices 1.. go to the queue (none fit: the owner walks them all itself)
        uint32_t qb = 0xFFFFFFFFu;
        if (nsl > 1u) {
          qb = atomicAdd(fz + GS_FZ_Q_ENTRIES, nsl - 1u);
          if (qb + (nsl - 1u) > fsq_cap) {  // (the part inside the queue is marked taken: helpers skip it)
            for (uint32_t k = qb; k < fsq_cap && k < qb + (nsl - 1u); ++k)
              __hip_atomic_store(reinterpret_cast<unsigned long long*>(fsq + k), (unsigned long long)GS_FSQ_TAKEN,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            qb = 0xFFFFFFFFu;
          } else {
            for (uint32_t j = 1; j < nsl; ++j)
              __hip_atomic_store(reinterpret_cast<unsigned long long*>(fsq + qb + j - 1u),
                                 ((unsigned long long)j << 32) | (wg + 1u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
        // published (helpers stop waiting once every owner has; no release fence: an agent-scope one
        // writes back the XCD's L2. A helper that sees every owner done before it sees its entry keeps
        // waiting while its index is below the tail; one that leaves early leaves the slice to its owner)
        atomicAdd(fz + GS_FZ_Q_OWNERS, 1u);
        s_job[1] = qb;
      }
    }
    // the slices this pass walks: helpers one; owners slice 0, then each queued slice it can still
    // claim (or every slice when the queue was full)
    for (;;) {
      const uint32_t p0 = slice * GsFusedShape<WG>::slice, p1 = min(P, p0 + GsFusedShape<WG>::slice);
     for (uint32_t kw = 0; kw < nt; kw += kcap) {  // histogram windows of the rect (one for most chunks)
      const uint32_t nw = min(kcap, nt - kw);
      if (kw) __syncthreads();  // (the previous window's scatter has read s_hist)
      for (uint32_t k = threadIdx.x; k < nw; k += WG) s_hist[k] = 0;
      __syncthreads();  // (the scan and the zeroed histogram)
      STAMP(0, 1);
      STAMP_SYNC();
      STAMP(0, 2);
      uint32_t pk[GS_FUSED_QREG];
      const uint32_t kept =
          p1 > p0 ? gs_wg_count_keep<WG>(s_incl, s_e, GS_FUSED_THREADS, p0, p1, s_hist, bx0, by0, rw, kw, kcap, pk) : 0u;
      __syncthreads();
      STAMP(0, 3);
      // reserve: one returning atomic per touched tile (all of a work-item's issued before any is
      // used); the LDS entry becomes the run's base
      const float rcp_rw = 1.0f / (float)max(rw, 1u);
      for (uint32_t k0 = threadIdx.x; k0 < nw; k0 += 4 * WG) {
        uint32_t c[4], t[4], base[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t kl = k0 + j * WG, k = kw + kl;
          c[j] = kl < nw ? s_hist[kl] : 0u;
          uint32_t ry = (uint32_t)((float)k * rcp_rw);  // k < 2^13 * 2^13: exact after the fix-ups
          ry = ry * rw > k ? ry - 1 : ry;
          ry = (ry + 1) * rw <= k ? ry + 1 : ry;
          t[j] = (by0 + ry) * bg.grid_x + bx0 + (k - ry * rw);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) base[j] = c[j] ? atomicAdd(cursor + t[j], c[j]) : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (!c[j]) continue;
          s_hist[k0 + j * WG] = base[j];
          acc_pairs += c[j];
          ++acc_res;
          if (base[j] <= scap && base[j] + c[j] > scap) atomicAdd(fz + GS_FZ_OVER_SCAP, 1u);  // (one crossing per spilled tile)
          if (base[j] + c[j] > 256u) {
            atomicMax(fz + GS_FZ_MAX_TILE, base[j] + c[j]);
            if (base[j] <= GS_MID && base[j] + c[j] > GS_MID) atomicAdd(fz + GS_FZ_ABOVE_MID, 1u);  // (one crossing per tile)
          }
        }
      }
      __syncthreads();  // every run's base is in s_hist
      STAMP(0, 4);
#pragma unroll
      for (uint32_t c = 0; c < GS_FUSED_QREG; ++c) {
        if (c < kept && pk[c] != GS_PK_NONE) {
          const uint32_t kl = pk[c] & 0x1FFFu, k = kw + kl;
          const uint32_t rel = s_hist[kl] + ((pk[c] >> 13) & ((1u << GS_KEEP_RB) - 1u));
          const uint4 e = s_e[pk[c] >> (13u + GS_KEEP_RB)];
          uint32_t ry = (uint32_t)((float)k * rcp_rw);  // k < 2^13: exact after the fix-ups
          ry = ry * rw > k ? ry - 1 : ry;
          ry = (ry + 1) * rw <= k ? ry + 1 : ry;
          const uint32_t t = (by0 + ry) * bg.grid_x + bx0 + (k - ry * rw);
          if (rel < scap) {
            const unsigned long long key = ((unsigned long long)e.w << 32) | e.z;
            tile_slots[(size_t)t * scap + rel] = key;
          }
        }
      }
     }  // (windows)
      if (!owner) break;
      // owner: the next of its slices that no helper has taken (uniform through LDS)
      __syncthreads();  // (every read of s_hist / s_job before they change)
      if (threadIdx.x == 0) {
        const uint32_t qb = s_job[1];
        uint32_t next = 0xFFFFFFFFu;
        for (uint32_t j = slice + 1; j < nsl; ++j) {
          if (qb == 0xFFFFFFFFu) {  // queue full: all of them here
            next = j;
            break;
          }
          if (atomicCAS(&fsq[qb + j - 1u].x, wg + 1u, GS_FSQ_TAKEN) == wg + 1u) {
            next = j;
            break;
          }
        }
        s_job[2] = next;
      }
      __syncthreads();
      const uint32_t next = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_job[2]);
      if (next == 0xFFFFFFFFu) break;
      slice = next;
    }
  }
  acc_pairs = wave_reduce<2>(acc_pairs);
  acc_res = wave_reduce<2>(acc_res);
  __syncthreads();
  if (lane == 0) {
    s_red[0][wave] = acc_pairs;
    s_red[1][wave] = acc_res;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // per-workgroup partials (the blend's block (0, 0) sums them: no fan-in atomics)
    uint32_t p = 0, r = 0;
    for (uint32_t w = 0; w < WG / 64; ++w) {
      p += s_red[0][w];
      r += s_red[1][w];
    }
    const uint32_t fw = blockIdx.y * gridDim.x + blockIdx.x;
    fzp[2 * fw] = p;
    fzp[2 * fw + 1] = r;
  }
  STAMP_SYNC();
  STAMP(0, 5);
}

}  // namespace ptgs
