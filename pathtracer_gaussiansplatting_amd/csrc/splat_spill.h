// splat_spill.h — stage: a tile whose pairs the front end could not all store, completed by its own blend
// workgroup through the spill pool. Called by gs_sort_blend_kernel (splat_blend.h), whose LDS arena it
// borrows. Relies on the counter words (splat_words.h), bitonic_flip_sort (splat_wave.h) and GS_BLOCK
// (splat_plan.h).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "splat_plan.h"
#include "splat_wave.h"
#include "splat_words.h"

namespace ptgs {

// ---- spilled tiles --------------------------------------------------------------------------------
// A tile whose pairs the front end could not all store (fused: more than its row's scap pairs, e.g.
// the camera moved closer than the previous frame that sized the rows; three launches: a segment that
// ends beyond the pair buffer sized from earlier frames) is completed by its own blend workgroup, in
// the same launch: the front-end workgroups whose bounding rect (crect) holds the tile are listed,
// their Gaussians' stored rects tested against the tile, and the keys (depth << 32 | gaussian, the
// front ends' keys) collected; then sorted (bitonic: in the LDS arena up to GS_SPILL_LDS keys, else in
// the pool) and the sorted gaussians written to the spill pool, from which the blend streams them like
// a large tile's. Same keys, same order, same blend: the image equals a frame whose rows had fit (and
// the oracle's). The pool (cap pairs per workspace) is reserved per tile with one atomic (GS_FZ_POOL_CURSOR,
// re-armed by the next frame's front end, which also hands the demand to the host to size the pool); a tile
// that does not fit is left at the background and counted (GS_FZ_INCOMPLETE; GS_KH_INCOMPLETE <- 1: the next
// call reports it).
struct GsSpill {
  uint32_t* fz;                   // device counters: GS_FZ_POOL_CURSOR, GS_FZ_SPILLED, GS_FZ_INCOMPLETE
  uint32_t* k_host;               // pinned host words: GS_KH_INCOMPLETE
  unsigned long long* keys;       // pool: keys of tiles above GS_SPILL_LDS pairs
  uint32_t* vals;                 // pool: sorted gaussians of every spilled tile
  uint32_t cap;                   // pool capacity (pairs)
  const ushort4* crect;           // per front-end workgroup (chunk c of band b at c * bands + b): rect of its pairs
  uint32_t nwg, bands, chunk, n;  // front-end workgroups, bands, Gaussians per chunk, Gaussians
  const ushort4* rects;           // per Gaussian (walk order): tile rect (empty: culled)
  const float* depths;            // per Gaussian (walk order): view depth
  const uint32_t* ids;            // the caller's index (NULL: the walk index)
};
#define GS_SPILL_LDS 1984u  // keys sorted in the blend's LDS arena (15 872 B + the candidate list + counters)
#define GS_SPILL_CAND 128u  // front-end workgroups tested per round

// Returns the sorted gaussians of tile (tx, ty) in the pool and their count in m (on entry: the
// tile's pair count), or nullptr when the pool is exhausted. Uses the arena (>= 16 400 B of LDS).
__device__ const uint32_t* gs_spill_tile(const GsSpill& sp, uint32_t tx, uint32_t ty, uint32_t& m, char* arena) {
  const uint32_t tid = threadIdx.x, n = m;
  unsigned long long* s_k = reinterpret_cast<unsigned long long*>(arena);
  uint32_t* s_c = reinterpret_cast<uint32_t*>(arena + 8 * GS_SPILL_LDS);
  uint32_t* s_w = s_c + GS_SPILL_CAND;  // [0] keys found, [1] pool offset, [2] candidates of the round
  const bool lds = n <= GS_SPILL_LDS;
  if (tid == 0) {
    s_w[0] = 0;
    s_w[2] = 0;
    uint32_t off = atomicAdd(sp.fz + GS_FZ_POOL_CURSOR, n);
    atomicAdd(sp.fz + GS_FZ_SPILLED, 1u);
    if (off > sp.cap || n > sp.cap - off) {
      off = 0xFFFFFFFFu;
      atomicAdd(sp.fz + GS_FZ_INCOMPLETE, 1u);
      __atomic_store_n(sp.k_host + GS_KH_INCOMPLETE, 1u, __ATOMIC_RELAXED);
      __threadfence_system();
    }
    s_w[1] = off;
  }
  __syncthreads();
  const uint32_t off = s_w[1];
  if (off == 0xFFFFFFFFu) return nullptr;
  unsigned long long* gk = sp.keys + off;
  for (uint32_t w0 = 0; w0 < sp.nwg; w0 += GS_SPILL_CAND) {
    if (tid < GS_SPILL_CAND && w0 + tid < sp.nwg) {
      const ushort4 r = sp.crect[w0 + tid];
      if (r.x <= tx && tx < r.z && r.y <= ty && ty < r.w) s_c[atomicAdd(s_w + 2, 1u)] = w0 + tid;
    }
    __syncthreads();
    const uint32_t nc = s_w[2];
    for (uint32_t k = 0; k < nc; ++k) {
      const uint32_t c = s_c[k] / sp.bands;
      const uint32_t g0 = c * sp.chunk, g1 = min(sp.n, g0 + sp.chunk);
      for (uint32_t i = g0 + tid; i < g1; i += GS_BLOCK) {
        const ushort4 r = sp.rects[i];
        if (r.x <= tx && tx < r.z && r.y <= ty && ty < r.w) {
          const unsigned long long key =
              ((unsigned long long)__float_as_uint(sp.depths[i]) << 32) | (sp.ids ? sp.ids[i] : i);
          const uint32_t p = atomicAdd(s_w, 1u);
          if (p < n) {
            if (lds) s_k[p] = key;
            else gk[p] = key;
          }
        }
      }
    }
    __syncthreads();
    if (tid == 0) s_w[2] = 0;
    __syncthreads();
  }
  m = min(s_w[0], n);  // (= n: the rects are the ones the front end counted)
  const uint32_t mm = m;
  if (lds) {
    bitonic_flip_sort(mm, [&](uint32_t a, uint32_t b) {
      const unsigned long long x = s_k[a], y = s_k[b];
      if (y < x) { s_k[a] = y; s_k[b] = x; }
    });
    for (uint32_t k = tid; k < mm; k += GS_BLOCK) sp.vals[off + k] = (uint32_t)s_k[k];
  } else {
    bitonic_flip_sort(mm, [&](uint32_t a, uint32_t b) {
      const unsigned long long x = gk[a], y = gk[b];
      if (y < x) { gk[a] = y; gk[b] = x; }
    });
    for (uint32_t k = tid; k < mm; k += GS_BLOCK) sp.vals[off + k] = (uint32_t)gk[k];
  }
  __syncthreads();  // the values (and the arena's last reads) before the blend stages records over them
  return sp.vals + off;
}

}  // namespace ptgs
