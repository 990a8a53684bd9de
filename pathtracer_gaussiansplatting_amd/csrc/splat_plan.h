// splat_plan.h — the host's planning rules of the 3DGS forward pass (splat.hip): plain values in, plain
// values out. No HIP include: tests/native/splat_plan_check.cpp builds it with a host compiler alone. The
// racy mailbox hints a rule depends on (splat_words.h, GsHostWord) are arguments, read by the caller at the
// point of the frame call where the rule applies.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace ptgs {

#define GS_BLOCK_X 16
#define GS_BLOCK_Y 16
#define GS_BLOCK (GS_BLOCK_X * GS_BLOCK_Y)

// ---- static limits of the kernels ------------------------------------------------------------------
#define GS_MAX_CHUNKS 1024   // colscan: 16 waves x up to 64 chunks each
#ifndef GS_CHUNK_MIN
#define GS_CHUNK_MIN 512     // Gaussians per chunk (at least)
#endif
#define GS_BAND_TILES 8192   // max tiles per band (LDS: 32 KiB count, 64 KiB scatter); W <= 131072 px
#define GS_TILE_SLOTS 256    // fixed key slots per tile (= the register-sort limit)
#define GS_MID 512           // tiles of (256, GS_MID] pairs are sorted inside the blend (rank counting)
#define GS_MAX_GROUPS 4096   // 64-tile groups (262144 tiles)
#define GS_ORDER_BUCKETS 256u  // gs_tile_order's counting-sort buckets (they live in the front end's LDS)
#ifndef GS_FUSED_OWN_CULL
// a tile-row frame of at most this many chunks: the fused workgroups test their own chunk's bound (no
// cull launch: C2 bands 1-2 us faster); above it the flags of a cull launch (each workgroup's bound
// test adds its latency to every round of workgroups: 10M at 4K, band 0 2.26 vs 2.09 ms)
#define GS_FUSED_OWN_CULL 1024u
#endif
#ifndef GS_FUSED_THREADS
#define GS_FUSED_THREADS 256  // Gaussians per fused workgroup (512 / 1 024 work-items: 1.5 us slower at C2)
#endif
// Work-items per fused workgroup (GS_FUSED_THREADS Gaussians; all walk the pairs): 512 for a frame on the
// caller's stream; 256 for an overlapped frame (SplatOverlap), whose front end runs beside the previous
// frame's blend: a 256-work-item workgroup of at most 64 VGPRs and ~14 KB of LDS takes the slot of one
// retiring blend workgroup (256 work-items, 64 VGPRs, 17 KB), where a 512-work-item one waited for the
// blend's tail (measured: the whole front end ran after the blend; C2 frames 63 vs 56 us serial).
#define GS_FUSED_WG 512
#ifndef GS_FUSED_WG_OV
#define GS_FUSED_WG_OV 256
#endif
template <uint32_t WG> struct GsFusedShape;
template <> struct GsFusedShape<512> {
  static constexpr uint32_t slice = 4096u;  // pairs per slice (C2's chunks hold 1.6k on average, 3.3k at most: one slice)
  static constexpr uint32_t lds_cap = 0u;   // histogram window in tiles (0: the band's)
};
template <> struct GsFusedShape<256> {
  static constexpr uint32_t slice = 2048u;
  static constexpr uint32_t lds_cap = 2048u;  // 8 KB (+ 5.6 KB static): within one blend workgroup's LDS
};
static_assert(GsFusedShape<256>::lds_cap == 2048u,
              "tests/test_splat_windows_gpu.py picks its frame sizes around this window (WINDOW): change both");
#ifndef GS_FUSED_HELPERS
#define GS_FUSED_HELPERS 128u  // helper workgroups per band (one queued slice each)
#endif
#ifndef GS_FUSED_MAX_SCAP
#define GS_FUSED_MAX_SCAP 2048u  // larger tiles (1M Gaussians at 1080p): three launches measured faster
#endif
#ifndef GS_FUSED_RUNS_PER_TILE
#define GS_FUSED_RUNS_PER_TILE 32u  // (C2 Morton order: 6; random order: 51; orbit views up to ~20, where
                                    // fused measured 0.13 vs 0.24 ms for three launches)
#endif
#ifndef GS_SORT_THREADS
#define GS_SORT_THREADS 256
#endif
#ifndef GS_RADIX_MAXR
#define GS_RADIX_MAXR (8448 / GS_SORT_THREADS)  // items per work-item in LDS: up to 8448 keys
#endif

struct SplatCam {
  float view[16];
  float mvp[16];  // proj * view
  float fx, fy;   // P00*W/2, P11*H/2 (fy negative: Vulkan y-down)
  float tan_fovx, tan_fovy;
  uint32_t W, H;
  uint32_t grid_x, grid_y;
  uint32_t row_begin, row_end;  // tile rows
  uint32_t cull;                // tile rows restricted and chunk bounds given: PreArgs.cskip is valid
  uint32_t tight;               // bin by the alpha box (frames without stats / published buffers)
  uint32_t rowcull;             // tile rows restricted: Gaussians whose radius bound misses them skip the rest
  float fmax2;                  // max(fx^2, fy^2)
  float w2;                     // an upper bound of the view rotation's squared spectral norm (1 for lookAt)
};

struct BinGrid {
  uint32_t band_rows, bands, chunks, chunk, grid_x, grid_y, tiles, groups, row0, row1;
};

// The frame's camera: the tile grid, the tile rows clamped to it (row_end < row_begin: an empty frame) and
// which culls and binning the frame takes. Stream-ordered frames bin by the alpha box; stats / published
// frames by the 3-sigma rectangles, unless publish_tight asks for the timed frames' binning (parity tests
// of their integer outputs).
inline SplatCam gs_plan_cam(const float* view, const float* mvp, float p00, float p11, uint32_t W, uint32_t H,
                            uint32_t tile_row_begin, uint32_t tile_row_end, bool chunk_bounds, bool stats,
                            bool publish, bool publish_tight) {
  SplatCam cam;
  std::memcpy(cam.view, view, sizeof(cam.view));
  std::memcpy(cam.mvp, mvp, sizeof(cam.mvp));
  cam.fx = p00 * (float)W * 0.5f;
  cam.fy = p11 * (float)H * 0.5f;
  cam.tan_fovx = 1.0f / p00;
  cam.tan_fovy = 1.0f / (p11 < 0.0f ? -p11 : p11);
  cam.W = W; cam.H = H;
  cam.grid_x = (W + GS_BLOCK_X - 1) / GS_BLOCK_X;
  cam.grid_y = (H + GS_BLOCK_Y - 1) / GS_BLOCK_Y;
  cam.row_begin = std::min(tile_row_begin, cam.grid_y);
  cam.row_end = std::min(tile_row_end, cam.grid_y);
  if (cam.row_end < cam.row_begin) cam.row_end = cam.row_begin;
  cam.rowcull = (cam.row_begin > 0 || cam.row_end < cam.grid_y) ? 1u : 0u;
  cam.cull = (chunk_bounds && cam.rowcull) ? 1u : 0u;
  cam.fmax2 = std::max(cam.fx * cam.fx, cam.fy * cam.fy);
  {  // |W|_2^2 <= the largest Gershgorin row sum of W W^T (W: the view's rotation part; 1 for a lookAt view)
    double ww[3][3], w2 = 0.0;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c)
        ww[r][c] = (double)view[r] * view[c] + (double)view[4 + r] * view[4 + c] + (double)view[8 + r] * view[8 + c];
    for (int r = 0; r < 3; ++r) w2 = std::max(w2, std::fabs(ww[r][0]) + std::fabs(ww[r][1]) + std::fabs(ww[r][2]));
    cam.w2 = (float)(w2 * (1.0 + 1e-5));
  }
  cam.tight = ((!stats && !publish) || (publish && publish_tight)) ? 1u : 0u;
  return cam;
}

// the frame's tiles [begin, end) in row-major order
inline uint32_t gs_tile_begin(const SplatCam& cam) { return cam.row_begin * cam.grid_x; }
inline uint32_t gs_tile_end(const SplatCam& cam) { return cam.row_end * cam.grid_x; }

// 256-Gaussian chunks of n Gaussians: the granule of the chunk bounds / skip flags and the fused front
// end's workgroups
inline uint32_t gs_chunks256(uint32_t n) { return (n + GS_FUSED_THREADS - 1u) / GS_FUSED_THREADS; }

// Bands of as many tile rows as fit GS_BAND_TILES (1080p: one band, 4K: four) x chunks of >= GS_CHUNK_MIN
// Gaussians, ~256 blocks in all (at most GS_MAX_CHUNKS chunks). The bands cover the frame's tile rows only.
// False: the image is beyond the kernels' static limits (W > 131072 px, or more than GS_MAX_GROUPS 64-tile
// groups).
// Chunks: the count / scatter walks are latency-bound loops over a chunk's Gaussians, while every chunk
// writes (count), scans (colscan) and reads (scatter) a histogram row of its band's tiles. So 256
// workgroups in all as long as the rows cost about as much as the walks; beyond that (at least twice
// as many Gaussians per chunk as band tiles: 10M at 4K, a single-band tile-row shard of it) up to
// GS_MAX_CHUNKS (10M at 4K: front end 4.3 -> 2.9 ms; 1M at 1080p with 1 024 chunks: 0.289 -> 0.330 ms).
inline bool gs_plan_grid(const SplatCam& cam, uint32_t n, BinGrid* out) {
  const uint32_t tiles = cam.grid_x * cam.grid_y;
  if (cam.grid_x > GS_BAND_TILES) return false;
  BinGrid bgrid;
  bgrid.grid_x = cam.grid_x;
  bgrid.grid_y = cam.grid_y;
  bgrid.tiles = tiles;
  if ((tiles + 63u) / 64u > GS_MAX_GROUPS) return false;
  bgrid.row0 = cam.row_begin;
  bgrid.row1 = cam.row_end;
  const uint32_t brows = cam.row_end - cam.row_begin;  // the frame's tile rows (the bands cover these)
  bgrid.groups = std::max(1u, (brows * cam.grid_x + 63u) / 64u);
  bgrid.band_rows = std::max(1u, std::min(std::max(brows, 1u), GS_BAND_TILES / cam.grid_x));
  bgrid.bands = std::max(1u, (brows + bgrid.band_rows - 1) / bgrid.band_rows);
  const uint32_t band_tiles = bgrid.band_rows * cam.grid_x;
  const uint32_t want_chunks = std::max(256u / bgrid.bands, (uint32_t)std::min<uint64_t>(GS_MAX_CHUNKS, n / std::max(1u, band_tiles / 2u)));
  bgrid.chunks = std::max(1u, std::min({(uint32_t)GS_MAX_CHUNKS / bgrid.bands, (n + GS_CHUNK_MIN - 1) / GS_CHUNK_MIN,
                                        want_chunks}));
  bgrid.chunk = std::max(1u, (n + bgrid.chunks - 1) / bgrid.chunks);
  *out = bgrid;
  return true;
}

// Spill pool (pairs): at least max(2^20, N) and the current capacity (a reservation included), and 1.25x
// the demand of the latest frame whose front end has run (a hint) when that exceeds the pool. A frame
// reported incomplete: its own demand reaches the host only with the NEXT front end; its spilled tiles
// hold at most its pair count, which is at most `largest_k`, the largest K any frame of the workspace has
// published (device-side running maxima, so a later lighter frame cannot hide it), so the pool grows to
// that now and this frame cannot exhaust it the same way.
inline uint64_t gs_plan_spill_pool(uint32_t n, uint32_t sp_cap, uint32_t demand, bool incomplete, uint32_t largest_k) {
  uint64_t want = std::max<uint64_t>(std::max<uint64_t>(1u << 20, n), sp_cap);
  if (demand > sp_cap) want = std::max<uint64_t>(want, (uint64_t)demand + demand / 4u);
  if (incomplete) want = std::max<uint64_t>(want, (uint64_t)largest_k + largest_k / 4u);
  return std::min<uint64_t>(want, 0xFFFFFFF0u);
}
// the pool's capacity (pairs) given its two allocations
inline uint32_t gs_spill_capacity(size_t keys_bytes, size_t vals_bytes) {
  return (uint32_t)std::min<size_t>(std::min(keys_bytes / 8, vals_bytes / 4), 0xFFFFFFF0u);
}

// Front end: the fused single launch (gs_bin_fused_kernel) once an earlier frame of this workspace has
// published its largest tile (have_hint; the rows' capacity scap follows it with 1/4 headroom, a power of
// two in [256, GS_FUSED_MAX_SCAP]); otherwise, or above that capacity, count + colscan + scatter (0).
// frontend: 0 three launches, 1 fused, 2 the policy: the fused path while frames touch at most
// GS_FUSED_RUNS_PER_TILE (workgroup, tile) runs per tile (Gaussians in a spatially coherent order: each
// workgroup touches a compact set of tiles; in random order every workgroup touches most tiles and the
// reservations cost more than the histograms), else three launches. Both front ends publish the frame's
// touched runs (the fused kernel's reservations, the count kernel's nonzero histogram entries); the
// latest one decides, so the choice is made from the first finished frame on and follows the data's
// coherence both ways.
inline uint32_t gs_plan_scap(int frontend, uint32_t touched_runs, bool have_hint, uint32_t n, uint32_t tiles,
                             uint32_t largest_tile) {
  const bool want_fused = frontend == 1 || (frontend == 2 && touched_runs <= GS_FUSED_RUNS_PER_TILE * tiles);
  uint32_t scap = 0;
  if (want_fused && have_hint && n) {
    const uint32_t big = std::max(256u, largest_tile + largest_tile / 4u);
    uint32_t c = 256;
    while (c < big && c < GS_FUSED_MAX_SCAP) c <<= 1;
    if (big <= GS_FUSED_MAX_SCAP && (size_t)tiles * c * 8 <= ((size_t)4 << 30)) scap = c;
  }
  return scap;
}

// The `over` composite ends each pixel with out = C + T * under, and a call with stats may enqueue its blend
// more than once (splat.hip, gs_wait_and_rerun: a fused frame above its rows, a three-launch frame above the
// pair buffer). Where the W * H RGBA32F ranges of `under` and `out` overlap at all, a second blend would read
// the first one's result as `under`: such a call blends over a copy of `under` taken before its first blend.
// A frame without stats blends once and copies nothing; without `under` there is nothing to keep.
inline bool gs_plan_under_copy(bool stats, const void* under, const void* out, uint32_t W, uint32_t H) {
  if (!stats || !under) return false;
  const uintptr_t u = (uintptr_t)under, o = (uintptr_t)out;
  return (u > o ? u - o : o - u) < (uint64_t)W * H * 16u;  // (the distance, not u + bytes: no wrap)
}

// Helper workgroups per band only when the latest fused frame queued slices (a static view whose chunks
// all fit one slice launches none; the owners walk any slice no helper takes, so a frame that queues more
// than the helpers take is complete anyway). Idle helpers polled the queue until every owner had
// published, and their last poll (~3 us sleep) could end the kernel late.
inline uint32_t gs_plan_helpers(bool always, uint32_t queued) {
  return always ? GS_FUSED_HELPERS : queued ? std::min<uint32_t>(GS_FUSED_HELPERS, queued + queued / 2u + 8u) : 0u;
}
// slice queue: room for twice the slices of the largest pair count seen (+ one per owner)
inline uint32_t gs_plan_queue_cap(uint32_t pairs_hint, uint32_t owners) {
  return std::max<uint32_t>(4096u, 2u * (pairs_hint / GsFusedShape<256>::slice) + owners);
}

// The fused workgroup's shape (GsFusedShape: 256 work-items beside another frame's blend, else 512; wg_env
// 256 / 512 overrides) and its dynamic LDS: the histogram window (the shape's lds_cap entries; 0: the whole
// band), at least the tile order's buckets.
struct GsFusedPlan {
  uint32_t wg;
  size_t lds;
};
inline GsFusedPlan gs_plan_fused_shape(int wg_env, bool overlapped, size_t band_lds) {
  GsFusedPlan p;
  p.wg = wg_env == 256 || wg_env == 512 ? (uint32_t)wg_env : overlapped ? (uint32_t)GS_FUSED_WG_OV : (uint32_t)GS_FUSED_WG;
  const uint32_t cap = p.wg == 256 ? GsFusedShape<256>::lds_cap : GsFusedShape<512>::lds_cap;
  p.lds = std::max<size_t>(cap ? std::min<size_t>(band_lds, (size_t)cap * 4u) : band_lds,
                           (size_t)GS_ORDER_BUCKETS * 4u);
  return p;
}

// The large-tile sort (gs_sort_large_kernel), from the hints of a recent frame: it runs when that frame's
// largest tile is above GS_MID; its LDS holds tiles of up to GS_SORT_THREADS * sort_r pairs (the largest
// tile + 1/8 headroom, sort_r odd), its workgroups follow the large-tile count (+ 1/4); tiles beyond the
// LDS limit sort in a global scratch (three launches), and a fused frame needs a workgroup per
// GS_SORT_THREADS tiles at least.
struct GsSortPlan {
  uint32_t r, grid;
};
inline GsSortPlan gs_plan_sort(uint32_t largest_tile, uint32_t large_tiles) {
  GsSortPlan p;
  const uint32_t big = largest_tile + largest_tile / 8u;
  p.r = std::min((uint32_t)GS_RADIX_MAXR, ((big + GS_SORT_THREADS - 1) / GS_SORT_THREADS) | 1u);
  p.grid = std::max(64u, std::min(4096u, large_tiles + large_tiles / 4u));
  return p;
}
inline bool gs_plan_sort_large(uint32_t largest_tile) { return largest_tile > GS_MID; }
inline bool gs_plan_sort_scratch(uint32_t largest_tile) { return largest_tile > GS_SORT_THREADS * GS_RADIX_MAXR; }
inline uint32_t gs_plan_sort_grid_fused(uint32_t sort_grid, uint32_t tiles) {
  return std::max(sort_grid, (tiles + GS_SORT_THREADS - 1) / GS_SORT_THREADS);
}

}  // namespace ptgs
