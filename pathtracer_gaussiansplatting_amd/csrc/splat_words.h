// splat_words.h — the counter words of the 3DGS forward pass: the four small word arrays through which the
// kernels and the host talk (pinned mailbox, device counters, the three-launch scalars, the large-tile list).
// Every stage header and the frame call (splat.hip) use these names; this header relies on no other.
#pragma once
#include <cstdint>

namespace ptgs {

// ---- counter words ---------------------------------------------------------------------------------
// The kernels and the host talk through four small word arrays. Every slot is named here, with its
// writer (W) and reader (R); front end = count / scatter or the fused kernel, blend = gs_sort_blend_kernel.

// k_host: the pinned, coherent host mailbox (SplatWorkspace::k_host; the device writes through k_dev).
// Racy hints: the host reads them without waiting, or after the K event when stats are requested.
enum GsHostWord : uint32_t {
  GS_KH_PAIRS = 0,        // the frame's pair count K. W: scatter / fused blend block (0, 0). R: pair buffers, queue size, stats
  GS_KH_MAX_TILE = 1,     // largest tile (fused: a bound, at least 256). W: same. R: scap, the next sort's shape
  GS_KH_LARGE_TILES = 2,  // tiles above GS_MID pairs. W: same. R: the next sort's grid
  GS_KH_RUNS = 4,         // touched (workgroup, tile) runs. W: same. R: the front-end policy, splat_front_end_info
  GS_KH_OVER_SCAP = 5,    // fused: tiles above their row's capacity (scatter: 0). W: same. R: the stats re-run
  GS_KH_PUBLISHED_BY = 6, // 1 fused / 2 three launches. W: same. A diagnostic: the host does not read it
  GS_KH_SPILL_DEMAND = 8, // the previous frame's spill demand (pairs). W: gs_spill_rearm. R: the pool's size
  GS_KH_INCOMPLETE = 9,   // <- 1: a tile the spill pool could not hold. W: gs_spill_tile. R (exchanged with 0): the next call's report, splat_status
  GS_KH_BAD_IDS = 10,     // <- 1: an id >= N (PreArgs::bad_ids). W: the preprocess. R (exchanged): the next call's report
  GS_KH_QUEUED = 11,      // slices the fused front end queued. W: fused blend block (0, 0). R: the helper count
  GS_KH_MAX_K_FUSED = 12, // the workspace's largest K, fused frames (GS_FZ_MAX_K). W: fused blend block (0, 0). R: the pool's size after a report
  GS_KH_MAX_K_THREE = 13, // the same for three-launch frames (GS_TOT_MAX_K). W: scatter. R: same
  GS_KH_WORDS = 16
};

// fz: device counters of both front ends, the blend and the spill pool (zeroed once; each user re-arms
// what it leaves nonzero). The queue words are polled by the helpers: a cache line of their own.
enum GsFzWord : uint32_t {
  GS_FZ_MAX_TILE = 1,     // largest tile above 256 pairs. W: fused front end (atomicMax). R + re-arm: fused blend block (0, 0)
  GS_FZ_ABOVE_MID = 4,    // tiles above GS_MID pairs. W: fused front end. R + re-arm: same
  GS_FZ_OVER_SCAP = 5,    // tiles above scap. W: fused front end. R + re-arm: same
  GS_FZ_POOL_CURSOR = 8,  // spill pool cursor (pairs). W: gs_spill_tile (atomicAdd). R + re-arm: the next front end (gs_spill_rearm), splat_status
  GS_FZ_SPILLED = 9,      // tiles completed through the pool, ever. W: gs_spill_tile. R: splat_status
  GS_FZ_INCOMPLETE = 10,  // tiles the pool could not hold, ever. W: gs_spill_tile. R: splat_status
  GS_FZ_MAX_DEMAND = 11,  // largest spill demand of a frame. W: gs_spill_rearm. R: splat_status
  GS_FZ_MAX_K = 13,       // largest K of a fused frame. W + R: fused blend block (0, 0), which hands it to GS_KH_MAX_K_FUSED
  GS_FZ_COUNTERS = 16,    // the counters above: what splat_status reads back
  GS_FZ_Q_CLAIMS = 32,    // slice queue: claims. W: helpers (atomicAdd). Re-arm: fused blend block (0, 0)
  GS_FZ_Q_ENTRIES = 33,   // slice queue: entries. W: owners. R: helpers, the blend (GS_KH_QUEUED). Re-arm: same
  GS_FZ_Q_OWNERS = 34,    // slice queue: owners that have published. W: owners. R: helpers. Re-arm: same
  GS_FZ_WORDS = 64
};
static_assert(GS_FZ_Q_CLAIMS * 4u % 64u == 0 && GS_FZ_Q_OWNERS / 16u == GS_FZ_Q_CLAIMS / 16u &&
              GS_FZ_COUNTERS <= GS_FZ_Q_CLAIMS, "the queue words share one cache line with no counter");

// total: the three-launch front end's scalars
enum GsTotalWord : uint32_t {
  GS_TOT_PAIRS = 0,     // K. W: scatter block (0, 0)
  GS_TOT_MAX_TILE = 1,  // largest tile. W: colscan (atomicMax); re-arm: count block (0, 0). R: scatter (GS_KH_MAX_TILE)
  GS_TOT_MAX_K = 2,     // largest K of a three-launch frame. W + R: scatter, which hands it to GS_KH_MAX_K_THREE
  GS_TOT_WORDS = 4
};
// large_ctr: the three-launch large-tile list
enum GsLargeWord : uint32_t {
  GS_LC_COUNT = 0,  // its length. W: colscan (atomicAdd); re-arm: count block (0, 0). R: scatter (GS_KH_LARGE_TILES), gs_sort_large_kernel
  GS_LC_WORDS = 4
};

}  // namespace ptgs
