// splat.hip — 3D Gaussian splatting forward rasterizer for gfx950.
//
// The reference has no Gaussian rasterizer; this restates the published forward
// pass (Kerbl et al., SIGGRAPH 2023) in the reference's camera conventions (glm::lookAt RH view,
// Vulkan ZO projection with [1][1] negated, camera.cpp:186-187). A frame is a front end that bins
// (Gaussian, tile) pairs, then a per-tile sort and blend. Two front ends (gs_plan_scap chooses):
//  three launches (the first frames of a workspace, incoherent orders, tiles above GS_FUSED_MAX_SCAP pairs):
//   1. count        (band of tile rows x chunk of Gaussians) workgroups: preprocess one Gaussian per
//                   work-item (frustum cull (d <= 0.2), Sigma = R S^2 R^T, EWA Sigma' = J W Sigma W^T J^T
//                   (+0.3 low-pass), conic, 3-sigma radius, tile rect, a 48-B blend record), then the
//                   chunk's pairs into an LDS tile histogram (load-balanced wave expansion)
//   2. colscan      per 64 tiles: prefix of the histograms over the chunks, tile totals, large-tile list
//   3. scatter      same grid as 1: (depth << 32 | gaussian) into each touched tile's segment through
//                   LDS cursors; tile ranges; K and the frame's other hints to pinned host memory
//  fused (the default once a frame has published its largest tile): one launch, gs_bin_fused_kernel:
//                   the same preprocess per 256-Gaussian chunk, the chunk's pairs counted in LDS, one
//                   returning atomic per touched tile reserves a run of the tile's fixed-capacity row;
//                   the blend's block (0, 0) publishes the hints
// then, for both:
//   sort large      (frames after one with a tile above GS_MID pairs) radix sort of the large tiles
//   sort+blend      one workgroup per 16x16 tile: sort by (depth, gaussian) (= the order of a stable
//                   global sort of (tile << 32 | depth) keys), publish keys/values, per-quadrant
//                   culled front-to-back alpha blend; a tile whose pairs the front end could not all
//                   store is completed through the spill pool (gs_spill_tile)
// Everything is enqueued before K is read back (buffers sized from earlier frames' hints, re-run on
// growth when stats are requested), so the host never stalls the GPU. Integer outputs (radii, tiles, keys,
// values, ranges) are the bit-exact contract with oracle/ptgs_oracle.c; the image is within 1e-4 relative
// L2 (hardware exp2 in the blend).
//
// This file is the one translation unit of the forward pass and holds its host side: the frame call
// (splat_gaussians: seven stages over one GsCall), reserve / status and the accessors. The device code is
// in per-stage headers, included by this file alone, in the order of a frame; each includes the headers whose
// names it uses:
//   splat_words.h       the counter words the kernels and the host talk through
//   splat_workspace.h   SplatWorkspace and its buffers (DevBuf, dev_buf.h)
//   splat_wave.h        wave64 / workgroup primitives: DPP scan and reduce, lane exchanges, the sorts' networks
//   splat_preprocess.h  PreArgs, gs_preprocess_one, the chunk cull
//   splat_bin.h         count / colscan / scatter, the walks both front ends share, the blend's tile order
//   splat_fused.h       GsFused, gs_bin_fused_kernel
//   splat_sort_large.h  gs_sort_large_kernel
//   splat_spill.h       GsSpill, gs_spill_tile
//   splat_blend.h       gs_sort_blend_kernel, the publish kernels
//   splat_spatial.h     not part of a frame: spatial order and chunk bounds of a Gaussian set (included at the
//                       end: the code object lists kernel templates in the order of their first launch, and
//                       the frame's come first)
// (splat_plan.h: the host's planning rules and the shapes shared with the kernels; splat_probe.h: stamps and probes)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "../../include/ptgs/ptgs.h"
#include "detmath.h"
#include "splat.h"
#include "splat_backward.h"
#include "splat_plan.h"
#include "splat_probe.h"
#include "splat_words.h"
#include "splat_workspace.h"
#include "splat_wave.h"
#include "splat_preprocess.h"
#include "splat_bin.h"
#include "splat_fused.h"
#include "splat_sort_large.h"
#include "splat_spill.h"
#include "splat_blend.h"

namespace ptgs {

// ---- the frame call --------------------------------------------------------------------------------
// splat_gaussians is a sequence of stages over one GsCall. The mailbox words (GsHostWord) are racy hints:
// each stage reads the ones it needs where it runs (some again after the K event, on purpose), never a
// snapshot taken once per call; the rules applied to them are splat_plan.h's.
struct GsCall {
  SplatWorkspace* w;
  const SplatArgs* a;
  hipStream_t s;
  const SplatOverlap* ov;  // null: a serial frame (frames with stats, published or timed always are)
  uint32_t n, tiles, rows, slot_keys;
  SplatCam cam;
  BinGrid bgrid;
  size_t band_lds;     // a band's histogram (bytes)
  PreArgs pa;
  uint32_t nwg_fused;  // the fused front end's owner workgroups (bands x 256-Gaussian chunks)
  uint32_t* order;     // the blend's tile order (heaviest tiles of the previous frame first; null: no rows)
  uint32_t scap;       // the fused rows' capacity (0: three launches)
  const float* under;  // the `over` composite's image: the caller's, or the workspace's copy of it (gs_keep_under)
};

static hipError_t gs_mark(const GsCall& c, int k) {
  return c.a->time_stages ? hipEventRecord(c.w->ev[k], c.s) : hipSuccess;
}

// a small word array, allocated and zeroed once
static hipError_t ensure_zeroed_once(DevBuf& b, uint32_t words) {
  if (b.p) return hipSuccess;
  hipError_t e;
  if ((e = ensure(b, words * 4u))) return e;
  return hipMemset(b.p, 0, words * 4u);
}

// The pair capacity the buffers give (the published keys count only for a frame that publishes them)
static uint32_t pair_capacity(const SplatWorkspace* w, bool publish) {
  size_t c = std::min(w->pairs.bytes / 8, w->vals_out.bytes / 4);
  if (publish) c = std::min(c, w->keys_out.bytes / 8);
  return (uint32_t)std::min<size_t>(c, 0xFFFFFFFFu);
}
// Grow the pair buffers to K pairs (hipFree waits for the frames that use the old buffers)
static hipError_t grow_pairs(SplatWorkspace* w, size_t K, bool keys) {
  hipError_t e;
  if ((e = ensure(w->pairs, K * 8))) return e;
  if ((e = ensure(w->vals_out, K * 4))) return e;
  if (keys && (e = ensure(w->keys_out, K * 8))) return e;
  return hipSuccess;
}
// Grow the spill pool to `pairs` (frees the old pool: waits)
static hipError_t grow_spill(SplatWorkspace* w, uint64_t pairs) {
  hipError_t e;
  if ((e = ensure(w->sp_keys, pairs * 8)) || (e = ensure(w->sp_vals, pairs * 4))) return e;
  w->sp_cap = gs_spill_capacity(w->sp_keys.bytes, w->sp_vals.bytes);
  return hipSuccess;
}

// Stage 2: the per-Gaussian and per-tile buffers, sized by the plan alone, and the counter arrays
static hipError_t gs_ensure_buffers(GsCall& c) {
  SplatWorkspace* w = c.w;
  const uint32_t n = c.n, tiles = c.tiles;
  const BinGrid& bgrid = c.bgrid;
  hipError_t e;
  if (c.a->time_stages && !w->ev[0])
    for (hipEvent_t& ev : w->ev)
      if ((e = hipEventCreate(&ev))) return e;
  if ((e = ensure(w->means2d, (size_t)n * 8))) return e;
  if ((e = ensure(w->depths, (size_t)n * 4))) return e;
  if ((e = ensure(w->conic, (size_t)n * 16))) return e;
  if ((e = ensure(w->rec, (size_t)n * 48))) return e;
  if ((e = ensure(w->radii, (size_t)n * 4))) return e;
  if ((e = ensure(w->dbg_depths, (size_t)n * 4))) return e;
  if ((e = ensure(w->touched, (size_t)n * 4))) return e;
  if ((e = ensure(w->rect, (size_t)n * 8))) return e;
  if ((e = ensure(w->ranges, (size_t)tiles * 8))) return e;
  if ((e = ensure(w->hist, (size_t)bgrid.chunks * tiles * 4))) return e;
  if ((e = ensure(w->nzbuf, (size_t)bgrid.chunks * bgrid.bands * 4))) return e;
  if ((e = ensure(w->tile_slots, (size_t)tiles * GS_TILE_SLOTS * 8))) return e;
  if ((e = ensure(w->tile_info, (size_t)tiles * 8))) return e;
  if ((e = ensure(w->group_total, (size_t)bgrid.groups * 4))) return e;
  if ((e = ensure(w->large, (size_t)tiles * 4))) return e;
  if ((e = ensure_zeroed_once(w->large_ctr, GS_LC_WORDS))) return e;
  if ((e = ensure_zeroed_once(w->total, GS_TOT_WORDS))) return e;
  if (!w->k_host) {
    if ((e = hipHostMalloc((void**)&w->k_host, GS_KH_WORDS * 4u, hipHostMallocCoherent | hipHostMallocMapped))) return e;
    std::memset(w->k_host, 0, GS_KH_WORDS * 4u);
    if ((e = hipHostGetDevicePointer((void**)&w->k_dev, w->k_host, 0))) return e;
  }
  if (!w->fz.p) {  // (zeroed in stream order: the first frame's front end is its first user)
    if ((e = ensure(w->fz, GS_FZ_WORDS * 4u))) return e;
    if ((e = hipMemsetAsync(w->fz.p, 0, GS_FZ_WORDS * 4u, c.s))) return e;
  }
#ifndef GS_K_EVENT_FLAGS
#define GS_K_EVENT_FLAGS (hipEventDisableTiming | hipEventDisableSystemFence)
#endif
  // the K event only signals the host (stats requested): k_host is fine-grained (coherent) memory the
  // GPU writes past its caches, so the event needs no system-scope cache release
  if (!w->k_event && (e = hipEventCreateWithFlags(&w->k_event, GS_K_EVENT_FLAGS))) return e;
  return hipSuccess;
}

// Stage 3. An earlier frame of this workspace left a spilled tile incomplete (pool exhausted;
// GS_KH_INCOMPLETE, a device store seen once that frame has run) or met an id >= N (GS_KH_BAD_IDS):
// reported by this call, which renders its own frame after growing the pool (splat_common maps it to
// PTGS_EINCOMPLETE / PTGS_EBADIDS). A call with stats waits for the earlier frames first (it is synchronous
// anyway), so their reports are its own and the flags its superseded runs may raise can be dropped later.
static hipError_t gs_collect_reports(const GsCall& c, uint32_t* report) {
  SplatWorkspace* w = c.w;
  hipError_t e;
  if (c.a->stats && (e = hipStreamSynchronize(c.s))) return e;
  if (__atomic_exchange_n(w->k_host + GS_KH_INCOMPLETE, 0u, __ATOMIC_ACQ_REL)) {
    ++w->incomplete;
    *report |= SPLAT_REPORT_INCOMPLETE;
  }
  if (__atomic_exchange_n(w->k_host + GS_KH_BAD_IDS, 0u, __ATOMIC_ACQ_REL)) *report |= SPLAT_REPORT_BAD_IDS;
  return hipSuccess;
}

// Stage 4: the spill pool (gs_plan_spill_pool; growth frees the old pool: waits) and the pair buffers.
// Pair capacity. The call is stream-ordered: scatter and blend are enqueued against the current pair
// buffer, and a tile whose segment ends beyond it is completed through the spill pool. The buffer starts
// at 8 pairs per Gaussian and grows from the K that earlier frames wrote to pinned host memory
// (GS_KH_PAIRS, read here without waiting: a hint); with stats requested the call waits for this frame's
// K and re-runs scatter + blend after growing, so that frame's published layout is always exact.
static hipError_t gs_size_pools(const GsCall& c, uint32_t report) {
  SplatWorkspace* w = c.w;
  const bool incomplete = (report & SPLAT_REPORT_INCOMPLETE) != 0;
  hipError_t e;
  const uint32_t demand = w->k_host[GS_KH_SPILL_DEMAND];
  const uint32_t largest_k =
      incomplete ? std::max({w->k_host[GS_KH_PAIRS], w->k_host[GS_KH_MAX_K_FUSED], w->k_host[GS_KH_MAX_K_THREE]}) : 0u;
  const uint64_t want = gs_plan_spill_pool(c.n, w->sp_cap, demand, incomplete, largest_k);
  if ((want > w->sp_cap || !w->sp_keys.p) && (e = grow_spill(w, want))) return e;
  if (w->pairs.bytes < (size_t)c.n * 64 && (e = grow_pairs(w, (size_t)c.n * 8, false))) return e;
  if (c.a->publish && (e = ensure(w->keys_out, w->pairs.bytes))) return e;
  if (w->k_host[GS_KH_PAIRS] > pair_capacity(w, c.a->publish) && (e = grow_pairs(w, w->k_host[GS_KH_PAIRS], c.a->publish)))
    return e;
  return hipSuccess;
}

// Stage 4, last: the `over` composite of a call with stats whose `under` overlaps `out` (every hybrid caller
// composites in place). Stage 6 may enqueue the blend again, and a second blend would read the first one's
// result as `under` and composite the Gaussians twice: every blend of such a call reads a copy of `under`
// taken here, in stream order before the first. Calls without stats blend once: no copy, nothing enqueued.
static hipError_t gs_keep_under(GsCall& c) {
  const SplatArgs& a = *c.a;
  c.under = a.under;
  if (!gs_plan_under_copy(a.stats != nullptr, a.under, a.out, a.W, a.H)) return hipSuccess;
  const size_t bytes = (size_t)a.W * a.H * 16;
  hipError_t e;
  if ((e = c.w->under_copy.ensure(bytes, 0))) return e;  // (an image's size: no headroom)
  if ((e = hipMemcpyAsync(c.w->under_copy.p, a.under, bytes, hipMemcpyDeviceToDevice, c.s))) return e;
  c.under = (const float*)c.w->under_copy.p;
  return hipSuccess;
}

// Stage 5, first: the front ends' per-Gaussian arguments and the buffers only they use
static hipError_t gs_front_end_args(GsCall& c) {
  SplatWorkspace* w = c.w;
  const ptgs_gaussians* g = c.a->g;
  const uint32_t n = c.n;
  hipError_t e;
  PreArgs& pa = c.pa;
  pa.means = g->means;
  pa.scales = g->scales;
  pa.rots = g->rotations;
  pa.opac = g->opacities;
  pa.colors = g->colors;
  pa.n = n;
  pa.means2d = (float2*)w->means2d.p;
  pa.depths = (float*)w->depths.p;
  pa.conic_o = (float4*)w->conic.p;
  pa.radii = (int*)w->radii.p;
  pa.touched = (uint32_t*)w->touched.p;
  pa.rects = (ushort4*)w->rect.p;
  pa.rec = (float4*)w->rec.p;
  pa.ids = g->ids;
  pa.dbg_depths = (float*)w->dbg_depths.p;
  pa.bad_ids = w->k_dev + GS_KH_BAD_IDS;
  // chunks whose bound misses the rows are skipped by the front end before their loads: the fused
  // kernel tests its own chunk's bound; the three-launch count reads flags of a small launch before it
  pa.cskip = nullptr;
  pa.cbounds = c.cam.cull ? (const float4*)g->chunk_bounds : nullptr;
  if (c.cam.cull) {
    if ((e = ensure(w->cskip, gs_chunks256(n)))) return e;
    pa.cskip = (const uint8_t*)w->cskip.p;
  }
  if (!c.a->publish) {  // the per-Gaussian debug outputs only for a published frame (ptgs_splat_get_buffers)
    pa.radii = nullptr;
    pa.touched = nullptr;
    pa.means2d = nullptr;
    pa.conic_o = nullptr;
    pa.dbg_depths = nullptr;
  }
  // per front-end workgroup chunk rects (gs_spill_tile): fused (bands x 256-Gaussian chunks) or count
  if ((e = ensure(w->crect, (size_t)std::max(c.nwg_fused, c.bgrid.bands * c.bgrid.chunks) * 8))) return e;
  c.order = nullptr;
  if (c.rows) {
    if ((e = ensure(w->order, (size_t)c.tiles * 4))) return e;
    c.order = (uint32_t*)w->order.p;
  }
  return hipSuccess;
}

// the environment's A/B switches
static int gs_env_frontend() {  // PTGS_GS_FRONTEND = "three" (0) / "fused" (1); unset: the policy (2)
  static const int v = [] {
    const char* s = getenv("PTGS_GS_FRONTEND");
    if (s && !strcmp(s, "three")) return 0;
    if (s && !strcmp(s, "fused")) return 1;
    return 2;
  }();
  return v;
}
static bool gs_env_helpers_always() {  // PTGS_GS_HELPERS = "always"
  static const bool v = [] {
    const char* s = getenv("PTGS_GS_HELPERS");
    return s && !strcmp(s, "always");
  }();
  return v;
}
static int gs_env_fe_wg() {  // PTGS_GS_FE_WG = 256 / 512
  static const int v = [] {
    const char* s = getenv("PTGS_GS_FE_WG");
    return s ? atoi(s) : 0;
  }();
  return v;
}

static hipError_t gs_cull_flags(const GsCall& c, hipStream_t cs) {
  if (!c.cam.cull) return hipSuccess;
  const uint32_t nch = gs_chunks256(c.n);
  hipLaunchKernelGGL(gs_chunk_cull_kernel, dim3((nch + 255u) / 256u), dim3(256), 0, cs, c.cam,
                     (const float4*)c.a->g->chunk_bounds, nch, (uint8_t*)c.w->cskip.p);
  return hipGetLastError();
}

// the sort's and the blend's view of a three-launch frame
static GsFused gs_not_fused(const GsCall& c) {
  const SplatSeq* seq = c.a->seq;
  return {0u, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, c.order, nullptr, 0u,
          seq ? seq->flag : nullptr, seq ? seq->ordinal : 0ull};
}

static hipError_t gs_blend(const GsCall& c, uint32_t cap, const GsFused& fu, unsigned long long* keys_out,
                           bool sort_large) {
  if (c.rows == 0) return hipSuccess;
  SplatWorkspace* w = c.w;
  const SplatArgs& a = *c.a;
  const bool fused_fe = fu.scap != 0;
  GsSpill sp;
  sp.fz = (uint32_t*)w->fz.p;
  sp.k_host = w->k_dev;
  sp.keys = (unsigned long long*)w->sp_keys.p;
  sp.vals = (uint32_t*)w->sp_vals.p;
  sp.cap = w->sp_cap;
  sp.crect = (const ushort4*)w->crect.p;
  sp.bands = c.bgrid.bands;
  sp.chunk = fused_fe ? GS_FUSED_THREADS : c.bgrid.chunk;
  sp.nwg = fused_fe ? c.nwg_fused : c.bgrid.bands * c.bgrid.chunks;
  sp.n = c.n;
  sp.rects = (const ushort4*)w->rect.p;
  sp.depths = (const float*)w->depths.p;
  sp.ids = a.g->ids;
  auto k = a.depth ? gs_sort_blend_kernel<true> : gs_sort_blend_kernel<false>;
  const dim3 grid(c.cam.grid_x, c.rows);
  hipLaunchKernelGGL(k, grid, dim3(GS_BLOCK), 0, c.s, c.cam, (const uint2*)w->ranges.p, (unsigned long long*)w->pairs.p,
                     sort_large ? (uint32_t)GS_MID : 0xFFFFFFFFu, keys_out, (uint32_t*)w->vals_out.p,
                     (const float4*)w->rec.p, a.bg[0], a.bg[1], a.bg[2], cap, c.slot_keys,
                     (const unsigned long long*)w->tile_slots.p, a.depth, (const float4*)c.under, (float4*)a.out, fu, sp);
  const hipError_t le = hipGetLastError();
  if (!le && a.seq && fu.seq_flag) a.seq->launched = true;
  return le;
}

// Tiles above GS_MID pairs: sorted by gs_sort_large_kernel ahead of the blend when the previous frame had
// any (else the blend sorts the rare one itself). Fused: no tile list, every workgroup checks up to
// GS_SORT_THREADS tiles by their cursors. Three launches (cap: the pair capacity): tiles beyond the LDS
// capacity sort in a global scratch ([2][g_cap] u32 + [2][g_cap] u16 at the pair offsets), allocated once a
// frame has had such tiles.
static hipError_t gs_sort_large(const GsCall& c, uint32_t cap, const GsFused& fu, unsigned long long* keys_out) {
  SplatWorkspace* w = c.w;
  hipError_t e;
  if (!w->sort_attr) {
    if ((e = hipFuncSetAttribute((const void*)gs_sort_large_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)gs_radix_lds(GS_RADIX_MAXR))))
      return e;
    w->sort_attr = true;
  }
  uint32_t g_cap = 0;
  if (!fu.scap && gs_plan_sort_scratch(w->k_host[GS_KH_MAX_TILE])) {
    if ((e = ensure(w->sort_scratch, (size_t)cap * 12u))) return e;
    g_cap = (uint32_t)std::min<size_t>(w->sort_scratch.bytes / 12u, 0xFFFFFFFFu);
  }
  uint32_t* g_dep = g_cap ? (uint32_t*)w->sort_scratch.p : nullptr;
  uint16_t* g_slot = g_cap ? (uint16_t*)(g_dep + 2 * (size_t)g_cap) : nullptr;
  const uint32_t grid = fu.scap ? gs_plan_sort_grid_fused(w->sort_grid, c.tiles) : w->sort_grid;
  hipLaunchKernelGGL(gs_sort_large_kernel, dim3(grid), dim3(GS_SORT_THREADS), gs_radix_lds(w->sort_r), c.s,
                     (const uint2*)w->ranges.p, (unsigned long long*)w->pairs.p,
                     (const unsigned long long*)w->tile_slots.p, (const uint32_t*)w->large.p,
                     (const uint32_t*)w->large_ctr.p, keys_out, (uint32_t*)w->vals_out.p,
                     (const uint32_t*)w->total.p, cap, w->sort_r, g_dep, g_slot, g_cap, fu, c.tiles);
  return hipGetLastError();
}

// Stage 5, fused: front end (on the overlap's stream, if any), large-tile sort, blend, and for a
// published frame the compaction into the three-launch layout
static hipError_t gs_enqueue_fused(const GsCall& c) {
  SplatWorkspace* w = c.w;
  const SplatArgs& a = *c.a;
  const SplatOverlap* ov = c.ov;
  const SplatCam& cam = c.cam;
  const hipStream_t s = c.s;
  const uint32_t tiles = c.tiles, scap = c.scap;
  hipError_t e2;
  if ((e2 = ensure(w->tile_slots, (size_t)tiles * scap * 8))) return e2;
  if ((e2 = ensure(w->vals_out, (size_t)tiles * scap * 4))) return e2;
  if (a.publish && (e2 = ensure(w->keys_out, (size_t)tiles * scap * 8))) return e2;
  // the front end's stream: the caller's, or (overlapped frame) the second stream once ov->wait is done
  const hipStream_t sf = ov ? ov->fe : s;
  if (ov && ov->wait && (e2 = hipStreamWaitEvent(sf, ov->wait, 0))) return e2;
  // (or the workspace's reuse from the blend ordinals, SplatSeq: a wait packet on the front end's queue,
  // which holds no workgroup slots while it waits and puts nothing on the caller's queue)
  if (ov && ov->wait_flag &&
      (e2 = hipStreamWaitValue64(sf, (void*)ov->wait_flag, ov->wait_ordinal, hipStreamWaitValueGte, ~0ull)))
    return e2;
  if (w->cursor.bytes < (size_t)tiles * 4) {  // zero between frames (the blend re-arms what it reads)
    if ((e2 = ensure(w->cursor, (size_t)tiles * 4))) return e2;
    if ((e2 = hipMemsetAsync(w->cursor.p, 0, w->cursor.bytes, sf))) return e2;
  }
  const uint32_t helpers = gs_plan_helpers(gs_env_helpers_always(), w->k_host[GS_KH_QUEUED]);
  // owners (bands x chunks) and helpers (bands x helpers) each publish their partials
  const uint32_t nwg = c.nwg_fused + c.bgrid.bands * helpers;
  if ((e2 = ensure(w->fzp, (size_t)nwg * 8))) return e2;
  // slice queue: zero once here, re-armed by the blend after every frame
  const uint32_t qcap = gs_plan_queue_cap(w->k_host[GS_KH_PAIRS], c.nwg_fused);
  if (w->fsq.bytes < (size_t)qcap * 8) {
    if ((e2 = ensure(w->fsq, (size_t)qcap * 8))) return e2;
    if ((e2 = hipMemsetAsync(w->fsq.p, 0, w->fsq.bytes, sf))) return e2;
  }
  const uint32_t fsq_cap = (uint32_t)std::min<size_t>(w->fsq.bytes / 8, 0x7FFFFFFFu);
  GsFused fu = {scap, (uint32_t*)w->cursor.p, (uint32_t*)w->fz.p, w->k_dev, (uint2*)w->ranges.p,
                (uint32_t*)w->fzp.p, nwg, c.order, (uint2*)w->fsq.p, fsq_cap, a.seq ? a.seq->flag : nullptr,
                a.seq ? a.seq->ordinal : 0ull};
  PreArgs fpa = c.pa;  // the fused walk keeps rects / depths in registers (band 0 stores them for gs_spill_tile)
  if (cam.cull && gs_chunks256(c.n) > GS_FUSED_OWN_CULL) {
    if ((e2 = gs_cull_flags(c, sf))) return e2;
    fpa.cbounds = nullptr;
  }
  fpa.rects = nullptr;
  fpa.depths = nullptr;
  BinGrid fg = c.bgrid;
  fg.chunks = gs_chunks256(c.n);
  fg.chunk = GS_FUSED_THREADS;
  // the tile order: the front end's extra workgroup from the previous frame's counts, or (overlapped,
  // own_order) a launch behind the front end from this frame's own counts
  const bool own_order = c.order && ov && ov->own_order;
  uint32_t* fe_order = own_order ? nullptr : c.order;
  const GsFusedPlan shape = gs_plan_fused_shape(gs_env_fe_wg(), ov != nullptr, c.band_lds);
  auto fk = shape.wg == 256 ? (cam.rowcull ? gs_bin_fused_kernel<true, 256> : gs_bin_fused_kernel<false, 256>)
                            : (cam.rowcull ? gs_bin_fused_kernel<true, 512> : gs_bin_fused_kernel<false, 512>);
  hipLaunchKernelGGL(fk, dim3(fg.bands, fg.chunks + helpers + (fe_order ? 1u : 0u)), dim3(shape.wg), shape.lds, sf,
                     cam, fpa, fg, scap, (uint32_t*)w->cursor.p, (uint32_t*)w->fz.p, (uint32_t*)w->fzp.p,
                     (unsigned long long*)w->tile_slots.p, (const uint2*)w->ranges.p, fe_order,
                     gs_tile_begin(cam), gs_tile_end(cam), (ushort4*)w->crect.p, (ushort4*)w->rect.p,
                     (float*)w->depths.p, w->k_dev, (uint2*)w->fsq.p, fsq_cap, (uint32_t)(shape.lds / 4u));
  if ((e2 = hipGetLastError())) return e2;
  if (own_order) {
    hipLaunchKernelGGL(gs_tile_order_kernel, dim3(1), dim3(GS_ORDER_THREADS), 0, sf, (const uint32_t*)w->cursor.p,
                       c.order, gs_tile_begin(cam), gs_tile_end(cam));
    if ((e2 = hipGetLastError())) return e2;
  }
  if (ov && ((e2 = hipEventRecord(ov->done, sf)) || (e2 = hipStreamWaitEvent(s, ov->done, 0)))) return e2;
  if ((e2 = gs_mark(c, 1)) || (e2 = gs_mark(c, 2)) || (e2 = gs_mark(c, 3))) return e2;
  unsigned long long* keys_out = a.publish ? (unsigned long long*)w->keys_out.p : nullptr;
  const bool sort_large = gs_plan_sort_large(w->k_host[GS_KH_MAX_TILE]);
  if (sort_large && (e2 = gs_sort_large(c, 0u, fu, keys_out))) return e2;
  if ((e2 = gs_mark(c, 4)) || (e2 = gs_mark(c, 5))) return e2;
  if ((e2 = gs_blend(c, 0u, fu, keys_out, sort_large))) return e2;
  if (a.publish) {  // compact the published rows into the three-launch layout (tests only)
    if ((e2 = ensure(w->pub_offs, (size_t)tiles * 4))) return e2;
    if ((e2 = ensure(w->keys_pub, (size_t)tiles * scap * 8))) return e2;  // (K <= tiles * scap)
    if ((e2 = ensure(w->vals_pub, (size_t)tiles * scap * 4))) return e2;
    const uint32_t tb = gs_tile_begin(cam), te = gs_tile_end(cam);
    hipLaunchKernelGGL(gs_publish_scan_kernel, dim3(1), dim3(GS_PUB_THREADS), 0, s, (const uint2*)w->ranges.p, tiles,
                       tb, te, scap, (uint32_t*)w->pub_offs.p);
    hipLaunchKernelGGL(gs_publish_copy_kernel, dim3(tiles), dim3(256), 0, s, (const uint2*)w->ranges.p,
                       (const uint32_t*)w->pub_offs.p, tb, te, scap, (const unsigned long long*)w->keys_out.p,
                       (const uint32_t*)w->vals_out.p, (unsigned long long*)w->keys_pub.p, (uint32_t*)w->vals_pub.p,
                       (uint2*)w->ranges.p);
    if ((e2 = hipGetLastError())) return e2;
  }
  if (a.stats && (e2 = hipEventRecord(w->k_event, s))) return e2;  // K is on the host after the blend
  return gs_mark(c, 6);
}

// Stage 5, three launches: scatter, large-tile sort and blend against a pair buffer of `cap` pairs (run
// again by stage 6 after growing it)
static hipError_t gs_enqueue_tail(const GsCall& c, uint32_t cap) {
  SplatWorkspace* w = c.w;
  const BinGrid& bgrid = c.bgrid;
  // (read here, not before: grow_pairs may have moved the published-keys buffer since the last call)
  unsigned long long* keys_out = c.a->publish ? (unsigned long long*)w->keys_out.p : nullptr;
  hipLaunchKernelGGL(gs_bin_scatter_kernel, dim3(bgrid.bands, bgrid.chunks), dim3(GS_BIN_THREADS),
                     2 * c.band_lds + (size_t)bgrid.groups * 4, c.s, bgrid, (const ushort4*)w->rect.p,
                     (const float*)w->depths.p, c.a->g->ids, c.n, (const uint32_t*)w->hist.p, (const uint2*)w->tile_info.p,
                     (const uint32_t*)w->group_total.p, (uint32_t*)w->total.p, (const uint32_t*)w->large_ctr.p, w->k_dev,
                     (const uint32_t*)w->nzbuf.p, bgrid.bands * bgrid.chunks, cap,
                     (uint2*)w->ranges.p, (unsigned long long*)w->pairs.p, (unsigned long long*)w->tile_slots.p);
  hipError_t e2 = hipGetLastError();
  if (e2) return e2;
  if (c.a->stats && (e2 = hipEventRecord(w->k_event, c.s))) return e2;  // K is on the host after the scatter
  if ((e2 = gs_mark(c, 3))) return e2;
  const GsFused no_fu = gs_not_fused(c);
  const bool sort_large = gs_plan_sort_large(w->k_host[GS_KH_MAX_TILE]);
  if (sort_large && (e2 = gs_sort_large(c, cap, no_fu, keys_out))) return e2;
  if ((e2 = gs_mark(c, 4)) || (e2 = gs_mark(c, 5))) return e2;
  if ((e2 = gs_blend(c, cap, no_fu, keys_out, sort_large))) return e2;
  return gs_mark(c, 6);
}
static hipError_t gs_enqueue_three(const GsCall& c) {
  SplatWorkspace* w = c.w;
  const SplatCam& cam = c.cam;
  const BinGrid& bgrid = c.bgrid;
  hipError_t e2;
  if ((e2 = ensure(w->tile_slots, (size_t)c.tiles * GS_TILE_SLOTS * 8))) return e2;
  if ((e2 = gs_cull_flags(c, c.s))) return e2;
  // (n == 0: one chunk of nothing; the count still zeroes the histograms and the colscan publishes K = 0)
  hipLaunchKernelGGL(cam.rowcull ? gs_bin_count_kernel<true> : gs_bin_count_kernel<false>,
                     dim3(bgrid.bands, bgrid.chunks + (c.order ? 1u : 0u)), dim3(GS_COUNT_THREADS),
                     std::max(c.band_lds, (size_t)GS_ORDER_BUCKETS * 4), c.s, cam, c.pa, bgrid, (uint32_t*)w->hist.p,
                     (uint32_t*)w->total.p, (uint32_t*)w->large_ctr.p, w->k_dev, (uint32_t*)w->nzbuf.p,
                     (const uint2*)w->ranges.p, c.order, gs_tile_begin(cam), gs_tile_end(cam),
                     (uint32_t*)w->fz.p, (ushort4*)w->crect.p);
  if ((e2 = hipGetLastError())) return e2;
  if ((e2 = gs_mark(c, 1))) return e2;
  hipLaunchKernelGGL(gs_bin_colscan_kernel, dim3(bgrid.groups), dim3(GS_COLSCAN_THREADS), 0, c.s, bgrid, (uint32_t*)w->hist.p,
                     (uint2*)w->tile_info.p, (uint32_t*)w->group_total.p, (uint32_t*)w->total.p, (uint32_t)GS_MID,
                     (uint32_t*)w->large.p, (uint32_t*)w->large_ctr.p);
  if ((e2 = hipGetLastError())) return e2;
  if ((e2 = gs_mark(c, 2))) return e2;
  return gs_enqueue_tail(c, pair_capacity(w, c.a->publish));
}

// Stage 6 (stats requested): wait for this frame's K. A fused frame with a tile above its row capacity, or
// a three-launch frame above the pair buffer, was completed through the spill pool; a call with stats
// re-runs it so that its published keys / values / ranges are the exact layout (three launches, grown
// buffers). *redone: the fused frame was re-run through three launches.
static hipError_t gs_wait_and_rerun(const GsCall& c, bool fused, uint32_t* K, bool* redone) {
  SplatWorkspace* w = c.w;
  const bool publish = c.a->publish;
  hipError_t e;
  if ((e = hipEventSynchronize(w->k_event))) return e;
  *K = w->k_host[GS_KH_PAIRS];
  if (fused && w->k_host[GS_KH_OVER_SCAP]) {
    *redone = true;
    if ((e = gs_mark(c, 0)) || (e = gs_enqueue_three(c))) return e;
    if ((e = hipEventSynchronize(w->k_event))) return e;
    *K = w->k_host[GS_KH_PAIRS];
  }
  bool regrown = false;
  if ((!fused || *redone) && *K > pair_capacity(w, publish)) {
    if ((e = grow_pairs(w, *K, publish))) return e;
    if ((e = gs_mark(c, 2))) return e;
    if ((e = gs_enqueue_tail(c, pair_capacity(w, publish)))) return e;
    regrown = true;
  }
  if (*redone || regrown) {  // the superseded run's spilled tiles may have exhausted the pool: the
                             // re-run completed the frame, so its report is dropped
    if ((e = hipStreamSynchronize(c.s))) return e;
    __atomic_store_n(w->k_host + GS_KH_INCOMPLETE, 0u, __ATOMIC_RELEASE);
  }
  return hipSuccess;
}

// Stage 7: what the next frame of this workspace plans from
static hipError_t gs_record_hints(const GsCall& c, bool fused, uint32_t K) {
  SplatWorkspace* w = c.w;
  const SplatArgs& a = *c.a;
  hipError_t e;
  w->last_fused = fused;
  w->last_scap = fused ? c.scap : 0u;
  // the fused path sizes its rows from the largest tile of a finished frame: valid once the host has
  // seen one complete (a frame still in flight has not written its hint yet)
  if (!w->have_hint) {
    if (!w->hint_event && (e = hipEventCreateWithFlags(&w->hint_event, hipEventDisableTiming))) return e;
    if (w->hint_recorded && hipEventQuery(w->hint_event) == hipSuccess) w->have_hint = true;
    if (!w->hint_recorded || a.stats) {
      if ((e = hipEventRecord(w->hint_event, c.s))) return e;
      w->hint_recorded = true;
    }
    if (a.stats) w->have_hint = true;  // (waited for above)
  }
  // the next frame's large-tile sort, from a recent frame's largest tile and large-tile count; hints only
  const GsSortPlan sp = gs_plan_sort(w->k_host[GS_KH_MAX_TILE], w->k_host[GS_KH_LARGE_TILES]);
  w->sort_r = sp.r;
  w->sort_grid = sp.grid;
  w->last_n = c.n;
  w->last_k = K;
  w->last_tiles = c.tiles;
  w->last_published = a.publish && a.stats;
  w->last_w = a.W;
  w->last_h = a.H;
  w->last_full = !a.depth && c.cam.row_begin == 0 && c.cam.row_end == c.cam.grid_y;
  return hipSuccess;
}

hipError_t splat_gaussians(SplatWorkspace* w, const SplatArgs& a, uint32_t* report) {
  hipError_t e;
  *report = 0;
  w->last_full = false;  // (a call that fails leaves no frame for the backward pass)
  w->timed = a.time_stages;
  GsCall c;
  c.w = w;
  c.a = &a;
  c.s = a.stream;
  c.ov = (a.stats || a.publish || a.time_stages) ? nullptr : a.ov;  // (these frames are synchronous or instrumented: serial)
  // 1. plan: the camera, the band / chunk grid (no mailbox word involved)
  c.n = a.g->count;
  c.cam = gs_plan_cam(a.view, a.mvp, a.p00, a.p11, a.W, a.H, a.tile_row_begin, a.tile_row_end,
                      a.g->chunk_bounds != nullptr, a.stats != nullptr, a.publish, a.publish_tight);
  if (!gs_plan_grid(c.cam, c.n, &c.bgrid)) return hipErrorInvalidValue;
  c.tiles = c.bgrid.tiles;
  c.rows = c.cam.row_end - c.cam.row_begin;
  c.band_lds = (size_t)c.bgrid.band_rows * c.cam.grid_x * 4;
  c.nwg_fused = c.bgrid.bands * gs_chunks256(c.n);
  c.slot_keys = c.n < (1u << 24) ? 1u : 0u;  // the register sort packs the gaussian in 24 bits
  // 2 - 4. buffers, the earlier frames' reports, the pools their hints size
  if ((e = gs_ensure_buffers(c))) return e;
  if ((e = gs_collect_reports(c, report))) return e;
  if ((e = gs_size_pools(c, *report))) return e;
  if ((e = gs_keep_under(c))) return e;
  // 5. the front end (gs_plan_scap, from the latest frame's touched runs and largest tile) and the frame
  if ((e = gs_front_end_args(c))) return e;
  c.scap = gs_plan_scap(gs_env_frontend(), w->k_host[GS_KH_RUNS], w->have_hint, c.n, c.tiles, w->k_host[GS_KH_MAX_TILE]);
  const bool fused = c.scap != 0;
  if ((e = gs_mark(c, 0))) return e;
  if ((e = fused ? gs_enqueue_fused(c) : gs_enqueue_three(c))) return e;
  // 6. with stats: this frame's K, and the exact layout
  uint32_t K = w->k_host[GS_KH_PAIRS];  // without stats: the latest K any frame published (a hint)
  bool redone = false;
  if (a.stats) {
    if ((e = gs_wait_and_rerun(c, fused, &K, &redone))) return e;
    a.stats->num_rendered = K;
    a.stats->tiles_x = c.cam.grid_x;
    a.stats->tiles_y = c.cam.grid_y;
    a.stats->num_visible = 0;
    a.stats->fused = fused && !redone ? 1u : 0u;
  }
  // 7. the next frame's hints
  return gs_record_hints(c, fused && !redone, K);
}

// pairs: the pair buffer (three launches: a frame of K <= pairs stores every pair) and the spill pool
// (fused rows: a frame's spilled tiles hold at most K pairs) — a frame of at most `pairs` pairs is always
// rendered completely, whichever front end runs and whatever its row capacity (hipGraph replays too)
hipError_t splat_reserve(SplatWorkspace* w, uint32_t pairs) {
  hipError_t e;
  if ((e = grow_pairs(w, pairs, w->keys_out.p != nullptr))) return e;
  if (pairs > w->sp_cap && (e = grow_spill(w, pairs))) return e;
  return hipSuccess;
}

hipError_t splat_status(SplatWorkspace* w, bool clear, SplatStatusOut* out) {
  *out = SplatStatusOut{};
  if (w->k_host && __atomic_exchange_n(w->k_host + GS_KH_INCOMPLETE, 0u, __ATOMIC_ACQ_REL)) ++w->incomplete;
  out->incomplete = w->incomplete;
  if (clear) w->incomplete = 0;
  out->capacity = pair_capacity(w, false);
  out->last_pairs = splat_pair_hint(w);
  out->spill_capacity = w->sp_cap;
  if (w->fz.p) {  // device counters (the caller has drained the workspace's stream)
    uint32_t ctr[GS_FZ_COUNTERS];
    const hipError_t e = hipMemcpy(ctr, w->fz.p, sizeof(ctr), hipMemcpyDeviceToHost);
    if (e) return e;
    out->spilled_tiles = ctr[GS_FZ_SPILLED] - w->spilled_base;
    out->incomplete_tiles = ctr[GS_FZ_INCOMPLETE] - w->incomplete_base;
    out->spill_demand = std::max(ctr[GS_FZ_POOL_CURSOR], ctr[GS_FZ_MAX_DEMAND]);
    if (clear) {
      w->spilled_base = ctr[GS_FZ_SPILLED];
      w->incomplete_base = ctr[GS_FZ_INCOMPLETE];
    }
  }
  return hipSuccess;
}

uint32_t splat_pair_hint(const SplatWorkspace* w) { return w->k_host ? w->k_host[GS_KH_PAIRS] : 0u; }

void splat_front_end_info(const SplatWorkspace* w, uint32_t* touched_runs, uint32_t* fused) {
  *touched_runs = w->k_host ? w->k_host[GS_KH_RUNS] : 0u;
  *fused = w->last_fused ? 1u : 0u;
}

hipError_t splat_stage_ms(SplatWorkspace* w, float* out_ms) {
  for (int k = 0; k < 6; ++k) out_ms[k] = 0.0f;
  if (!w->timed || !w->ev[0]) return hipSuccess;
  hipError_t e = hipEventSynchronize(w->ev[6]);
  if (e) return e;
  for (int k = 0; k < 6; ++k)
    if ((e = hipEventElapsedTime(&out_ms[k], w->ev[k], w->ev[k + 1]))) return e;
  return hipSuccess;
}

void splat_get_buffers(const SplatWorkspace* w, ptgs_splat_buffers* out) {
  out->radii = (const int32_t*)w->radii.p;
  out->tiles_touched = (const uint32_t*)w->touched.p;
  out->sorted_keys = !w->last_published ? nullptr : (const uint64_t*)(w->last_fused ? w->keys_pub.p : w->keys_out.p);
  out->sorted_values = !w->last_published ? nullptr : (const uint32_t*)(w->last_fused ? w->vals_pub.p : w->vals_out.p);
  out->tile_ranges = (const uint32_t*)w->ranges.p;
  out->means2d = (const float*)w->means2d.p;
  out->depths = (const float*)w->dbg_depths.p;
  out->conic_opacity = (const float*)w->conic.p;
  out->num_gaussians = w->last_n;
  out->num_rendered = w->last_k;
  out->num_tiles = w->last_tiles;
}

void splat_last_frame(const SplatWorkspace* w, SplatFrame* out) {
  out->valid = w->last_published && w->last_full;
  out->n = w->last_n;
  out->W = w->last_w;
  out->H = w->last_h;
  out->tiles = w->last_tiles;
  out->sorted_values = (const uint32_t*)(w->last_fused ? w->vals_pub.p : w->vals_out.p);
  out->ranges = (const uint2*)w->ranges.p;
  out->rec = (const float4*)w->rec.p;
  out->radii = (const int*)w->radii.p;
}

hipError_t splat_backward_scratch(SplatWorkspace* w, uint32_t n, uint32_t floats_per_gaussian, float** acc) {
  const hipError_t e = ensure(w->grad_acc, (size_t)n * floats_per_gaussian * 4);
  *acc = (float*)w->grad_acc.p;
  return e;
}

hipError_t splat_backward_pose_scratch(SplatWorkspace* w, uint32_t n, float** partials) {
  const hipError_t e = ensure(w->pose_partials, (size_t)((n + 255u) / 256u) * GS_POSE_K * 4);
  *partials = (float*)w->pose_partials.p;
  return e;
}

void splat_get_tile_rows(const SplatWorkspace* w, const unsigned long long** rows, uint32_t* cap) {
  *rows = w->last_scap ? (const unsigned long long*)w->tile_slots.p : nullptr;
  *cap = w->last_scap;
}

hipError_t splat_point_keys(SplatWorkspace* w, size_t npix, unsigned long long** keys) {
  hipError_t e = ensure(w->point_keys, npix * 8);
  *keys = (unsigned long long*)w->point_keys.p;
  return e;
}

}  // namespace ptgs

// scene preparation, after the frame's code (see the map above)
#include "splat_spatial.h"

GS_STAMP_EXPORT
