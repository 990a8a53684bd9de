// splat_workspace.h — the forward pass's workspace, one per ptgs_ctx: every device buffer a frame uses, the
// pinned mailbox, the events and what the host remembers from frame to frame. Host code only. The buffers are
// DevBuf members (dev_buf.h) and free themselves; the word arrays' slots are named in splat_words.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dev_buf.h"
#include "splat.h"

namespace ptgs {

struct SplatWorkspace {
  DevBuf means2d, depths, conic, rec, radii, touched, pairs, keys_out, vals_out, ranges, hist, tile_info,
      group_total, tile_slots, point_keys, total, rect, large, large_ctr, sort_scratch;
  DevBuf cursor, fz, pub_offs, keys_pub, vals_pub;  // fused front end (see gs_bin_fused_kernel); fz: counters
  DevBuf dbg_depths, fzp, nzbuf, order;  // order: the blend's tile order (heavy first, fused frames)
  DevBuf crect, sp_keys, sp_vals;  // spilled tiles (gs_spill_tile): chunk rects, the spill pool
  DevBuf fsq;                 // the fused front end's slice queue
  DevBuf cskip;               // per 256-Gaussian chunk: skipped by a tile-row-restricted frame
  DevBuf grad_acc;            // the backward pass's per-Gaussian sums (splat_backward.hip)
  DevBuf pose_partials;       // the pose gradient's per-workgroup partial sums (splat_backward.hip)
  DevBuf under_copy;          // a stats frame's `under` where it overlaps `out` (gs_plan_under_copy)
  uint32_t sp_cap = 0;        // spill pool capacity (pairs)
  uint32_t incomplete = 0;    // frames reported incomplete (spill pool exhausted) since the last status clear
  uint32_t spilled_base = 0, incomplete_base = 0;  // GS_FZ_SPILLED / GS_FZ_INCOMPLETE at the last status clear
  bool ids_error = false;     // a frame met an out-of-range ptgs_gaussians.ids entry
  bool have_hint = false;     // a finished frame has published its largest tile: the fused path can size its rows
  bool hint_recorded = false;
  hipEvent_t hint_event = nullptr;
  bool last_fused = false;    // the last frame ran the fused front end
  uint32_t last_scap = 0;     // and its slot rows' capacity (ptgs_splat_get_tile_rows)
  uint32_t* k_host = nullptr;  // pinned, coherent [GS_KH_WORDS] (GsHostWord)
  uint32_t* k_dev = nullptr;   // its device-side address
  hipEvent_t k_event = nullptr;
  uint32_t last_n = 0, last_k = 0, last_tiles = 0;
  bool last_published = false;  // the last frame published its sorted keys / values and was synchronised
  uint32_t last_w = 0, last_h = 0;  // its image size
  bool last_full = false;       // and it rendered every tile row without the `over` composite (splat_last_frame)
  uint32_t sort_r = 3;        // large-tile radix sort: items per work-item (from the previous frame's largest tile)
  uint32_t sort_grid = 256;   // its workgroups (from the previous frame's large-tile count)
  bool sort_attr = false;     // its dynamic-LDS limit raised
  hipEvent_t ev[7] = {};
  bool timed = false;
};

SplatWorkspace* splat_workspace_create() { return new SplatWorkspace(); }

void splat_workspace_destroy(SplatWorkspace* w) {
  if (!w) return;
  if (w->k_host) (void)hipHostFree(w->k_host);
  for (hipEvent_t& e : w->ev)
    if (e) (void)hipEventDestroy(e);
  if (w->k_event) (void)hipEventDestroy(w->k_event);
  if (w->hint_event) (void)hipEventDestroy(w->hint_event);
  delete w;  // (the DevBuf members free their buffers)
}

// The forward pass's growth policy: at least 16 bytes, a quarter more than asked for
static hipError_t ensure(DevBuf& b, size_t bytes) {
  if (bytes == 0) bytes = 16;
  return b.ensure(bytes, bytes / 4);
}

}  // namespace ptgs
