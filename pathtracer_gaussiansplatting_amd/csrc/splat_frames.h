// splat_frames.h — what a context's splat frame calls share, under one owner (api.cpp alone includes this):
// the workspaces, the streams and events that run them side by side, the signal word of the blend ordinals,
// the run of overlapped calls and the reports kept for the next call (splat_run.h decides; this holds).
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/ptgs/ptgs.h"
#include "splat.h"
#include "splat_run.h"

namespace ptgs {

// which of the context's workspaces a traversal is at (ptgs_splat_status_read counts them differently)
enum class SplatRole { Current, OtherRing, View };

struct SplatFrames {
  // PTGS_FLAG_SPLAT_OVERLAP: ring[0] is the context's first workspace (there from the start), ring[1 ..
  // run.depth - 1] come when the context first overlaps; ring[pos] rendered the latest frame and is the one
  // every other call works on (current()). `fe` is the front-end stream, `marker` the caller's stream at the
  // start of a run (or later: next_wait), `done` the front end's end, `signal` the device word the blends
  // store their ordinals in.
  SplatWorkspace* ring[kSplatRingMax] = {};
  uint32_t pos = 0;
  hipStream_t fe = nullptr;
  hipEvent_t marker = nullptr, done = nullptr;
  unsigned long long* signal = nullptr;
  SplatRun run;
  uint32_t pending_report = 0;  // earlier frames' reports not yet returned (latch_report)
  // ptgs_splat_gaussians_views: views 1.. run on their own workspaces and non-blocking streams, forked from /
  // joined back into the caller's stream with events (view 0 renders into current() on the caller's stream)
  struct View {
    SplatWorkspace* ws = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t join = nullptr;
  } views[PTGS_MAX_VIEWS - 1];
  hipEvent_t fork = nullptr;

  // (runs inside `new ptgs_ctx()`, before ptgs_create has selected the device: splat_workspace_create does no
  // HIP work, it allocates on first use; should that change, create ring[0] in ptgs_create instead)
  SplatFrames() { ring[0] = splat_workspace_create(); }
  SplatFrames(const SplatFrames&) = delete;
  SplatFrames& operator=(const SplatFrames&) = delete;
  ~SplatFrames() {
    (void)for_each_workspace([](SplatRole, uint32_t, SplatWorkspace* ws) {
      splat_workspace_destroy(ws);
      return hipSuccess;
    });
    for (View& v : views) {
      if (v.stream) (void)hipStreamDestroy(v.stream);
      if (v.join) (void)hipEventDestroy(v.join);
    }
    if (fe) (void)hipStreamDestroy(fe);
    for (hipEvent_t ev : {fork, marker, done})
      if (ev) (void)hipEventDestroy(ev);
    if (signal) (void)hipFree(signal);
  }

  SplatWorkspace* current() const { return ring[pos]; }
  View& view(uint32_t v) { return views[v - 1]; }  // v = 1 .. PTGS_MAX_VIEWS - 1
  // the next overlapped call takes the ring's next workspace (last used run.depth calls ago)
  void advance() { pos = (pos + 1) % run.depth; }

  // f(role, view, workspace) over every workspace there is: the current one, the views' (view = 1 ..), the
  // ring's others (view = 0 for both ring roles). Stops at the first error and returns it.
  template <class F>
  hipError_t for_each_workspace(F&& f) {
    hipError_t e = f(SplatRole::Current, 0u, current());
    for (uint32_t v = 1; v < PTGS_MAX_VIEWS && e == hipSuccess; ++v)
      if (view(v).ws) e = f(SplatRole::View, v, view(v).ws);
    for (uint32_t i = 0; i < kSplatRingMax && e == hipSuccess; ++i)
      if (ring[i] && i != pos) e = f(SplatRole::OtherRing, 0u, ring[i]);
    return e;
  }
};

}  // namespace ptgs
