// splat_run.h — what a splat frame call decides on the host without the device: what the front end of an
// overlapped call (PTGS_FLAG_SPLAT_OVERLAP) waits for, how many workspaces the ring holds, and which of the
// earlier frames' reports a call returns. Plain values in, plain values out; streams are opaque pointers.
// No HIP include: tests/native/splat_run_check.cpp builds it with a host compiler alone. api.cpp turns the
// answers into events, stream waits and error codes (splat_overlap_begin, splat_finish).
#pragma once

#include <stdint.h>

#include <cstdlib>

namespace ptgs {

// Frames in flight: the front end of call k may run beside the blends of calls k - 1 .. k - depth + 1, each
// on a workspace of its own, so the ring holds depth workspaces (PTGS_GS_OV_DEPTH=2 .. 4, default 3).
constexpr uint32_t kSplatRingMax = 4;  // workspaces the ring may hold (PTGS_OV_RING in earlier sources)
constexpr uint32_t kSplatRingDefault = 3;
inline uint32_t splat_ring_depth(const char* env) {
  const int x = env ? std::atoi(env) : (int)kSplatRingDefault;
  return (uint32_t)(x < 2 ? 2 : x > (int)kSplatRingMax ? (int)kSplatRingMax : x);
}

// A run: consecutive accepted overlapped calls of a context. A call without the flag and a views call end it.
// The workspace that call k takes was last used by call k - depth, whose blend ran before the blend of call
// k - back (back = depth - 1) on the caller's stream: once THAT blend has started the workspace is free.
// So the rule looks back at most kSplatLookBack calls, and that is all the state keeps: prev[j] is the
// call j + 1 calls back, and `calls` counts the run's calls only up to kSplatLookBack.
constexpr uint32_t kSplatLookBack = kSplatRingMax - 1;
struct SplatRun {
  uint32_t depth = 0;         // workspaces in the ring, 2 .. kSplatRingMax (0: the context has not overlapped)
  uint32_t calls = 0;         // min(accepted calls so far in the run, kSplatLookBack)
  uint64_t next_ordinal = 1;  // of the next blend; ordinals go on counting across runs
  struct Call {
    uint64_t ordinal;  // of the blend it launched (0: none)
    const void* stream;
  } prev[kSplatLookBack] = {};
};

// What the front end of the next call, made on `stream`, waits for before it touches its workspace.
struct SplatWait {
  enum Kind : uint32_t {
    Ordinal,    // the blend ordinal `ordinal` in the signal word: no event on the caller's stream
    RunMarker,  // the marker event already recorded in this run (it covers the workspace's last use)
    NewMarker   // a marker to be recorded on `stream` now, then waited for
  } kind;
  uint64_t ordinal;
};

// With k accepted calls so far in the run and same = the previous min(k, back) calls were all on `stream`:
// the ordinal of call k - back when k >= back && same and that call launched a blend; otherwise the run's
// marker when 0 < k < back && same (the workspace was last used before the run); otherwise a new marker (the
// first call of a run, a call whose ordering is not known: no blend launched, or another stream).
// (calls saturates at kSplatLookBack >= back, so both comparisons with back read as they would with k)
inline SplatWait next_wait(const SplatRun& r, const void* stream) {
  const uint32_t back = r.depth - 1;
  bool same = true;
  for (uint32_t j = 0; j < r.calls && j < back; ++j) same = same && r.prev[j].stream == stream;
  if (r.calls >= back && same && r.prev[back - 1].ordinal) return {SplatWait::Ordinal, r.prev[back - 1].ordinal};
  if (r.calls > 0 && r.calls < back && same) return {SplatWait::RunMarker, 0};
  return {SplatWait::NewMarker, 0};
}

// After an accepted call's frame: its stream, and its blend's ordinal if it launched one with it.
inline void record(SplatRun& r, const void* stream, bool launched, uint64_t ordinal) {
  for (uint32_t j = kSplatLookBack - 1; j > 0; --j) r.prev[j] = r.prev[j - 1];
  r.prev[0] = {launched ? ordinal : 0, stream};
  if (launched) r.next_ordinal = ordinal + 1;
  if (r.calls < kSplatLookBack) ++r.calls;
}

// (prev[] is not read before `calls` calls have been recorded again)
inline void end_run(SplatRun& r) { r.calls = 0; }

// The reports about EARLIER frames (the bits of SplatReport, splat.h) and the code a call returns. Each kind
// of report is returned once, never dropped, one per call, in ptgs.h's order (PTGS_EBADIDS): a call that
// fails for a reason of its own returns that code and keeps every report for the calls after it; a
// successful call returns bad ids first and keeps an incomplete frame for the call after it.
constexpr uint32_t kSplatReportIncomplete = 1u, kSplatReportBadIds = 2u;
enum class SplatCode : uint32_t { Ok, Own, BadIds, Incomplete };  // Own: the call's own failure code
struct SplatLatch {
  SplatCode code;
  uint32_t pending;  // kept for the next call
};
inline SplatLatch latch_report(uint32_t pending, bool rc_ok, uint32_t report) {
  report |= pending;
  if (!rc_ok) return {SplatCode::Own, report};
  if (report & kSplatReportBadIds) return {SplatCode::BadIds, report & kSplatReportIncomplete};
  if (report & kSplatReportIncomplete) return {SplatCode::Incomplete, 0};
  return {SplatCode::Ok, 0};
}

}  // namespace ptgs
