// splat_run_check — csrc/splat_run.h against a reference model, on the host alone (no HIP, no GPU).
//
// Wait rule: for each ring depth 2, 3, 4 every sequence of 9 calls, depth-first; a call is one of: stream A
// with a blend launched, stream A with no blend launched, stream B with a blend launched, rejected (its
// arguments failed: the frame call returns before it touches the run), run ended (a call without the flag, or
// a views call). 9 calls take the run's call counter past every look-back (3 at most) and well beyond it.
// At every step next_wait is compared with the model below, which keeps the UNBOUNDED history of the run
// and applies the rule as ptgs.h / the header's comment state it:
//   back = depth - 1, k = accepted calls so far in the run, same = the previous min(k, back) calls were all
//   on this stream;
//   Ordinal of call k - back   when k >= back && same and that call launched a blend,
//   RunMarker                  otherwise, when 0 < k < back && same,
//   NewMarker                  otherwise.
// Also: an Ordinal names the ordinal recorded as launched by the call exactly depth - 1 accepted calls back in
// the same run; the ordinals handed out are strictly increasing and advance only past launched blends, across
// runs too. A rejected call is a step at which nothing is recorded and the walk goes on from the same state
// (next_wait takes the state by const reference, so the header cannot change it; that api.cpp rejects a call
// before it touches the run is pinned by the GPU test of the rejected call, not here).
// Report latch: 4 report masks x 4 pending masks x {ok, failing} against the table of ptgs.h's text
// (PTGS_EBADIDS, "Order of the reports"). Ring depth: PTGS_GS_OV_DEPTH strings.
//
// Prints "splat_run_check cases N violations V"; exit status 1 when V != 0.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "splat_run.h"

using namespace ptgs;

namespace {

constexpr int kCalls = 9;
enum Choice { A_BLEND, A_NONE, B_BLEND, REJECTED, RUN_ENDED, kChoices };

long long g_cases = 0, g_violations = 0;
void violation(const char* what, uint32_t depth, int step) {
  if (++g_violations <= 20) fprintf(stderr, "violation: %s (depth %u, call %d of its sequence)\n", what, depth, step);
}

// the model: everything the run has seen, never truncated
struct Model {
  struct Call {
    uint64_t ordinal;  // 0: no blend launched
    const void* stream;
  } hist[kCalls];
  int k = 0;                  // accepted calls so far in the run
  uint64_t last_blend = 0;    // the ordinal of the latest launched blend of the context (0: none yet)
};

SplatWait model_wait(const Model& m, uint32_t depth, const void* stream) {
  const int back = (int)depth - 1, k = m.k;
  bool same = true;
  for (int j = 1; j <= (k < back ? k : back); ++j) same = same && m.hist[k - j].stream == stream;
  if (k >= back && same && m.hist[k - back].ordinal) return {SplatWait::Ordinal, m.hist[k - back].ordinal};
  if (0 < k && k < back && same) return {SplatWait::RunMarker, 0};
  return {SplatWait::NewMarker, 0};
}

const char kStreams[2] = {};  // (two distinct addresses: the streams are opaque)
const void* const kStreamA = &kStreams[0];
const void* const kStreamB = &kStreams[1];

void walk(SplatRun run, Model m, uint32_t depth, int step) {
  if (step == kCalls) return;
  for (int ch = 0; ch < kChoices; ++ch) {
    SplatRun r = run;
    Model mm = m;
    ++g_cases;
    if (ch == REJECTED) {
      // (the frame call returns before splat_overlap_begin: nothing is asked of the run and nothing recorded.
      // The walk continues from the unchanged state; the comparison guards this program's own copying)
      if (memcmp(&r, &run, sizeof(r)) != 0) violation("the walk's copy of the state differs", depth, step);
    } else if (ch == RUN_ENDED) {
      end_run(r);
      mm.k = 0;
      if (r.next_ordinal != run.next_ordinal) violation("ending a run changed the next ordinal", depth, step);
    } else {
      const void* stream = ch == B_BLEND ? kStreamB : kStreamA;
      const bool launched = ch != A_NONE;
      const SplatWait got = next_wait(r, stream), want = model_wait(mm, depth, stream);
      if (got.kind != want.kind || got.ordinal != want.ordinal) violation("next_wait differs from the model", depth, step);
      if (got.kind == SplatWait::Ordinal) {
        const int back = (int)depth - 1;
        if (mm.k < back || got.ordinal == 0 || got.ordinal != mm.hist[mm.k - back].ordinal)
          violation("an Ordinal that the call depth - 1 calls back did not launch", depth, step);
      }
      // the ordinal this call's blend gets: one past the latest launched blend, whatever run that was in
      const uint64_t ordinal = r.next_ordinal;
      if (ordinal != mm.last_blend + 1) violation("the ordinal handed out is not one past the latest launched blend", depth, step);
      record(r, stream, launched, ordinal);
      mm.hist[mm.k++] = {launched ? ordinal : 0, stream};
      if (launched) mm.last_blend = ordinal;
      if (r.next_ordinal != mm.last_blend + 1) violation("the next ordinal did not follow the launched blends", depth, step);
    }
    walk(r, mm, depth, step + 1);
  }
}

void check_latch() {
  // ok calls, by the union of the pending and the new reports (bit 0 incomplete, bit 1 bad ids): bad ids
  // first, an incomplete frame beside them kept for the call after; then incomplete; then OK
  const SplatLatch ok_table[4] = {{SplatCode::Ok, 0}, {SplatCode::Incomplete, 0}, {SplatCode::BadIds, 0},
                                  {SplatCode::BadIds, kSplatReportIncomplete}};
  for (uint32_t report = 0; report < 4; ++report)
    for (uint32_t pending = 0; pending < 4; ++pending)
      for (int ok = 0; ok < 2; ++ok) {
        ++g_cases;
        const SplatLatch got = latch_report(pending, ok != 0, report);
        // a failing call returns its own code and keeps the union pending
        const SplatLatch want = ok ? ok_table[report | pending] : SplatLatch{SplatCode::Own, report | pending};
        if (got.code != want.code || got.pending != want.pending) violation("latch_report differs from ptgs.h's table", 0, (int)(report * 8 + pending * 2 + ok));
      }
  // both reports from one frame, in turn: PTGS_EBADIDS, PTGS_EINCOMPLETE, PTGS_OK (a failing call between
  // them returns its own code and drops nothing)
  SplatLatch l = latch_report(0, true, kSplatReportIncomplete | kSplatReportBadIds);
  bool chain = l.code == SplatCode::BadIds;
  l = latch_report(l.pending, false, 0);
  chain = chain && l.code == SplatCode::Own;
  l = latch_report(l.pending, true, 0);
  chain = chain && l.code == SplatCode::Incomplete;
  l = latch_report(l.pending, true, 0);
  chain = chain && l.code == SplatCode::Ok && l.pending == 0;
  if (!chain) violation("the two reports of one frame were not returned in turn", 0, 0);
}

void check_depth() {
  const struct {
    const char* env;
    uint32_t depth;
  } cases[] = {{nullptr, 3}, {"", 2}, {"0", 2}, {"2", 2}, {"3", 3}, {"4", 4}, {"9", 4}, {"-1", 2}, {"x", 2}};
  for (const auto& c : cases) {
    ++g_cases;
    if (splat_ring_depth(c.env) != c.depth) violation("splat_ring_depth", c.depth, 0);
  }
}

}  // namespace

int main() {
  static_assert(sizeof(SplatRun) == 16 + kSplatLookBack * 16, "SplatRun has padding: the bytewise comparison would read it");
  for (uint32_t depth = 2; depth <= kSplatRingMax; ++depth) {
    SplatRun run;
    run.depth = depth;
    walk(run, Model{}, depth, 0);
  }
  check_latch();
  check_depth();
  // 3 depths x (5 + 5^2 + .. + 5^9) steps, 32 latch cases, 9 depth strings
  long long steps = 0, p = 1;
  for (int i = 1; i <= kCalls; ++i) steps += (p *= kChoices);
  const long long expected = 3 * steps + 32 + 9;
  if (g_cases != expected) violation("the enumeration's count is not the arithmetic one", 0, 0);
  printf("splat_run_check cases %lld violations %lld\n", g_cases, g_violations);
  return g_violations ? 1 : 0;
}
