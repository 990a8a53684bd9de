// bvh_tries_check — stand-alone host check of the scene upload's BVH try policy (csrc/bvh_tries.h).
//
//   bvh_tries_check [tris.bin ...]
//
// Always: the parsing rules of PTGS_BVH_TRIES and PTGS_BVH_NODE_LIMIT, and the policy over a stub builder that
// counts what it acquires and releases the way the GPU builders of api.cpp own their device buffers. Per
// tris.bin (float32 triangles, 9 floats each): the policy over the host builder (bvh.cpp) against a reference
// computed by calling build_bvh / collapse_bvh4 for every try of the default list directly. Prints, per file,
// "policy <file> depth2 D needs N0 N1 N2 N3 stop K" (K: the try that stack_total = smallest need + 1 keeps)
// and at the end "bvh_tries_check violations V". Exit status 1 when V > 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "bvh.h"
#include "bvh_tries.h"

using namespace ptgs;

static unsigned long long g_viol = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      ++g_viol;                                                      \
      printf("  line %d: %s\n", __LINE__, #cond);                    \
    }                                                                \
  } while (0)

static const uint32_t S = 39u;  // the traversal stack's LDS entries (pt_device.h PTGS_STACK)

static bool same(const BvhTry& a, const BvhTry& b) { return a.leaf == b.leaf && a.fan == b.fan && a.depth == b.depth; }
static bool same(const std::vector<BvhTry>& a, const std::vector<BvhTry>& b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); ++i)
    if (!same(a[i], b[i])) return false;
  return true;
}

static void check_parsing() {
  const std::vector<BvhTry> def = default_bvh_tries(S);
  CHECK(same(def, {{3, 4, 38}, {4, 4, 38}, {3, 3, 38}, {3, 2, 38}}));
  CHECK(same(lbvh_bvh_tries(S), {{0, 4, 38}, {0, 3, 38}, {0, 2, 38}}));
  CHECK(same(parse_bvh_tries(nullptr, S), def));
  CHECK(same(parse_bvh_tries("", S), def));
  CHECK(same(parse_bvh_tries("2:4:38", S), {{2, 4, 38}}));
  CHECK(same(parse_bvh_tries("3:4:38,4:4:30", S), {{3, 4, 38}, {4, 4, 30}}));
  CHECK(same(parse_bvh_tries("0:4:38", S), def));   // leaf below 1
  CHECK(same(parse_bvh_tries("17:4:38", S), def));  // leaf above 16
  CHECK(same(parse_bvh_tries("3:5:38", S), def));   // fan above 4
  CHECK(same(parse_bvh_tries("3:1:38", S), def));   // fan below 2
  CHECK(same(parse_bvh_tries("3:4:39", S), def));   // depth at the LDS stack
  CHECK(same(parse_bvh_tries("3:4:0", S), def));    // depth below 1
  CHECK(same(parse_bvh_tries("junk", S), def));
  CHECK(same(parse_bvh_tries("3:4", S), def));
  CHECK(same(parse_bvh_tries("0:4:38,2:4:38", S), {{2, 4, 38}}));
  CHECK(same(parse_bvh_tries("2:4:38,3:5:38", S), {{2, 4, 38}}));
  CHECK(same(parse_bvh_tries("junk,16:2:1,,1:3:38", S), {{16, 2, 1}, {1, 3, 38}}));
  CHECK(same(parse_bvh_tries("3:4:20", 20u), default_bvh_tries(20u)));  // (the depth bound is the argument)
  CHECK(same(parse_bvh_tries("3:4:19", 20u), {{3, 4, 19}}));

  const uint32_t hw = 0x7fffffffu / 128u;
  CHECK(hw == 16777215u);
  CHECK(bvh_node_limit(nullptr) == hw);
  CHECK(bvh_node_limit("0") == hw);
  CHECK(bvh_node_limit("1") == 1u);
  CHECK(bvh_node_limit("16777214") == 16777214u);
  CHECK(bvh_node_limit("16777215") == hw);
  CHECK(bvh_node_limit("16777216") == hw);
  CHECK(bvh_node_limit("4000000000") == hw);
  CHECK(bvh_node_limit("junk") == hw);
}

// ---- the policy over the host builder -----------------------------------------------------------------

// api.cpp's HostSahBuilder, restated
struct HostBuilder {
  const std::vector<BuildTri>& tris;
  BvhOut bvh;
  std::vector<float> n4;
  uint32_t num4 = 0;
  BvhStep build(int leaf, uint32_t depth, uint32_t stack_lds) {
    build_bvh(tris, leaf, depth, bvh);
    return bvh.depth >= stack_lds ? BvhStep::TooDeep : BvhStep::Ok;
  }
  BvhStep collapse(int fan, uint32_t& need, uint32_t& depth4) {
    need = 0;
    collapse_bvh4(bvh.nodes, n4, num4, need, depth4, fan);
    return BvhStep::Ok;
  }
};

struct RefTree {
  std::vector<float> n4, tris;
  uint32_t num4 = 0, need = 0, dep4 = 0, depth2 = 0;
};

static bool same_tree(const HostBuilder& b, const BvhTriesResult& r, const RefTree& ref) {
  return b.num4 == ref.num4 && r.need == ref.need && r.depth4 == ref.dep4 && b.n4.size() == ref.n4.size() &&
         std::memcmp(b.n4.data(), ref.n4.data(), ref.n4.size() * sizeof(float)) == 0 &&
         b.bvh.tris.size() == ref.tris.size() &&
         std::memcmp(b.bvh.tris.data(), ref.tris.data(), ref.tris.size() * sizeof(float)) == 0;
}

static int builds_up_to(const std::vector<BvhTry>& t, size_t k) {
  int n = 0;
  for (size_t i = 0; i <= k; ++i)
    if (i == 0 || t[i].leaf != t[i - 1].leaf || t[i].depth != t[i - 1].depth) ++n;
  return n;
}

static void check_host_policy(const char* path) {
  FILE* fp = fopen(path, "rb");
  if (!fp) { perror(path); ++g_viol; return; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  std::vector<BuildTri> tris(raw.size() / 9);
  for (size_t i = 0; i < tris.size(); ++i) {
    BuildTri& t = tris[i];
    std::memcpy(t.v0, &raw[9 * i], 12);
    std::memcpy(t.v1, &raw[9 * i + 3], 12);
    std::memcpy(t.v2, &raw[9 * i + 6], 12);
    t.mesh = 0; t.prim = (uint32_t)i; t.gid = (uint32_t)i; t.flags = 0;
  }

  // the reference: every try of the default list, built and collapsed directly
  const std::vector<BvhTry> tl = default_bvh_tries(S);
  std::vector<RefTree> ref(tl.size());
  uint32_t lo = ~0u, hi = 0;
  for (size_t k = 0; k < tl.size(); ++k) {
    BvhOut bvh;
    build_bvh(tris, tl[k].leaf, tl[k].depth, bvh);
    collapse_bvh4(bvh.nodes, ref[k].n4, ref[k].num4, ref[k].need, ref[k].dep4, tl[k].fan);
    ref[k].tris.swap(bvh.tris);
    ref[k].depth2 = bvh.depth;
    lo = ref[k].need < lo ? ref[k].need : lo;
    hi = ref[k].need > hi ? ref[k].need : hi;
  }
  size_t stop = 0;
  while (ref[stop].need != lo) ++stop;
  printf("policy %s depth2 %u needs", path, ref[0].depth2);
  for (const RefTree& r : ref) printf(" %u", r.need);
  printf(" stop %zu\n", stop);

  int logged = 0;
  auto log = [&logged](const BvhTry&, uint32_t, uint32_t) { ++logged; };
  {  // (a) above every need: the first try, one build, one collapse
    HostBuilder b{tris};
    const BvhTriesResult r = run_bvh_tries(b, tl, S, hi + 1u, log);
    CHECK(r.fit == BvhFit::Fits && same(r.kept, tl[0]) && r.builds == 1 && r.collapses == 1 && logged == 1);
    CHECK(same_tree(b, r, ref[0]));
  }
  {  // (b) the smallest need + 1: the first try that reaches the smallest need
    logged = 0;
    HostBuilder b{tris};
    const BvhTriesResult r = run_bvh_tries(b, tl, S, lo + 1u, log);
    CHECK(stop >= 1);  // (otherwise this is case (a) again: the test's input must make a later try the first fit)
    CHECK(r.fit == BvhFit::Fits && same(r.kept, tl[stop]) && r.collapses == (int)stop + 1 && logged == r.collapses);
    CHECK(r.builds == builds_up_to(tl, stop));
    CHECK(same_tree(b, r, ref[stop]));
  }
  for (size_t k = 0; k < tl.size(); ++k) {  // every try's need + 1: the first try at or below that need
    HostBuilder b{tris};
    const BvhTriesResult r = run_bvh_tries(b, tl, S, ref[k].need + 1u, log);
    size_t first = 0;
    while (ref[first].need > ref[k].need) ++first;
    CHECK(r.fit == BvhFit::Fits && same(r.kept, tl[first]) && r.collapses == (int)first + 1);
    CHECK(r.builds == builds_up_to(tl, first) && same_tree(b, r, ref[first]));
  }
  {  // the smallest need itself: nothing fits, every try was collapsed, the last one is kept
    logged = 0;
    HostBuilder b{tris};
    const BvhTriesResult r = run_bvh_tries(b, tl, S, lo, log);
    CHECK(r.fit == BvhFit::DoesNotFit && same(r.kept, tl.back()) && r.collapses == (int)tl.size() && logged == r.collapses);
    CHECK(r.builds == builds_up_to(tl, tl.size() - 1));
    CHECK(same_tree(b, r, ref.back()));
  }
  {  // an LDS stack no deeper than the first BVH2: ends after that one build, nothing collapsed
    logged = 0;
    HostBuilder b{tris};
    const BvhTriesResult r = run_bvh_tries(b, tl, ref[0].depth2, hi + 1u, log);
    CHECK(r.fit == BvhFit::TooDeep && r.builds == 1 && r.collapses == 0 && logged == 0);
    CHECK(same(r.kept, BvhTry{0, 0, 0}) && b.bvh.depth == ref[0].depth2);
    HostBuilder b1{tris};  // one entry more holds it
    const BvhTriesResult r1 = run_bvh_tries(b1, tl, ref[0].depth2 + 1u, hi + 1u, log);
    CHECK(r1.fit == BvhFit::Fits && r1.builds == 1 && r1.collapses == 1);
  }
}

// ---- the policy over a stub that owns counted buffers as api.cpp's GPU builders own device memory --------

struct Pool {
  int acquired = 0, released = 0, bad = 0;
  std::set<int> live;
  int acquire() {
    live.insert(++acquired);
    return acquired;
  }
  void release(int id) {  // (0: nothing held, as hipFree(nullptr))
    if (id == 0) return;
    if (live.erase(id) != 1) ++bad;  // released twice, or never acquired
    ++released;
  }
};

struct StubBuilder {
  Pool& pool;
  int fail_build = 0;                   // this build (1-based) ends with build_status ...
  BvhStep build_status = BvhStep::Error;
  bool fail_filled = false;             // ... and leaves the BVH2's buffers behind (bvh_gpu.h: not supported, out filled)
  int fail_collapse = 0;                // this collapse (1-based) ends with Error
  std::vector<uint32_t> needs;          // per collapse (the last repeats)
  int bvh2[3] = {0, 0, 0}, n4 = 0, builds = 0, collapses = 0;
  explicit StubBuilder(Pool& p) : pool(p) {}
  ~StubBuilder() {
    release_bvh2();
    pool.release(n4);
  }
  void release_bvh2() {
    for (int& b : bvh2) { pool.release(b); b = 0; }
  }
  BvhStep build(int, uint32_t, uint32_t) {
    release_bvh2();
    const bool fails = ++builds == fail_build;
    if (!fails || fail_filled)
      for (int& b : bvh2) b = pool.acquire();
    return fails ? build_status : BvhStep::Ok;
  }
  BvhStep collapse(int, uint32_t& need, uint32_t& depth4) {
    if (bvh2[0] == 0) ++pool.bad;  // a collapse with no BVH2
    pool.release(n4);
    n4 = 0;
    if (++collapses == fail_collapse) return BvhStep::Error;
    n4 = pool.acquire();
    need = needs[std::min((size_t)collapses, needs.size()) - 1];
    depth4 = 7;
    return BvhStep::Ok;
  }
  std::set<int> hand_over() {  // the collapsed nodes, the records and the flags survive the builder
    pool.release(bvh2[0]);
    const std::set<int> kept = {n4, bvh2[1], bvh2[2]};
    bvh2[0] = bvh2[1] = bvh2[2] = n4 = 0;
    return kept;
  }
};

static void check_stub_policy() {
  const std::vector<BvhTry> def = default_bvh_tries(S), lb = lbvh_bvh_tries(S);
  const uint32_t total = 48u;
  auto nolog = [](const BvhTry&, uint32_t, uint32_t) {};
  {  // an error on the n-th build
    for (int nth : {1, 2, 3}) {
      Pool pool;
      {
        StubBuilder b(pool);
        b.fail_build = nth;
        b.needs = {total};
        const BvhTriesResult r = run_bvh_tries(b, def, S, total, nolog);
        CHECK(r.fit == BvhFit::Error && r.builds == nth && r.collapses == nth - 1);
        CHECK(nth == 1 ? same(r.kept, BvhTry{0, 0, 0}) : same(r.kept, def[nth - 2]));
      }
      CHECK(pool.live.empty() && pool.acquired == pool.released && pool.bad == 0 && pool.acquired == 4 * (nth - 1));
    }
  }
  {  // not supported on the first build, with and without the buffers left behind
    for (bool filled : {false, true}) {
      Pool pool;
      {
        StubBuilder b(pool);
        b.fail_build = 1;
        b.build_status = BvhStep::NotSupported;
        b.fail_filled = filled;
        b.needs = {0};
        const BvhTriesResult r = run_bvh_tries(b, def, S, total, nolog);
        CHECK(r.fit == BvhFit::NotSupported && r.builds == 1 && r.collapses == 0);
        CHECK((int)pool.live.size() == (filled ? 3 : 0));
      }
      CHECK(pool.live.empty() && pool.acquired == pool.released && pool.bad == 0 && pool.acquired == (filled ? 3 : 0));
    }
  }
  {  // an error in a collapse after a successful build: the first, and one after a fan-out that did not fit
    for (int nth : {1, 3}) {
      Pool pool;
      {
        StubBuilder b(pool);
        b.fail_collapse = nth;
        b.needs = {total + 5u};
        const BvhTriesResult r = run_bvh_tries(b, lb, S, total, nolog);
        CHECK(r.fit == BvhFit::Error && r.builds == 1 && r.collapses == nth && same(r.kept, lb[nth - 1]));
      }
      CHECK(pool.live.empty() && pool.acquired == pool.released && pool.bad == 0 && pool.acquired == 3 + nth - 1);
    }
  }
  {  // the LBVH's list with a need that never fits: one build, three collapses
    Pool pool;
    int logged = 0;
    {
      StubBuilder b(pool);
      b.needs = {total + 9u, total + 1u, total};
      const BvhTriesResult r =
          run_bvh_tries(b, lb, S, total, [&logged](const BvhTry&, uint32_t, uint32_t) { ++logged; });
      CHECK(r.fit == BvhFit::DoesNotFit && r.builds == 1 && r.collapses == 3 && logged == 3);
      CHECK(same(r.kept, BvhTry{0, 2, S - 1}) && r.need == total && r.depth4 == 7u);
      CHECK(pool.live.size() == 4u);  // one BVH2 and the latest collapse only
    }
    CHECK(pool.live.empty() && pool.acquired == pool.released && pool.bad == 0 && pool.acquired == 3 + 3);
  }
  {  // a fit at the first try and one after a rebuild, handed over: exactly the handed-over set survives
    for (int fit_at : {1, 2, 4}) {
      Pool pool;
      std::set<int> kept;
      {
        StubBuilder b(pool);
        b.needs.assign((size_t)fit_at, total);
        b.needs.back() = total - 1u;
        const BvhTriesResult r = run_bvh_tries(b, def, S, total, nolog);
        CHECK(r.fit == BvhFit::Fits && r.collapses == fit_at && same(r.kept, def[fit_at - 1]) && r.need == total - 1u);
        CHECK(r.builds == builds_up_to(def, (size_t)fit_at - 1));
        kept = b.hand_over();
      }
      CHECK(kept.size() == 3u && pool.live == kept && pool.acquired - pool.released == 3 && pool.bad == 0);
    }
  }
}

int main(int argc, char** argv) {
  check_parsing();
  check_stub_policy();
  for (int i = 1; i < argc; ++i) check_host_policy(argv[i]);
  printf("bvh_tries_check violations %llu\n", g_viol);
  return g_viol ? 1 : 0;
}
