// bvh_tries.h — which tree shapes the scene upload tries, and in what order: plain values in, plain values
// out. No HIP include: tests/native/bvh_tries_check.cpp builds it with a host compiler alone. The upload's
// three builders (api.cpp: host SAH, GPU SAH, GPU LBVH) run under the one loop below; the traversal's stack
// capacities (pt_device.h PTGS_STACK, PTGS_STACK_TOTAL) are arguments.
#pragma once

#include <stdint.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

// Largest BVH leaf (triangles). C3 at 64 spp (tools/ab_pt.py, interleaved): 1 -> 3 602, 2 -> 4 849,
// 3 -> 4 836, 4 -> 4 463, 8 -> -10% Mrays/s; 3 keeps the tree a level shallower than 2 for the
// traversal-stack budget of large meshes
#ifndef PTGS_BVH_LEAF
#define PTGS_BVH_LEAF 3
#endif

namespace ptgs {

// (leaf size, fan-out) tried in this order until the tree's worst-case stack need fits the whole stack
// (LDS + overflow): a scene whose 3-triangle-leaf tree is too deep for a 4-wide collapse is rebuilt with
// 4-triangle leaves before the fan-out is narrowed (a 2-wide fallback traced C5 at 1.38 Grays/s, the
// 4-triangle-leaf 4-wide tree at ~2.1; with the stack overflow C5 keeps 3-triangle leaves: need 40)
// Each try also carries the SAH build's depth budget (bvh.cpp: past it, balanced splits).
struct BvhTry {
  int leaf, fan;
  uint32_t depth;
};

// stack_lds: the traversal stack's LDS entries; a BVH2 must stay below it (a 2-wide "collapse" needs its depth)
inline std::vector<BvhTry> default_bvh_tries(uint32_t stack_lds) {
  return {{PTGS_BVH_LEAF, 4, stack_lds - 1}, {PTGS_BVH_LEAF + 1, 4, stack_lds - 1},
          {PTGS_BVH_LEAF, 3, stack_lds - 1}, {PTGS_BVH_LEAF, 2, stack_lds - 1}};
}
// the LBVH has fixed leaves (leaf 0): one build, fan-out 4, 3, 2
inline std::vector<BvhTry> lbvh_bvh_tries(uint32_t stack_lds) {
  return {{0, 4, stack_lds - 1}, {0, 3, stack_lds - 1}, {0, 2, stack_lds - 1}};
}
// PTGS_BVH_TRIES="leaf:fan:depth,..." replaces the default list (A/B of tree shapes: tools/ab_pt.py
// AB_SCENE=c5). Entries outside leaf 1..16, fan 2..4, depth 1..stack_lds - 1 are dropped; none left (or
// env null): the default list.
inline std::vector<BvhTry> parse_bvh_tries(const char* env, uint32_t stack_lds) {
  std::vector<BvhTry> v;
  if (env) {
    for (const char* p = env; *p;) {
      int l = 0, f = 0;
      unsigned d = 0;
      if (sscanf(p, "%d:%d:%u", &l, &f, &d) == 3 && l >= 1 && l <= 16 && f >= 2 && f <= 4 && d >= 1 && d < stack_lds)
        v.push_back({l, f, d});
      while (*p && *p != ',') ++p;
      if (*p == ',') ++p;
    }
  }
  if (v.empty()) v = default_bvh_tries(stack_lds);
  return v;
}

// 4-wide nodes the traversal can address: 128-B nodes behind 31-bit byte offsets (pt_device.h box4).
// PTGS_BVH_NODE_LIMIT lowers it (the guard's GPU test).
#define PTGS_NODE4_BYTES 128u
inline uint32_t bvh_node_limit(const char* env) {
  const uint32_t hw = 0x7fffffffu / PTGS_NODE4_BYTES;
  const unsigned long v = env ? strtoul(env, nullptr, 10) : 0ul;
  return v && v < hw ? (uint32_t)v : hw;
}

// What a builder's step reports, and what the tries come to. TooDeep: a BVH2 at or beyond stack_lds (the
// host builder's: no later try is made; the GPU builders report theirs as NotSupported).
enum class BvhStep { Ok, NotSupported, Error, TooDeep };
enum class BvhFit { Fits, DoesNotFit, NotSupported, Error, TooDeep };
struct BvhTriesResult {
  BvhFit fit;
  BvhTry kept;              // the try whose collapse ran last ({0, 0, 0}: none ran)
  uint32_t need, depth4;    // that collapse's worst-case stack need and 4-wide depth
  int builds, collapses;    // steps started
};

// Runs the tries over a builder until a collapsed tree's stack need is below stack_total:
//   BvhStep builder.build(int leaf, uint32_t depth_budget, uint32_t stack_lds)   (re)builds the BVH2
//   BvhStep builder.collapse(int fan, uint32_t& need, uint32_t& depth4)          collapses the current BVH2
// The BVH2 is rebuilt only when the leaf size or the depth budget changes; a step that is not Ok ends the
// run with its status. log(try, depth4, need) is called after every collapse that succeeded.
template <class Builder, class Log>
BvhTriesResult run_bvh_tries(Builder& builder, const std::vector<BvhTry>& tries, uint32_t stack_lds,
                             uint32_t stack_total, Log&& log) {
  BvhTriesResult r{BvhFit::DoesNotFit, BvhTry{0, 0, 0}, stack_total, 0, 0, 0};
  auto ended = [&r](BvhStep s) {
    r.fit = s == BvhStep::NotSupported ? BvhFit::NotSupported : s == BvhStep::Error ? BvhFit::Error : BvhFit::TooDeep;
    return r;
  };
  int built_leaf = -1;
  uint32_t built_depth = 0;
  for (const BvhTry& t : tries) {
    if (t.leaf != built_leaf || t.depth != built_depth) {
      ++r.builds;
      const BvhStep s = builder.build(t.leaf, t.depth, stack_lds);
      if (s != BvhStep::Ok) return ended(s);
      built_leaf = t.leaf;
      built_depth = t.depth;
    }
    ++r.collapses;
    r.kept = t;
    const BvhStep s = builder.collapse(t.fan, r.need, r.depth4);
    if (s != BvhStep::Ok) return ended(s);
    log(t, r.depth4, r.need);
    if (r.need < stack_total) {
      r.fit = BvhFit::Fits;
      break;
    }
  }
  return r;
}

}  // namespace ptgs
