// tree_budget_check — stand-alone host check of the stack-budgeted collapse (bvh_opt.h collapse_bvh4_budget) and
// of the optimiser's use of it, for what tree_opt_check (which sees only the upload's call) cannot see.
//
//   tree_budget_check <tris.bin> <leaf> <fan> <depth> [quick]
//
// tris.bin holds float32 triangles (9 floats each, at least two). The program builds the host BVH2 as the scene
// upload does (build_bvh) and checks, violations when one fails:
//   - a budget that never binds (the greedy need + 1, and 1 << 20) gives collapse_bvh4's bytes, need and depth;
//   - every limit from the greedy need down to bvh2_height + 1 gives a tree whose need, recomputed by a fresh
//     pass over the output, is below the limit and is the reported one; its leaf links are the greedy tree's,
//     each as often; every node but the root is linked exactly once; slots 0 and 1 are never empty; every
//     interior child's box holds the boxes in the node it links;
//   - the limit bvh2_height (and 1, and 0) returns false with no nodes;
//   - optimize_bvh4 on the canonical nodes: with the limit at the reinserted BVH2's height + 1 it applies, at
//     the canonical fan-out, with need < limit; with the limit at that height it reports "not applied"; with two
//     limits (height, greedy need + 1) it meets the second and says so; the same call twice gives the same bytes.
// `quick` walks the limits in steps (large meshes). Prints one line of "name value" pairs; exit status 1 when
// violations > 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"
#include "bvh_opt.h"

using namespace ptgs;

static unsigned long long g_viol = 0;
static void violation(const char* what, uint32_t limit) {
  if (g_viol < 8) fprintf(stderr, "tree_budget_check: %s (limit %u)\n", what, limit);
  ++g_viol;
}

static int32_t link_of(const std::vector<float>& n4, uint32_t i, int j) {
  int32_t l;
  std::memcpy(&l, &n4[32 * (size_t)i + 24 + j], 4);
  return l;
}

// need, depth, sorted leaf links of a 4-wide tree; structure violations
static void inspect(const std::vector<float>& n4, uint32_t num, uint32_t limit, uint32_t& need, uint32_t& depth,
                    std::vector<int32_t>& leaves) {
  std::vector<uint32_t> nd(num, 0), dp(num, 1), linked(num, 0);
  leaves.clear();
  for (size_t i = num; i-- > 0;) {  // children after parents
    uint32_t cnt = 0, m = 0, d = 0;
    for (int j = 0; j < 4; ++j) {
      const int32_t l = link_of(n4, (uint32_t)i, j);
      if (l == 0) {
        if (j < 2) violation("an empty slot 0 or 1", limit);
        continue;
      }
      ++cnt;
      if (l < 0) { leaves.push_back(l); continue; }
      if ((uint32_t)l >= num || (size_t)l <= i) { violation("an interior link out of range or not after its parent", limit); continue; }
      ++linked[(size_t)l];
      m = std::max(m, nd[(size_t)l]);
      d = std::max(d, dp[(size_t)l]);
      // the child's stored box is the union of the boxes in the linked node
      const float* c = &n4[32 * (size_t)l];
      for (int a = 0; a < 3; ++a) {
        float lo = 1e30f, hi = -1e30f;
        for (int k = 0; k < 4; ++k)
          if (link_of(n4, (uint32_t)l, k) != 0) { lo = std::min(lo, c[(2 * a) * 4 + k]); hi = std::max(hi, c[(2 * a + 1) * 4 + k]); }
        if (lo < n4[32 * i + (2 * a) * 4 + j] || hi > n4[32 * i + (2 * a + 1) * 4 + j]) violation("a child box does not hold the boxes below it", limit);
      }
    }
    nd[i] = cnt ? cnt - 1 + m : 0;
    dp[i] = 1 + d;
  }
  for (uint32_t i = 1; i < num; ++i)
    if (linked[i] != 1) violation("a node is not linked exactly once", limit);
  need = num ? nd[0] : 0;
  depth = num ? dp[0] : 0;
  std::sort(leaves.begin(), leaves.end());
}

static bool same_bytes(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}

int main(int argc, char** argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: tree_budget_check <tris.bin> <leaf> <fan> <depth> [quick]\n");
    return 2;
  }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leafsz = atoi(argv[2]), fan = atoi(argv[3]);
  const uint32_t depth = (uint32_t)atoi(argv[4]);
  const bool quick = argc > 5;
  std::vector<BuildTri> tris(raw.size() / 9);
  for (size_t i = 0; i < tris.size(); ++i) {
    BuildTri& t = tris[i];
    std::memcpy(t.v0, &raw[9 * i], 12);
    std::memcpy(t.v1, &raw[9 * i + 3], 12);
    std::memcpy(t.v2, &raw[9 * i + 6], 12);
    t.mesh = 0; t.prim = (uint32_t)i; t.gid = (uint32_t)i; t.flags = 0;
  }
  BvhOut bvh;
  build_bvh(tris, leafsz, depth, bvh);
  if (bvh.nodes.empty()) {
    fprintf(stderr, "tree_budget_check: no BVH2 node (fewer than two leaves)\n");
    return 2;
  }
  const uint32_t h2 = bvh2_height(bvh.nodes);

  std::vector<float> greedy, got;
  std::vector<int32_t> leaves_g, leaves;
  uint32_t num_g = 0, need_g = 0, dep_g = 0, num = 0, need = 0, dep = 0, fneed = 0, fdep = 0;
  collapse_bvh4(bvh.nodes, greedy, num_g, need_g, dep_g, fan);
  inspect(greedy, num_g, 0, fneed, fdep, leaves_g);
  if (fneed != need_g || fdep != dep_g) violation("the fresh pass disagrees with collapse_bvh4", 0);
  if (need_g < h2) violation("the greedy need is below the BVH2's height", 0);

  for (const uint32_t limit : {need_g + 1u, 1u << 20}) {  // never binds
    if (!collapse_bvh4_budget(bvh.nodes, got, num, need, dep, fan, limit) || !same_bytes(got, greedy) || num != num_g ||
        need != need_g || dep != dep_g)
      violation("a budget that does not bind: not the greedy collapse", limit);
  }
  uint32_t limits_run = 0, nodes_tight = 0, need_tight = 0, depth_tight = 0;
  const uint32_t step = quick ? std::max(1u, (need_g - h2) / 4u) : 1u;
  for (uint32_t limit = need_g; limit > h2;) {
    if (!collapse_bvh4_budget(bvh.nodes, got, num, need, dep, fan, limit)) {
      violation("a feasible budget is refused", limit);
    } else {
      inspect(got, num, limit, fneed, fdep, leaves);
      if ((size_t)num * 32 != got.size()) violation("the node count", limit);
      if (fneed != need || fdep != dep) violation("the reported need or depth", limit);
      if (!(need < limit)) violation("the need reaches the limit", limit);
      if (leaves != leaves_g) violation("the leaf links differ from the greedy tree's", limit);
      nodes_tight = num; need_tight = need; depth_tight = dep;
    }
    ++limits_run;
    if (limit == h2 + 1u) break;
    limit = limit - h2 - 1u < step ? h2 + 1u : limit - step;  // (the tightest limit is always run)
  }
  for (const uint32_t limit : {h2, 1u, 0u}) {
    if (limit > h2) continue;
    if (collapse_bvh4_budget(bvh.nodes, got, num, need, dep, fan, limit) || !got.empty())
      violation("an infeasible budget is not refused", limit);
  }

  // the optimiser: the same rule on its reinserted BVH2
  TreeOptInfo probe, info, info2;
  std::vector<float> out, out2;
  const bool probed = optimize_bvh4(greedy.data(), num_g, fan, 1u << 20, out, probe);
  uint32_t need_at = 0, applied_at = 0, applied_below = 0, limit_two = 0;
  if (probed && probe.height2 >= 1u) {
    const uint32_t ho = probe.height2;
    if (probe.need < ho) violation("the optimised greedy need is below the reinserted BVH2's height", 0);
    applied_at = optimize_bvh4(greedy.data(), num_g, fan, ho + 1u, out, info) ? 1u : 0u;
    if (!applied_at || info.fan != (uint32_t)std::max(2, std::min(4, fan)) || !(info.need < ho + 1u) || info.limit != ho + 1u) {
      violation("the optimiser under the tightest feasible limit", ho + 1u);
    } else {
      inspect(out, info.num_nodes, ho + 1u, fneed, fdep, leaves);
      if (fneed != info.need || fdep != info.depth || leaves != leaves_g) violation("the optimiser's budgeted tree", ho + 1u);
      need_at = info.need;
      if (!optimize_bvh4(greedy.data(), num_g, fan, ho + 1u, out2, info2) || !same_bytes(out, out2) || info2.need != info.need)
        violation("two runs differ", ho + 1u);
    }
    applied_below = optimize_bvh4(greedy.data(), num_g, fan, ho, out, info) ? 1u : 0u;
    if (applied_below || !out.empty()) violation("the optimiser under an infeasible limit applies", ho);
    const uint32_t two[2] = {ho, probe.need + 1u};
    if (!optimize_bvh4(greedy.data(), num_g, fan, two, 2, out, info) || info.limit != two[1] || info.need != probe.need)
      violation("two limits: the second is not the one met", two[1]);
    limit_two = info.limit;
  }

  printf("tree_budget_check: violations %llu triangles %zu height2 %u nodes_greedy %u need_greedy %u depth_greedy %u "
         "limits_run %u nodes_tight %u need_tight %u depth_tight %u opt_applied %u opt_height2 %u opt_need_greedy %u "
         "opt_need_tight %u opt_applied_tight %u opt_applied_below %u opt_limit_two %u\n",
         g_viol, tris.size(), h2, num_g, need_g, dep_g, limits_run, nodes_tight, need_tight, depth_tight,
         probed ? 1u : 0u, probe.height2, probe.need, need_at, applied_at, applied_below, limit_two);
  return g_viol ? 1 : 0;
}
