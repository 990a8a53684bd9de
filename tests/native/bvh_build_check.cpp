// bvh_build_check — stand-alone host check of the binned-SAH builder and the 4-wide collapse (bvh.cpp),
// the reference the GPU builders are compared with.
//
//   bvh_build_check <tris.bin> <leaf> <fan> <depth> [dump.bin]
//
// tris.bin holds float32 triangles (9 floats each). The program builds the tree as the scene upload does
// (build_bvh with the leaf size and depth budget, collapse_bvh4 with the fan-out) and checks, on the BVH2
// and on the 4-wide nodes:
//   - every triangle lies in exactly one leaf, a leaf holds 1 .. <leaf> triangles, no leaf range leaves
//     the triangle array, the records' ids are a permutation;
//   - every child box contains all vertices of all triangles below it (exactly: boxes are padded outward);
//   - the BVH2's depth equals the reported one and does not exceed the depth budget;
//   - a split the budget forces to be balanced (bvh.cpp: d + ceil(log2(n / leaf)) + 1 >= budget) sends
//     n / 2 triangles left, and no left centroid lies beyond a right one along the widest centroid axis;
//   - the reported 4-wide node count, stack need and depth equal a recomputation over the 4-wide nodes;
//   - every 4-wide node has 2 .. <fan> occupied slots, in front; empty slots hold the 1e30 point boxes and
//     link 0; every node but the root is linked once, from a lower index (breadth-first numbering).
// dump.bin, when given, receives the 4-wide node count (u32), the 4-wide nodes and the triangle records
// (for the tests' numpy restatement of these conditions, which the GPU tests apply to device trees).
// Prints one line of "name value" pairs; `balanced` counts the budget-forced splits, `sah` the others.
// Exit status 1 when violations > 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"

using namespace ptgs;

namespace {

struct VBox {
  float lo[3], hi[3];
  VBox() {
    for (int a = 0; a < 3; ++a) { lo[a] = INFINITY; hi[a] = -INFINITY; }
  }
  void grow(const float* p) {
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); }
  }
  void grow(const VBox& b) {
    for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); }
  }
};

struct Check {
  const std::vector<BuildTri>& tris;
  const BvhOut& bvh;
  int leaf;
  uint32_t budget;
  unsigned long long viol = 0, balanced = 0, sah = 0, leaves = 0;
  uint32_t depth2 = 0, max_leaf = 0;
  std::vector<uint32_t> cover;  // leaves that hold record k
  std::vector<uint32_t> gid;    // record k's triangle

  Check(const std::vector<BuildTri>& t, const BvhOut& b, int l, uint32_t d) : tris(t), bvh(b), leaf(l), budget(d) {}

  void fail(const char* what, long long a, long long b) {
    if (viol++ < 20) fprintf(stderr, "bvh_build_check: %s (%lld, %lld)\n", what, a, b);
  }

  // vertex bounds of the records [first, first + count); marks them covered when `mark`
  bool leaf_range(int32_t link, uint32_t& first, uint32_t& count) {
    const uint32_t L = ~(uint32_t)link;
    first = L & 0x07ffffffu;
    count = (L >> 27) + 1u;
    if ((uint64_t)first + count > tris.size()) { fail("leaf range leaves the array", first, count); return false; }
    if (count > (uint32_t)leaf) fail("leaf larger than the leaf size", count, leaf);
    return true;
  }
  VBox leaf_box(uint32_t first, uint32_t count) const {
    VBox b;
    for (uint32_t k = first; k < first + count; ++k) {
      const BuildTri& t = tris[gid[k]];
      b.grow(t.v0); b.grow(t.v1); b.grow(t.v2);
    }
    return b;
  }
  void contains(const float* lo, const float* hi, const VBox& v, const char* what, long long node) {
    for (int a = 0; a < 3; ++a)
      if (!(lo[a] <= v.lo[a]) || !(hi[a] >= v.hi[a])) { fail(what, node, a); return; }
  }
  // bvh.cpp Ref::c of record k
  float centroid(uint32_t k, int a) const {
    const BuildTri& t = tris[gid[k]];
    const float lo = std::min(std::min(t.v0[a], t.v1[a]), t.v2[a]), hi = std::max(std::max(t.v0[a], t.v1[a]), t.v2[a]);
    return 0.5f * (lo + hi);
  }

  // BVH2 subtree below `link` at depth d: its records [begin, end) and vertex bounds
  VBox walk2(int32_t link, uint32_t d, uint32_t& begin, uint32_t& end) {
    depth2 = std::max(depth2, d);
    if (link < 0) {
      uint32_t first = 0, count = 0;
      if (!leaf_range(link, first, count)) { begin = end = 0; return VBox(); }
      ++leaves;
      max_leaf = std::max(max_leaf, count);
      for (uint32_t k = first; k < first + count; ++k) ++cover[k];
      begin = first;
      end = first + count;
      return leaf_box(first, count);
    }
    if ((uint32_t)link >= bvh.num_nodes || d > 64) { fail("bad BVH2 link", link, d); begin = end = 0; return VBox(); }
    const float* n = &bvh.nodes[16 * (size_t)link];
    int32_t c[2];
    std::memcpy(c, &n[12], 8);
    const float lo0[3] = {n[0], n[2], n[8]}, hi0[3] = {n[1], n[3], n[9]};
    const float lo1[3] = {n[4], n[6], n[10]}, hi1[3] = {n[5], n[7], n[11]};
    uint32_t b0, e0, b1, e1;
    const VBox v0 = walk2(c[0], d + 1, b0, e0);
    if (tris.size() == 1 && c[0] == c[1]) {  // the one-triangle root: both children are the same leaf
      begin = b0; end = e0;
      contains(lo0, hi0, v0, "BVH2 child box 0", link);
      contains(lo1, hi1, v0, "BVH2 child box 1", link);
      return v0;
    }
    const VBox v1 = walk2(c[1], d + 1, b1, e1);
    contains(lo0, hi0, v0, "BVH2 child box 0", link);
    contains(lo1, hi1, v1, "BVH2 child box 1", link);
    if (e0 != b1) fail("children's ranges are not adjacent", e0, b1);
    begin = b0;
    end = e1;
    const uint32_t cnt = end - begin;
    uint32_t need = 0;
    while (((uint64_t)leaf << need) < cnt) need++;
    if (!(d + need + 1 < budget)) {  // bvh.cpp: no SAH split here
      ++balanced;
      if (e0 - b0 != cnt / 2) fail("budget-forced split is not balanced", e0 - b0, cnt);
      float clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (uint32_t k = begin; k < end; ++k)
        for (int a = 0; a < 3; ++a) { clo[a] = std::min(clo[a], centroid(k, a)); chi[a] = std::max(chi[a], centroid(k, a)); }
      int axis = 0;
      if (chi[1] - clo[1] > chi[axis] - clo[axis]) axis = 1;
      if (chi[2] - clo[2] > chi[axis] - clo[axis]) axis = 2;
      float lmax = -INFINITY, rmin = INFINITY;
      for (uint32_t k = b0; k < e0; ++k) lmax = std::max(lmax, centroid(k, axis));
      for (uint32_t k = b1; k < e1; ++k) rmin = std::min(rmin, centroid(k, axis));
      if (!(lmax <= rmin)) fail("balanced split does not order the centroids", link, axis);
    } else {
      ++sah;
    }
    VBox v = v0;
    v.grow(v1);
    return v;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: bvh_build_check tris.bin leaf fan depth\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leaf = atoi(argv[2]), fan = atoi(argv[3]);
  const uint32_t budget = (uint32_t)atoi(argv[4]);
  if (raw.size() < 9 || leaf < 1 || leaf > 16 || fan < 2 || fan > 4 || budget < 1) { fprintf(stderr, "bad arguments\n"); return 2; }
  std::vector<BuildTri> tris(raw.size() / 9);
  for (size_t i = 0; i < tris.size(); ++i) {
    BuildTri& t = tris[i];
    std::memcpy(t.v0, &raw[9 * i], 12);
    std::memcpy(t.v1, &raw[9 * i + 3], 12);
    std::memcpy(t.v2, &raw[9 * i + 6], 12);
    t.mesh = 0; t.prim = (uint32_t)i; t.gid = (uint32_t)i; t.flags = 0;
  }
  BvhOut bvh;
  build_bvh(tris, leaf, budget, bvh);
  std::vector<float> n4;
  uint32_t num4 = 0, need = 0, dep4 = 0;
  collapse_bvh4(bvh.nodes, n4, num4, need, dep4, fan);

  if (argc > 5) {  // the 4-wide nodes and the triangle records, as ptgs_scene_get_bvh exposes them
    FILE* out = fopen(argv[5], "wb");
    if (!out) { perror(argv[5]); return 2; }
    fwrite(&num4, 4, 1, out);
    fwrite(n4.data(), sizeof(float), n4.size(), out);
    fwrite(bvh.tris.data(), sizeof(float), bvh.tris.size(), out);
    fclose(out);
  }

  Check ck(tris, bvh, leaf, budget);
  const size_t nt = tris.size();
  // triangle records: ids a permutation of the input
  ck.gid.assign(nt, 0);
  ck.cover.assign(nt, 0);
  if (bvh.tris.size() != 12 * nt || bvh.nodes.size() != 16 * (size_t)bvh.num_nodes) ck.fail("array sizes", bvh.tris.size(), bvh.nodes.size());
  {
    std::vector<uint32_t> seen(nt, 0);
    for (size_t k = 0; k < nt && 12 * k + 11 < bvh.tris.size(); ++k) {
      uint32_t g;
      std::memcpy(&g, &bvh.tris[12 * k + 11], 4);
      if (g >= nt) { ck.fail("record id out of range", (long long)k, g); g = 0; }
      ck.gid[k] = g;
      ++seen[g];
    }
    for (size_t g = 0; g < nt; ++g)
      if (seen[g] != 1) ck.fail("triangle not in exactly one record", (long long)g, seen[g]);
  }
  // BVH2
  {
    uint32_t b = 0, e = 0;
    ck.walk2(0, 0, b, e);
    if (b != 0 || e != nt) ck.fail("the root does not span the array", b, e);
    for (size_t k = 0; k < nt; ++k)
      if (ck.cover[k] != 1) ck.fail("BVH2: record not in exactly one leaf", (long long)k, ck.cover[k]);
    if (ck.depth2 != bvh.depth) ck.fail("reported BVH2 depth", ck.depth2, bvh.depth);
    if (ck.depth2 > budget) ck.fail("BVH2 depth exceeds the budget", ck.depth2, budget);
    if (ck.max_leaf != bvh.max_leaf) ck.fail("reported largest leaf", ck.max_leaf, bvh.max_leaf);
  }
  // 4-wide nodes, children after parents: a reverse pass gives vertex bounds, stack need and depth
  unsigned long long empty = 0, leaves4 = 0;
  uint32_t need4 = 0, depth4 = 0;
  if (n4.size() != 32 * (size_t)num4 || num4 == 0) {
    ck.fail("4-wide array size", (long long)n4.size(), num4);
  } else {
    std::vector<VBox> vb(num4);
    std::vector<uint32_t> nd(num4, 0), dp(num4, 0), linked(num4, 0);
    std::fill(ck.cover.begin(), ck.cover.end(), 0u);
    for (size_t i = num4; i-- > 0;) {
      const float* f = &n4[32 * i];
      uint32_t occupied = 0, m = 0, d = 0;
      bool gap = false;
      for (int j = 0; j < 4; ++j) {
        int32_t link;
        std::memcpy(&link, &f[24 + j], 4);
        bool far = true;
        for (int a = 0; a < 6; ++a) far = far && f[a * 4 + j] == 1e30f;
        if (far) {
          ++empty;
          gap = true;
          if (link != 0) ck.fail("empty slot with a link", (long long)i, j);
          continue;
        }
        ++occupied;
        if (gap) ck.fail("occupied slot after an empty one", (long long)i, j);
        const float lo[3] = {f[0 + j], f[8 + j], f[16 + j]}, hi[3] = {f[4 + j], f[12 + j], f[20 + j]};
        VBox v;
        if (link < 0) {
          uint32_t first = 0, count = 0;
          if (!ck.leaf_range(link, first, count)) continue;
          ++leaves4;
          for (uint32_t k = first; k < first + count; ++k) ++ck.cover[k];
          v = ck.leaf_box(first, count);
        } else if ((size_t)link <= i || (uint32_t)link >= num4) {
          ck.fail("4-wide link not to a later node", (long long)i, link);
          continue;
        } else {
          ++linked[link];
          v = vb[link];
          m = std::max(m, nd[link]);
          d = std::max(d, dp[link]);
        }
        ck.contains(lo, hi, v, "4-wide child box", (long long)i);
        vb[i].grow(v);
      }
      if (occupied < 2 || occupied > (uint32_t)fan) ck.fail("occupied slots", (long long)i, occupied);
      nd[i] = (occupied ? occupied - 1 : 0) + m;
      dp[i] = 1 + d;
      for (int k = 28; k < 32; ++k)
        if (f[k] != 0.0f) ck.fail("unused words not zero", (long long)i, k);
    }
    for (uint32_t i = 1; i < num4; ++i)
      if (linked[i] != 1) ck.fail("4-wide node not linked exactly once", i, linked[i]);
    if (!(tris.size() == 1))
      for (size_t k = 0; k < nt; ++k)
        if (ck.cover[k] != 1) ck.fail("4-wide: record not in exactly one leaf", (long long)k, ck.cover[k]);
    need4 = nd[0];
    depth4 = dp[0];
    if (need4 != need) ck.fail("reported stack need", need4, need);
    if (depth4 != dep4) ck.fail("reported 4-wide depth", depth4, dep4);
  }
  printf("bvh_build_check tris %zu nodes2 %u depth2 %u leaves %llu maxleaf %u balanced %llu sah %llu nodes4 %u depth4 %u "
         "stack %u leaves4 %llu empty %llu violations %llu\n",
         nt, bvh.num_nodes, ck.depth2, ck.leaves, ck.max_leaf, ck.balanced, ck.sah, num4, depth4, need4, leaves4, empty,
         ck.viol);
  return ck.viol ? 1 : 0;
}
