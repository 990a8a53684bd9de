// tree_opt_check — stand-alone host check of the reinsertion-optimised traversal tree (bvh_opt.h) and the host
// evidence for it: the lockstep node steps of both megakernel walks on the canonical and on the optimised nodes.
//
//   tree_opt_check <tris.bin> <leaf> <fan> <depth> <waves> [limit]
//
// tris.bin holds float32 triangles (9 floats each; an empty file: the empty tree). The program builds the
// canonical host tree as the scene upload does (build_bvh, collapse_bvh4) and calls what the upload calls
// (make_opt_traversal_nodes). limit: the stack limit handed to the optimiser; 0 (default) is the upload's rule
// (PTGS_STACK when the canonical need is below it, else PTGS_STACK + PTGS_STACK_OVF); -1 is the canonical need
// + 1 (the canonical tree sits at the limit).
// Structure, violations when one fails:
//   - the optimised nodes' leaf links are the canonical ones, each as often; interior links are in range and
//     every node but the root is linked exactly once; slots 0 and 1 are never empty;
//   - every interior child box contains the boxes of the leaves below it;
//   - the reported need and depth are what a fresh pass over the output computes, and the need is below the limit;
//   - a second run gives identical bytes (nodes, compact nodes, report);
//   - with the limit at 1 (below any need) the optimiser reports "not applied" and the compact nodes are the plain
//     conversion's, byte for byte.
// Walks: the 64-lane lockstep models of tests/native/closest_walk_check.cpp (the shipped two-site walk with the
// packed stack word and the cull at pop) and tests/native/anyhit_walk_check.cpp (the shipped single-exit walk),
// run on the same seeded waves over the canonical and the optimised compact nodes. Violations: a closest-hit
// (t, gid) or an occlusion that differs from a brute-force test of every triangle, on either tree; a stack write
// at or above the walked tree's stack need or PTGS_STACK + PTGS_STACK_OVF. Every fifth triangle is non-opaque
// for the any-hit walk (accepted by a fixed hash of (gid, seed)).
// Prints one line of "name value" pairs (c_: closest-hit, a_: any-hit; _can: canonical, _opt: optimised; wave
// and lane node steps, triangle steps); exit status 1 when violations > 0.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"
#include "bvh_opt.h"
#include "stack_key.h"

using namespace ptgs;

static uint32_t g_rng = 24680u;
static uint32_t urand32() {
  g_rng = g_rng * 747796405u + 2891336453u;
  uint32_t w = ((g_rng >> ((g_rng >> 28u) + 4u)) ^ g_rng) * 277803737u;
  return (w >> 22u) ^ w;
}
static float urand() { return (float)(urand32() >> 8) * (1.0f / 16777216.0f); }  // [0, 1)
static float safe_inv(float d) {  // pt_device.h
  const float eps = 1e-20f;
  float a = std::fabs(d) < eps ? (d < 0.0f ? -eps : eps) : d;
  return 1.0f / a;
}
static float qbyte(uint32_t w, int j) { return (float)((w >> (8 * j)) & 0xffu); }

static unsigned long long g_viol = 0;
static void violation(const char* what) {
  if (g_viol < 8) fprintf(stderr, "tree_opt_check: %s\n", what);
  ++g_viol;
}

static const uint32_t kStack = 39u, kStackTotal = 39u + 9u;  // pt_device.h PTGS_STACK, + PTGS_STACK_OVF
static const uint32_t ANY_DONE = 0x7fffffffu;

struct Tree {
  std::vector<float> n4;
  std::vector<uint32_t> n64;  // packed links
  uint32_t num = 0, need = 0, depth = 0;
  StackLayout lay{};
  uint32_t done = 0x7fffffffu;  // the culling walk's DONE: the key's bits clear
};
struct Mesh {
  std::vector<float> tris;  // 12 floats per triangle
  std::vector<uint32_t> flags;
};
struct RayH {
  float o[3], d[3], inv[3], oinv[3], tmin, tmax;
  uint32_t seed;
};
struct HitH {
  float t;
  uint32_t gid;
};

static uint32_t tri_gid(const float* T) { uint32_t g; std::memcpy(&g, T + 11, 4); return g; }
static bool tri_isect(const RayH& r, const float* T, float& t) {  // pt_device.h tri_isect
  const float* v0 = T; const float* e1 = T + 4; const float* e2 = T + 8;
  const float p[3] = {r.d[1] * e2[2] - r.d[2] * e2[1], r.d[2] * e2[0] - r.d[0] * e2[2], r.d[0] * e2[1] - r.d[1] * e2[0]};
  const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
  if (det == 0.0f) return false;
  const float inv_det = 1.0f / det;
  const float tv[3] = {r.o[0] - v0[0], r.o[1] - v0[1], r.o[2] - v0[2]};
  const float u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) * inv_det;
  if (u < 0.0f || u > 1.0f) return false;
  const float q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const float v = (r.d[0] * q[0] + r.d[1] * q[1] + r.d[2] * q[2]) * inv_det;
  if (v < 0.0f || u + v > 1.0f) return false;
  t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv_det;
  return true;
}
static void tri_closest(const RayH& r, const float* T, HitH& h) {  // leaf_closest's tests (opaque triangles)
  float t;
  if (!tri_isect(r, T, t)) return;
  if (!(t >= r.tmin && t <= h.t)) return;
  if (t == h.t && tri_gid(T) >= h.gid) return;
  h.t = t;
  h.gid = tri_gid(T);
}
static bool accept(uint32_t gid, uint32_t seed) {  // any pure function of (triangle, seed)
  uint32_t s = seed ^ (gid * 0x9E3779B9u);
  s = s * 747796405u + 2891336453u;
  return (((s >> 15) ^ s) & 3u) != 0u;
}
static bool tri_occludes(const Mesh& m, const RayH& r, uint32_t slot) {
  const float* T = &m.tris[12 * (size_t)slot];
  float t;
  if (!tri_isect(r, T, t) || !(t >= r.tmin && t <= r.tmax)) return false;
  if (m.flags[slot] & 1u) return accept(tri_gid(T), r.seed);
  return true;
}

// box4_q: tcap is the closest-hit walk's shrinking cap, or the any-hit walk's constant tmax
static void box4(const Tree& tr, const RayH& r, uint32_t node, float tcap, bool hit[4], float tn[4], uint32_t c[4]) {
  const uint32_t* o = &tr.n64[PTGS_NODE64_DWORDS * (size_t)node];
  float org[3], step[3];
  std::memcpy(org, o, 12);
  std::memcpy(step, o + 3, 12);
  for (int j = 0; j < 4; ++j) {
    float q0[3], q1[3];
    for (int a = 0; a < 3; ++a) {
      const bool neg = r.inv[a] < 0.0f;
      const float s = step[a] * r.inv[a], cc = std::fmaf(org[a], r.inv[a], -r.oinv[a]);
      q0[a] = std::fmaf(qbyte(o[6 + 2 * a + (neg ? 1 : 0)], j), s, cc);
      q1[a] = std::fmaf(qbyte(o[6 + 2 * a + (neg ? 0 : 1)], j), s, cc);
    }
    const float n = std::fmax(std::fmax(q0[0], q0[1]), std::fmax(q0[2], r.tmin));
    const float f = std::fmin(std::fmin(std::fmin(q1[0], q1[1]), q1[2]), tcap);
    hit[j] = (n <= f * 1.0000004f) && (j < 2 || o[12 + j] != 0u);
    tn[j] = hit[j] ? n : INFINITY;
    c[j] = o[12 + j];
  }
}

struct Lane {
  RayH r;
  bool active = false;  // part of the wave's launch
  bool in = false;      // still in the walk (not returned)
  HitH h{0.0f, 0u};
  bool result = false;
  uint32_t node = 0, leaf = 0, sp = 0, hw = 0;
  std::vector<uint32_t> stack;
};
struct Stats {
  unsigned long long node_steps = 0, lane_nodes = 0, tri_steps = 0, lane_tris = 0, culled = 0, hw = 0;
};

static void push(const Tree& tr, Lane& l, uint32_t word) {
  if (l.sp >= tr.need || l.sp >= kStackTotal) { violation("stack write at or above the need"); return; }
  l.stack[l.sp++] = word;
  if (l.sp > l.hw) l.hw = l.sp;
}
static void leaf_span(const Tree& tr, uint32_t link, uint32_t& start, uint32_t& count) {  // leaf_range<true>
  start = link & tr.lay.leaf_start_mask;
  count = ((link & 0x7fffffffu) >> tr.lay.leaf_shift) + 1u;
}

// ---- closest hit: the two-site walk (closest_walk_check.cpp, variant "old") ----
static uint32_t pop_closest(const Tree& tr, Lane& l, Stats& st) {
  const float cap = l.h.t * 1.0000004f;
  const uint32_t km = tr.lay.key_mask;
  uint32_t x;
  for (;;) {
    x = l.sp ? l.stack[--l.sp] : tr.done;
    if (!(stack_bound(x, km) > cap)) break;
    ++st.culled;
  }
  return stack_link(x, km);
}
static uint32_t leaf_closest(const Tree& tr, const Mesh& m, Lane& l, uint32_t link, Stats& st) {
  uint32_t start, count;
  leaf_span(tr, link, start, count);
  for (uint32_t k = 0; k < count; ++k) tri_closest(l.r, &m.tris[12 * (size_t)(start + k)], l.h);
  st.lane_tris += count;
  return count;
}
static void walk_closest(const Tree& tr, const Mesh& m, Lane* L, Stats& st) {
  const uint32_t DONE = tr.done;
  auto interior = [&](uint32_t node) { return (int32_t)node >= 0 && node != DONE; };
  for (;;) {
    bool any_in = false;
    for (int i = 0; i < 64; ++i) any_in |= L[i].in;
    if (!any_in) return;
    bool N[64];
    for (int i = 0; i < 64; ++i) N[i] = L[i].in && interior(L[i].node);
    for (;;) {
      bool any = false;
      for (int i = 0; i < 64; ++i) any |= N[i];
      if (!any) break;
      ++st.node_steps;
      for (int i = 0; i < 64; ++i) {
        if (!N[i]) continue;
        Lane& l = L[i];
        ++st.lane_nodes;
        bool hit[4];
        float tn[4];
        uint32_t c[4];
        box4(tr, l.r, l.node, l.h.t, hit, tn, c);
        const bool need = !(hit[0] || hit[1] || hit[2] || hit[3]);
        if (!need) {  // enter_box4 with a hit child: sorted, farthest pushed first
          auto cswap = [&](int a, int b) {
            if (tn[b] < tn[a]) { std::swap(tn[a], tn[b]); std::swap(c[a], c[b]); }
          };
          cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
          for (int j = 3; j >= 1; --j)
            if (tn[j] != INFINITY) push(tr, l, stack_pack(c[j], tn[j], tr.lay.key_mask));
          l.node = c[0];
        }
        if (need) l.node = pop_closest(tr, l, st);
        if ((int32_t)l.node < 0 && l.leaf == DONE) {
          l.leaf = l.node;
          l.node = pop_closest(tr, l, st);
        }
      }
      bool all = true;  // every lane of this iteration holds a leaf or is done
      for (int i = 0; i < 64; ++i)
        if (N[i] && !(L[i].leaf != DONE || L[i].node == DONE)) all = false;
      if (all) break;
      for (int i = 0; i < 64; ++i) N[i] = N[i] && interior(L[i].node);
    }
    uint32_t iters = 0;
    for (int i = 0; i < 64; ++i) {
      Lane& l = L[i];
      if (!l.in) continue;
      uint32_t k = 0;
      if (l.leaf != DONE) {
        k += leaf_closest(tr, m, l, l.leaf, st);
        l.leaf = DONE;
      }
      if ((int32_t)l.node < 0) {
        k += leaf_closest(tr, m, l, l.node, st);
        l.node = pop_closest(tr, l, st);
      }
      iters = std::max(iters, k);
      if (l.node == DONE) l.in = false;
    }
    st.tri_steps += iters;
  }
}

// ---- any hit: the single-exit walk (anyhit_walk_check.cpp, "se") ----
static void walk_any(const Tree& tr, const Mesh& m, Lane* L, Stats& st) {
  const uint32_t DONE = ANY_DONE;
  bool occluded[64] = {};
  for (;;) {
    bool any_in = false;
    for (int i = 0; i < 64; ++i) any_in |= L[i].in;
    if (!any_in) return;
    bool N[64];
    for (int i = 0; i < 64; ++i) N[i] = L[i].in && (int32_t)L[i].node >= 0 && L[i].node != DONE;
    for (;;) {
      bool any = false;
      for (int i = 0; i < 64; ++i) any |= N[i];
      if (!any) break;
      ++st.node_steps;
      for (int i = 0; i < 64; ++i) {
        if (!N[i]) continue;
        Lane& l = L[i];
        ++st.lane_nodes;
        bool hit[4];
        float tn[4];
        uint32_t c[4];
        box4(tr, l.r, l.node, l.r.tmax, hit, tn, c);
        int first = -1;  // the first hit child in slot order is entered, the others pushed in slot order
        for (int j = 0; j < 4; ++j)
          if (hit[j]) {
            if (first < 0) first = j;
            else push(tr, l, c[j]);
          }
        l.node = first >= 0 ? c[first] : (l.sp ? l.stack[--l.sp] : DONE);
      }
      for (int i = 0; i < 64; ++i) N[i] = N[i] && (int32_t)L[i].node >= 0 && L[i].node != DONE;
    }
    unsigned long long iters = 0;
    for (int i = 0; i < 64; ++i) {
      Lane& l = L[i];
      if (!l.in) continue;
      if ((int32_t)l.node < 0) {
        uint32_t start, count;
        leaf_span(tr, l.node, start, count);
        unsigned long long k = 0;
        bool occ = false;
        for (; k < count && !occ; ++k) {
          ++st.lane_tris;
          occ = tri_occludes(m, l.r, start + (uint32_t)k);
        }
        iters = std::max(iters, k);
        occluded[i] = occ;
        l.node = l.sp ? l.stack[--l.sp] : DONE;
        if (occ) l.node = DONE;
      }
      if (l.node == DONE) { l.in = false; l.result = occluded[i]; }
    }
    st.tri_steps += iters;
  }
}

static void reset(const Tree& tr, Lane* L, bool closest) {
  for (int i = 0; i < 64; ++i) {
    Lane& l = L[i];
    l.in = l.active && tr.num > 0;
    l.h = HitH{l.r.tmax, 0xffffffffu};
    l.result = false;
    l.node = 0; l.leaf = closest ? tr.done : ANY_DONE; l.sp = 0; l.hw = 0;
    l.stack.assign(tr.need ? tr.need : 1, 0u);
  }
}

// need and depth of 4-wide nodes whose children come after their parents; the structure checks on the way
static void fresh_need_depth(const std::vector<float>& n4, uint32_t num, uint32_t& need_out, uint32_t& depth_out) {
  std::vector<uint32_t> need(num, 0), dep(num, 1), linked(num, 0);
  std::vector<float> sub((size_t)num * 6);  // the union of the leaf boxes below each node
  for (size_t i = num; i-- > 0;) {
    const float* f = &n4[32 * i];
    uint32_t cnt = 0, m = 0, d = 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int j = 0; j < 4; ++j) {
      int32_t link;
      std::memcpy(&link, &f[24 + j], 4);
      if (link == 0) {
        if (j < 2) violation("an empty slot 0 or 1");
        continue;
      }
      ++cnt;
      float clo[3], chi[3];
      for (int a = 0; a < 3; ++a) { clo[a] = f[(2 * a) * 4 + j]; chi[a] = f[(2 * a + 1) * 4 + j]; }
      if (link > 0) {
        if ((uint32_t)link >= num || (size_t)link <= i) { violation("an interior link out of range"); continue; }
        ++linked[link];
        m = std::max(m, need[link]);
        d = std::max(d, dep[link]);
        for (int a = 0; a < 3; ++a)
          if (!(clo[a] <= sub[6 * (size_t)link + a] && chi[a] >= sub[6 * (size_t)link + 3 + a]))
            violation("a child box does not contain its subtree's leaf boxes");
      }
      for (int a = 0; a < 3; ++a) {
        lo[a] = std::fmin(lo[a], link > 0 ? sub[6 * (size_t)link + a] : clo[a]);
        hi[a] = std::fmax(hi[a], link > 0 ? sub[6 * (size_t)link + 3 + a] : chi[a]);
      }
    }
    for (int a = 0; a < 3; ++a) { sub[6 * i + a] = lo[a]; sub[6 * i + 3 + a] = hi[a]; }
    if (cnt < 2) violation("a node with fewer than two children");
    need[i] = (cnt ? cnt - 1 : 0) + m;
    dep[i] = 1 + d;
  }
  for (uint32_t i = 1; i < num; ++i)
    if (linked[i] != 1) violation("a node that is not linked exactly once");
  need_out = num ? need[0] : 0;
  depth_out = num ? dep[0] : 0;
}
// (the nodes' links are int bits in float words, NaNs among them: bytes, not values)
static bool same_bytes(const std::vector<float>& a, const std::vector<float>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0);
}
static std::vector<int32_t> leaf_links(const std::vector<float>& n4, uint32_t num) {
  std::vector<int32_t> v;
  for (uint32_t i = 0; i < num; ++i)
    for (int j = 0; j < 4; ++j) {
      int32_t link;
      std::memcpy(&link, &n4[32 * (size_t)i + 24 + j], 4);
      if (link < 0) v.push_back(link);
    }
  std::sort(v.begin(), v.end());
  return v;
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: tree_opt_check tris.bin leaf fan depth waves [limit]\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leafsz = atoi(argv[2]), fan = atoi(argv[3]), waves = atoi(argv[5]);
  const uint32_t depth = (uint32_t)atoi(argv[4]);
  const int limit_arg = argc > 6 ? atoi(argv[6]) : 0;

  Tree can, opt;
  Mesh mesh;
  float blo[3] = {-1.0f, -1.0f, -1.0f}, bhi[3] = {1.0f, 1.0f, 1.0f};
  std::vector<BuildTri> tris(raw.size() / 9);
  if (!tris.empty())
    for (int a = 0; a < 3; ++a) { blo[a] = 1e30f; bhi[a] = -1e30f; }
  for (size_t i = 0; i < tris.size(); ++i) {
    BuildTri& t = tris[i];
    std::memcpy(t.v0, &raw[9 * i], 12);
    std::memcpy(t.v1, &raw[9 * i + 3], 12);
    std::memcpy(t.v2, &raw[9 * i + 6], 12);
    t.mesh = 0; t.prim = (uint32_t)i; t.gid = (uint32_t)i; t.flags = (i % 5u == 0u) ? 1u : 0u;
    for (int k = 0; k < 9; ++k) {
      blo[k % 3] = std::fmin(blo[k % 3], raw[9 * i + k]);
      bhi[k % 3] = std::fmax(bhi[k % 3], raw[9 * i + k]);
    }
  }
  {
    // (the empty tree too: build_bvh gives it the root no ray reaches, as the upload does)
    BvhOut bvh;
    build_bvh(tris, leafsz, depth, bvh);
    if (bvh.nodes.empty() && tris.size() == 1) {
      // build_bvh returns a lone triangle as a leaf with no node to hold it: the root its single-triangle branch
      // writes for a deeper range (both children the same leaf) stands in for it here
      bvh.nodes.assign(16, 0.0f);
      float* f = bvh.nodes.data();
      for (int c = 0; c < 2; ++c) {
        f[4 * c + 0] = blo[0]; f[4 * c + 1] = bhi[0]; f[4 * c + 2] = blo[1]; f[4 * c + 3] = bhi[1];
        f[8 + 2 * c] = blo[2]; f[9 + 2 * c] = bhi[2];
      }
      const int32_t leaf = ~(int32_t)0;  // one triangle at record 0
      std::memcpy(&f[12], &leaf, 4);
      std::memcpy(&f[13], &leaf, 4);
    }
    collapse_bvh4(bvh.nodes, can.n4, can.num, can.need, can.depth, fan);
    mesh.tris.swap(bvh.tris);
    mesh.flags.swap(bvh.tri_flags);
  }
  const uint32_t limit = limit_arg > 0 ? (uint32_t)limit_arg : limit_arg < 0 ? can.need + 1u : can.need < kStack ? kStack : kStackTotal;
  if (!make_traversal_nodes(can.n4.data(), can.num, -1, can.n64, can.lay)) {
    printf("tree_opt_check: conversion refused\n");
    return 1;
  }
  can.done = 0x7fffffffu & ~can.lay.key_mask;

  TreeOptInfo info, info2, info_off;
  if (!make_opt_traversal_nodes(can.n4.data(), can.num, fan, limit, true, -1, opt.n64, opt.lay, info, &opt.n4)) {
    printf("tree_opt_check: conversion refused\n");
    return 1;
  }
  opt.num = (uint32_t)(opt.n4.size() / 32);
  opt.done = 0x7fffffffu & ~opt.lay.key_mask;
  fresh_need_depth(opt.n4, opt.num, opt.need, opt.depth);
  if (info.applied) {
    if (info.num_nodes != opt.num || info.need != opt.need || info.depth != opt.depth) violation("the reported count, need or depth");
    if (!(opt.need < limit)) violation("the optimised need reaches the limit");
    if (leaf_links(opt.n4, opt.num) != leaf_links(can.n4, can.num)) violation("the leaf links differ from the canonical ones");
  } else {
    if (!same_bytes(opt.n4, can.n4) || opt.n64 != can.n64) violation("not applied, but the nodes are not the canonical ones");
  }
  {  // a second run: identical bytes
    Tree again;
    if (!make_opt_traversal_nodes(can.n4.data(), can.num, fan, limit, true, -1, again.n64, again.lay, info2, &again.n4) ||
        !same_bytes(again.n4, opt.n4) || again.n64 != opt.n64 ||
        info2.applied != info.applied || info2.num_nodes != info.num_nodes || info2.need != info.need ||
        info2.depth != info.depth || info2.area_after != info.area_after || info2.area_before != info.area_before)
      violation("two runs differ");
  }
  {  // a limit below any need: not applied, the plain conversion's bytes
    Tree off;
    if (!make_opt_traversal_nodes(can.n4.data(), can.num, fan, 1u, true, -1, off.n64, off.lay, info_off, &off.n4) ||
        info_off.applied || off.n64 != can.n64 || !same_bytes(off.n4, can.n4) || off.lay.key_mask != can.lay.key_mask ||
        off.lay.leaf_shift != can.lay.leaf_shift)
      violation("limit 1: applied, or not the plain conversion");
  }
  for (const Tree* tr : {&can, &opt}) {
    if (tr->num > tr->done) violation("an interior index reaches DONE");
  }

  const float ext[3] = {bhi[0] - blo[0], bhi[1] - blo[1], bhi[2] - blo[2]};
  const float diag = std::sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
  Stats sc[2], sa[2];
  unsigned long long nrays = 0, nhit = 0, nocc = 0, k = 0;
  std::vector<Lane> lanes(64);
  Lane* L = lanes.data();
  const Tree* T[2] = {&can, &opt};
  for (int w = 0; w < waves; ++w) {
    const uint32_t nact = 1u + urand32() % 64u;
    for (int i = 0; i < 64; ++i) L[i].active = false;
    for (uint32_t a = 0; a < nact;) {
      const uint32_t i = urand32() % 64u;
      if (!L[i].active) { L[i].active = true; ++a; }
    }
    // the rays of closest_walk_check / anyhit_walk_check; the any-hit walk takes the same ray with a shadow ray's
    // tmax (mode 0: a segment between two points of the bounds)
    float any_tmax[64];
    for (int i = 0; i < 64; ++i) {
      if (!L[i].active) continue;
      RayH& r = L[i].r;
      const int mode = (int)(k % 4);  // 0: segment; 1: general; 2: one axis-parallel component; 3: origin outside
      float len = 0.0f;
      for (int a = 0; a < 3; ++a) {
        const float u = mode == 3 ? (urand() * 3.0f - 1.0f) : urand();
        r.o[a] = blo[a] + u * ext[a];
        float d = mode == 0 ? (blo[a] + urand() * ext[a]) - r.o[a] : urand() * 2.0f - 1.0f;
        if (mode == 2 && a == (int)(k / 4 % 3)) d = (k & 16) ? 0.0f : -0.0f;
        r.d[a] = d;
        len += d * d;
      }
      len = std::sqrt(len);
      if (!(len > 0.0f)) { r.d[0] = 1.0f; len = 1.0f; }
      for (int a = 0; a < 3; ++a) {
        r.d[a] /= len;
        r.inv[a] = safe_inv(r.d[a]);
        r.oinv[a] = r.o[a] * r.inv[a];
      }
      r.tmin = 0.001f;
      const float lo = std::log(1e-3f * diag), hi = std::log(1e4f);
      any_tmax[i] = mode == 0 ? std::fmax(len - 0.005f, 0.002f) : std::exp(lo + urand() * (hi - lo));
      r.seed = urand32();
      ++k;
      ++nrays;
    }
    // closest hit, tmax 1e4
    HitH ref[64];
    for (int i = 0; i < 64; ++i) {
      if (!L[i].active) continue;
      L[i].r.tmax = 10000.0f;
      ref[i] = HitH{L[i].r.tmax, 0xffffffffu};
      for (size_t s = 0; s < mesh.flags.size() && !tris.empty(); ++s) tri_closest(L[i].r, &mesh.tris[12 * s], ref[i]);
      nhit += ref[i].gid != 0xffffffffu;
    }
    for (int v = 0; v < 2; ++v) {
      reset(*T[v], L, true);
      walk_closest(*T[v], mesh, L, sc[v]);
      for (int i = 0; i < 64; ++i) {
        if (!L[i].active) continue;
        if (std::memcmp(&L[i].h.t, &ref[i].t, 4) != 0 || L[i].h.gid != ref[i].gid) violation("a closest hit differs from brute force");
        if (L[i].sp != 0) violation("the closest-hit walk ends on a stack that is not empty");
        sc[v].hw = std::max<unsigned long long>(sc[v].hw, L[i].hw);
      }
    }
    // any hit
    bool occ[64];
    for (int i = 0; i < 64; ++i) {
      if (!L[i].active) continue;
      L[i].r.tmax = any_tmax[i];
      occ[i] = false;
      for (size_t s = 0; s < mesh.flags.size() && !tris.empty() && !occ[i]; ++s) occ[i] = tri_occludes(mesh, L[i].r, (uint32_t)s);
      nocc += occ[i];
    }
    for (int v = 0; v < 2; ++v) {
      reset(*T[v], L, false);
      walk_any(*T[v], mesh, L, sa[v]);
      for (int i = 0; i < 64; ++i) {
        if (!L[i].active) continue;
        if (L[i].result != occ[i]) violation("an occlusion differs from brute force");
        sa[v].hw = std::max<unsigned long long>(sa[v].hw, L[i].hw);
      }
    }
  }
  printf("tree_opt_check applied %u limit %u nodes_can %u nodes_opt %u need_can %u need_opt %u depth_can %u depth_opt %u "
         "fan_opt %u area_can %.6f area_opt %.6f ms %.3f waves %d rays %llu hits %llu occluded %llu "
         "c_node_steps_can %llu c_node_steps_opt %llu c_lane_nodes_can %llu c_lane_nodes_opt %llu "
         "c_tri_steps_can %llu c_tri_steps_opt %llu c_lane_tris_can %llu c_lane_tris_opt %llu "
         "c_high_water_can %llu c_high_water_opt %llu "
         "a_node_steps_can %llu a_node_steps_opt %llu a_lane_nodes_can %llu a_lane_nodes_opt %llu "
         "a_tri_steps_can %llu a_tri_steps_opt %llu a_lane_tris_can %llu a_lane_tris_opt %llu "
         "a_high_water_can %llu a_high_water_opt %llu violations %llu\n",
         info.applied, limit, can.num, opt.num, can.need, opt.need, can.depth, opt.depth, info.fan, info.area_before,
         info.applied ? info.area_after : info.area_before, info.ms, waves, nrays, nhit, nocc,
         sc[0].node_steps, sc[1].node_steps, sc[0].lane_nodes, sc[1].lane_nodes, sc[0].tri_steps, sc[1].tri_steps,
         sc[0].lane_tris, sc[1].lane_tris, sc[0].hw, sc[1].hw,
         sa[0].node_steps, sa[1].node_steps, sa[0].lane_nodes, sa[1].lane_nodes, sa[0].tri_steps, sa[1].tri_steps,
         sa[0].lane_tris, sa[1].lane_tris, sa[0].hw, sa[1].hw, g_viol);
  return g_viol ? 1 : 0;
}
