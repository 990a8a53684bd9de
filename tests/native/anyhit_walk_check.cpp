// anyhit_walk_check — stand-alone host check of the path tracer's any-hit (shadow) walk
// (pt_device.h trace_any / leaf_any; the postponed leaf: tools/patches/pt_any_park_rejected.patch).
//
//   anyhit_walk_check <tris.bin> <leaf> <fan> <depth> <waves>
//
// tris.bin holds float32 triangles (9 floats each; an empty file: the empty tree). The program builds the
// host tree as the scene upload does (build_bvh, collapse_bvh4, make_traversal_nodes)
// and restates the walk as a 64-lane lockstep model: the lanes of a wave that are in a loop run its body
// together and the loop ends when the last of them leaves, as the hardware's exec mask does it. The float
// expressions are the kernel's (box4_q, tri_isect and leaf_any's folded form; -ffp-contract=off, explicit
// fmaf). Three walks are modelled:
//   old   the walk with two returns, a continue and the per-lane `have` chain (the kernel's before the single
//         exit: DESIGN.md §5, round 9);
//   se    single exit, the entered child and the pushes derived from the four children's wave hit masks (the
//         walk that ships);
//   park  se with the postponed leaf (the patch).
// Every fifth triangle is flagged non-opaque; a flagged triangle is accepted by a fixed hash of (gid, seed).
// Rays, all seeded, four kinds in turn: a segment between two points of the scene bounds (tmax = its length
// - 0.005, as shadow_towards); a general direction; one axis-parallel component (+0 / -0); an origin outside
// the bounds; the last three with tmax log-uniform in [1e-3 x the diagonal, 1e4]. Each wave has a random
// subset of 1 to 64 active lanes, so the break ballot of the parked walk sees inactive lanes.
// Violations: the old walk differs from a brute-force test of every triangle; a new walk differs from the old
// one; a stack write at or above the tree's stack need (collapse_bvh4's max_stack) or above the kernel's
// PTGS_STACK + PTGS_STACK_OVF; a push by a lane that is not in the node loop (inactive, or done).
// Prints one line of "name value" pairs; exit status 1 when violations > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"
#include "stack_key.h"

using namespace ptgs;

static uint32_t g_rng = 13579u;
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

struct Tree {
  std::vector<float> n4;
  std::vector<uint32_t> n64;  // packed links
  std::vector<float> tris;    // 12 floats per triangle
  std::vector<uint32_t> flags;
  uint32_t num = 0, need = 0;
  StackLayout lay{};
};
struct RayH {
  float o[3], d[3], inv[3], oinv[3], tmin, tmax;
  uint32_t seed;
};
static const uint32_t DONE = 0x7fffffffu;
static const uint32_t kStackTotal = 39u + 9u;  // pt_device.h PTGS_STACK + PTGS_STACK_OVF

static uint32_t tri_gid(const float* T) { uint32_t g; std::memcpy(&g, T + 11, 4); return g; }
static bool accept(uint32_t gid, uint32_t seed) {  // any pure function of (triangle, seed)
  uint32_t s = seed ^ (gid * 0x9E3779B9u);
  s = s * 747796405u + 2891336453u;
  return (((s >> 15) ^ s) & 3u) != 0u;
}
// pt_device.h tri_isect + the old walk's range test
static bool tri_old(const RayH& r, const float* T) {
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
  const float t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv_det;
  return t >= r.tmin && t <= r.tmax;
}
// leaf_any's folded form: every expression evaluated, one predicate
static bool tri_new(const RayH& r, const float* T) {
  const float* v0 = T; const float* e1 = T + 4; const float* e2 = T + 8;
  const float p[3] = {r.d[1] * e2[2] - r.d[2] * e2[1], r.d[2] * e2[0] - r.d[0] * e2[2], r.d[0] * e2[1] - r.d[1] * e2[0]};
  const float det = e1[0] * p[0] + e1[1] * p[1] + e1[2] * p[2];
  const float inv_det = 1.0f / det;
  const float tv[3] = {r.o[0] - v0[0], r.o[1] - v0[1], r.o[2] - v0[2]};
  const float u = (tv[0] * p[0] + tv[1] * p[1] + tv[2] * p[2]) * inv_det;
  const float q[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
  const float v = (r.d[0] * q[0] + r.d[1] * q[1] + r.d[2] * q[2]) * inv_det;
  const float t = (e2[0] * q[0] + e2[1] * q[1] + e2[2] * q[2]) * inv_det;
  return (det != 0.0f) & !(u < 0.0f) & !(u > 1.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t >= r.tmin) & (t <= r.tmax);
}
static bool tri_occludes(const Tree& tr, const RayH& r, uint32_t slot, bool folded) {
  const float* T = &tr.tris[12 * (size_t)slot];
  if (!(folded ? tri_new(r, T) : tri_old(r, T))) return false;
  if (tr.flags[slot] & 1u) return accept(tri_gid(T), r.seed);
  return true;
}
static bool brute(const Tree& tr, const RayH& r) {
  for (size_t s = 0; s < tr.flags.size(); ++s)
    if (tri_occludes(tr, r, (uint32_t)s, false)) return true;
  return false;
}

// box4_q with the constant cap of trace_any
static void box4(const Tree& tr, const RayH& r, uint32_t node, bool hit[4], uint32_t c[4]) {
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
    const float f = std::fmin(std::fmin(std::fmin(q1[0], q1[1]), q1[2]), r.tmax);
    hit[j] = (n <= f * 1.0000004f) && (j < 2 || o[12 + j] != 0u);
    c[j] = o[12 + j];
  }
}

struct Lane {
  RayH r;
  bool active = false;   // part of the wave's launch
  bool in = false;       // still in the walk (not returned)
  bool result = false;
  uint32_t node = 0, leaf = DONE, sp = 0, hw = 0;
  std::vector<uint32_t> stack;
};
struct Stats {
  unsigned long long node_steps = 0, tri_steps = 0, lane_nodes = 0, lane_tris = 0, hw = 0;
};

static void push(const Tree& tr, Lane& l, bool in_loop, uint32_t c) {
  if (!in_loop) { ++g_viol; return; }  // a lane outside the node loop (inactive / done) never writes
  if (l.sp >= tr.need || l.sp >= kStackTotal) { ++g_viol; return; }
  l.stack[l.sp++] = c;
  if (l.sp > l.hw) l.hw = l.sp;
}
static uint32_t pop(Lane& l) {
  if (!l.sp) return DONE;
  return l.stack[--l.sp];
}
static void leaf_span(const Tree& tr, uint32_t link, uint32_t& start, uint32_t& count) {  // leaf_range<true>
  start = link & tr.lay.leaf_start_mask;
  count = ((link & 0x7fffffffu) >> tr.lay.leaf_shift) + 1u;
}

// the walk before: two returns, a continue, the `have` chain
static void walk_old(const Tree& tr, Lane* L, Stats& st) {
  for (;;) {
    bool any_in = false;
    for (int i = 0; i < 64; ++i) any_in |= L[i].in;
    if (!any_in) return;
    // while (node >= 0)
    for (;;) {
      bool any = false;
      bool N[64];
      for (int i = 0; i < 64; ++i) { N[i] = L[i].in && (int32_t)L[i].node >= 0; any |= N[i]; }
      if (!any) break;
      ++st.node_steps;
      for (int i = 0; i < 64; ++i) {
        if (!N[i]) continue;
        Lane& l = L[i];
        ++st.lane_nodes;
        bool hit[4]; uint32_t c[4];
        box4(tr, l.r, l.node, hit, c);
        bool have = false;
        uint32_t next = 0x80000000u;
        for (int j = 0; j < 4; ++j)
          if (hit[j]) {
            if (!have) { next = c[j]; have = true; }
            else push(tr, l, true, c[j]);
          }
        if (!have) {
          if (l.sp == 0) { l.in = false; l.result = false; continue; }
          l.node = pop(l);
          continue;
        }
        l.node = next;
      }
    }
    // the leaf of every lane still in
    unsigned long long iters = 0;
    for (int i = 0; i < 64; ++i) {
      Lane& l = L[i];
      if (!l.in) continue;
      uint32_t start, count;
      leaf_span(tr, l.node, start, count);
      unsigned long long k = 0;
      for (; k < count;) {
        ++st.lane_tris;
        const bool occ = tri_occludes(tr, l.r, start + (uint32_t)k, false);
        ++k;
        if (occ) { l.in = false; l.result = true; break; }
      }
      if (k > iters) iters = k;
      if (l.in) {
        if (l.sp == 0) { l.in = false; l.result = false; }
        else l.node = pop(l);
      }
    }
    st.tri_steps += iters;
  }
}

// the single-exit walk, with or without the postponed leaf
static void walk_new(const Tree& tr, Lane* L, bool park, Stats& st) {
  bool occluded[64] = {};
  for (;;) {
    bool any_in = false;
    for (int i = 0; i < 64; ++i) any_in |= L[i].in;
    if (!any_in) return;
    // while (node >= 0 && node != DONE)
    bool N[64];
    for (int i = 0; i < 64; ++i) N[i] = L[i].in && (int32_t)L[i].node >= 0 && L[i].node != DONE;
    for (;;) {
      bool any = false;
      for (int i = 0; i < 64; ++i) any |= N[i];
      if (!any) break;
      ++st.node_steps;
      // the four children's hit masks over the lanes in the loop (Box4::hm: ballots under exec)
      unsigned long long h[4] = {0, 0, 0, 0};
      uint32_t c[64][4];
      for (int i = 0; i < 64; ++i) {
        if (!N[i]) continue;
        ++st.lane_nodes;
        bool hit[4];
        box4(tr, L[i].r, L[i].node, hit, c[i]);
        for (int j = 0; j < 4; ++j) h[j] |= (unsigned long long)hit[j] << i;
      }
      const unsigned long long o01 = h[0] | h[1], o012 = o01 | h[2];
      const unsigned long long anyc = o012 | h[3], p1 = h[0] & h[1], p2 = o01 & h[2], p3 = o012 & h[3];
      for (int i = 0; i < 64; ++i) {
        // (the masks' bits outside the loop's lanes would be stores by lanes that are not in it)
        const unsigned long long bit = 1ull << i;
        if (!N[i]) {
          if ((p1 | p2 | p3) & bit) push(tr, L[i], false, 0);
          continue;
        }
        Lane& l = L[i];
        if (anyc & bit) {
          if (p1 & bit) push(tr, l, true, c[i][1]);
          if (p2 & bit) push(tr, l, true, c[i][2]);
          if (p3 & bit) push(tr, l, true, c[i][3]);
          uint32_t node = c[i][3];
          if (h[2] & bit) node = c[i][2];
          if (h[1] & bit) node = c[i][1];
          if (h[0] & bit) node = c[i][0];
          l.node = node;
        } else {
          l.node = pop(l);
        }
        if (park && (int32_t)l.node < 0 && l.leaf == DONE) {
          l.leaf = l.node;
          l.node = pop(l);
        }
      }
      if (park) {  // every lane of this iteration holds a leaf or is done
        bool all = true;
        for (int i = 0; i < 64; ++i)
          if (N[i] && !(L[i].leaf != DONE || L[i].node == DONE)) all = false;
        if (all) break;
      }
      for (int i = 0; i < 64; ++i) N[i] = N[i] && (int32_t)L[i].node >= 0 && L[i].node != DONE;
    }
    // one leaf site
    unsigned long long iters = 0;
    for (int i = 0; i < 64; ++i) {
      Lane& l = L[i];
      if (!l.in) continue;
      uint32_t link = DONE;
      if (park) link = l.leaf;
      else if ((int32_t)l.node < 0) link = l.node;
      if (link != DONE) {
        uint32_t start, count;
        leaf_span(tr, link, start, count);
        unsigned long long k = 0;
        bool occ = false;
        for (; k < count && !occ; ++k) {
          ++st.lane_tris;
          occ = tri_occludes(tr, l.r, start + (uint32_t)k, true);
        }
        if (k > iters) iters = k;
        occluded[i] = occ;
      }
      if (park) {
        if (link != DONE) {
          l.leaf = DONE;
          if (occluded[i]) l.node = DONE;
        }
        if ((int32_t)l.node < 0) {
          l.leaf = l.node;
          l.node = pop(l);
        }
        if (l.node == DONE && l.leaf == DONE) { l.in = false; l.result = occluded[i]; }
      } else {
        if (link != DONE) {
          l.node = pop(l);
          if (occluded[i]) l.node = DONE;
        }
        if (l.node == DONE) { l.in = false; l.result = occluded[i]; }
      }
    }
    st.tri_steps += iters;
  }
}

static void reset(const Tree& tr, Lane* L) {
  for (int i = 0; i < 64; ++i) {
    Lane& l = L[i];
    l.in = l.active && tr.num > 0;
    l.result = false;
    l.node = 0; l.leaf = DONE; l.sp = 0; l.hw = 0;
    l.stack.assign(tr.need ? tr.need : 1, 0u);
  }
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: anyhit_walk_check tris.bin leaf fan depth waves\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leafsz = atoi(argv[2]), fan = atoi(argv[3]), waves = atoi(argv[5]);
  const uint32_t depth = (uint32_t)atoi(argv[4]);

  Tree tr;
  float blo[3] = {-1.0f, -1.0f, -1.0f}, bhi[3] = {1.0f, 1.0f, 1.0f};
  if (raw.size() >= 9) {
    std::vector<BuildTri> tris(raw.size() / 9);
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
    BvhOut bvh;
    build_bvh(tris, leafsz, depth, bvh);
    uint32_t dep4 = 0;
    collapse_bvh4(bvh.nodes, tr.n4, tr.num, tr.need, dep4, fan);
    tr.tris.swap(bvh.tris);
    tr.flags.swap(bvh.tri_flags);
  }
  if (!make_traversal_nodes(tr.n4.data(), tr.num, -1, tr.n64, tr.lay)) {
    printf("anyhit_walk_check: conversion refused\n");
    return 1;
  }
  if (tr.num >= DONE) ++g_viol;  // no interior index reaches the sentinel

  const float ext[3] = {bhi[0] - blo[0], bhi[1] - blo[1], bhi[2] - blo[2]};
  const float diag = std::sqrt(ext[0] * ext[0] + ext[1] * ext[1] + ext[2] * ext[2]);
  Stats so, ss, sp;
  unsigned long long nrays = 0, nocc = 0, hw = 0, k = 0;
  std::vector<Lane> lanes(64);
  Lane* L = lanes.data();
  for (int w = 0; w < waves; ++w) {
    const uint32_t nact = 1u + urand32() % 64u;
    for (int i = 0; i < 64; ++i) L[i].active = false;
    for (uint32_t a = 0; a < nact;) {
      const uint32_t i = urand32() % 64u;
      if (!L[i].active) { L[i].active = true; ++a; }
    }
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
      // 1e-3 x the diagonal .. 1e4, log-uniform
      const float lo = std::log(1e-3f * diag), hi = std::log(1e4f);
      r.tmax = mode == 0 ? len - 0.005f : std::exp(lo + urand() * (hi - lo));
      r.seed = urand32();
      ++k;
      ++nrays;
    }
    bool ref[64];
    reset(tr, L);
    walk_old(tr, L, so);
    for (int i = 0; i < 64; ++i) {
      if (!L[i].active) continue;
      ref[i] = L[i].result;
      nocc += ref[i];
      if (L[i].hw > hw) hw = L[i].hw;
      if (brute(tr, L[i].r) != ref[i]) ++g_viol;
    }
    for (int v = 0; v < 2; ++v) {
      reset(tr, L);
      walk_new(tr, L, v == 1, v == 1 ? sp : ss);
      for (int i = 0; i < 64; ++i) {
        if (!L[i].active) continue;
        if (L[i].result != ref[i]) ++g_viol;
        if (L[i].hw > hw) hw = L[i].hw;
      }
    }
  }
  printf("anyhit_walk_check nodes %u need %u waves %d rays %llu occluded %llu high_water %llu "
         "node_steps_old %llu node_steps_se %llu node_steps_park %llu tri_steps_old %llu tri_steps_se %llu "
         "tri_steps_park %llu lane_nodes_old %llu lane_nodes_se %llu lane_nodes_park %llu lane_tris_old %llu "
         "lane_tris_se %llu lane_tris_park %llu violations %llu\n",
         tr.num, tr.need, waves, nrays, nocc, hw, so.node_steps, ss.node_steps, sp.node_steps, so.tri_steps,
         ss.tri_steps, sp.tri_steps, so.lane_nodes, ss.lane_nodes, sp.lane_nodes, so.lane_tris, ss.lane_tris,
         sp.lane_tris, g_viol);
  return g_viol ? 1 : 0;
}
