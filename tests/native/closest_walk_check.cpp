// closest_walk_check — stand-alone host check of the node step of the path tracer's closest-hit walk
// (pt_device.h trace_closest<.., N64, CULL>, and the one-pop-site forms of tools/patches/pt_one_pop_rejected.patch).
//
//   closest_walk_check <tris.bin> <leaf> <fan> <depth> <waves>
//
// tris.bin holds float32 triangles (9 floats each; an empty file: the empty tree). The program builds the
// host tree as the scene upload does (build_bvh, collapse_bvh4, make_traversal_nodes) and restates the walk as
// a 64-lane lockstep model: the lanes of a wave that are in a loop run its body together and the loop ends when
// the last of them leaves (or at the wave-uniform break), as the hardware's exec mask does it. The float
// expressions are the kernel's (box4_q, tri_isect and leaf_closest's tests; -ffp-contract=off, explicit fmaf);
// the stack holds the packed words (stack_key.h) and pop drops every word whose bound is above the hit distance
// of that moment. Three walks are modelled:
//   old  two pop sites in the node step (the walk that ships): the "no child hit" pop of enter_box4, and the pop
//        after the entered leaf is parked;
//   b1   one site (the patch's form 1): a lane that pops a leaf while it holds none parks it and pops again,
//        a second pass of the one pop loop;
//   b2   one site, one pop (the patch's form 2): a leaf popped by a lane with no hit child leaves the node loop
//        in `node`.
// The node loop's test is the kernel's one unsigned compare in b1 and b2 and the two signed compares it replaced
// in old.
// Rays, all seeded, four kinds in turn: two of a general direction from a point of the scene bounds, one with an
// axis-parallel component (+0 / -0), one with its origin outside the bounds; tmax 1e4. Each wave has a random
// subset of 1 to 64 active lanes, so the break ballot sees inactive lanes.
// Violations: a walk's (t, gid) differs from a brute-force test of every triangle (leaf_closest's tests in
// triangle order); a stack write at or above the tree's stack need (collapse_bvh4's max_stack) or above the
// kernel's PTGS_STACK + PTGS_STACK_OVF; a stack write by a lane that is not in the node loop; b1's per-lane
// sequence of visited nodes and leaves differs from old's; an interior index that reaches DONE.
// Prints one line of "name value" pairs (the modelled wave and lane node steps of the three walks among them);
// exit status 1 when violations > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"
#include "stack_key.h"

using namespace ptgs;

static uint32_t g_rng = 97531u;
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
  uint32_t num = 0, need = 0;
  StackLayout lay{};
  uint32_t done = 0x7fffffffu;  // the culling walk's DONE: the key's bits clear
};
struct RayH {
  float o[3], d[3], inv[3], oinv[3], tmin, tmax;
};
struct HitH {
  float t;
  uint32_t gid;
};
static const uint32_t kStackTotal = 39u + 9u;  // pt_device.h PTGS_STACK + PTGS_STACK_OVF

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
static HitH brute(const Tree& tr, const RayH& r) {
  HitH h{r.tmax, 0xffffffffu};
  for (size_t s = 0; s < tr.tris.size() / 12; ++s) tri_closest(r, &tr.tris[12 * s], h);
  return h;
}

// box4_q with the walk's shrinking cap
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
  uint32_t node = 0, leaf = 0, sp = 0, hw = 0;
  std::vector<uint32_t> stack;
  std::vector<uint32_t> visits;  // node indices and leaf links, in the order the lane tests them
};
struct Stats {
  unsigned long long node_steps = 0, lane_nodes = 0, leaf_phases = 0, lane_leaves = 0, pops = 0, culled = 0;
};

static void push(const Tree& tr, Lane& l, bool in_loop, uint32_t c, float tn) {
  if (!in_loop) { ++g_viol; return; }  // a lane outside the node loop (inactive / done / holding two leaves) never writes
  if (l.sp >= tr.need || l.sp >= kStackTotal) { ++g_viol; return; }
  if (!(tn >= 0.0f)) ++g_viol;  // the key's precondition
  l.stack[l.sp++] = stack_pack(c, tn, tr.lay.key_mask);
  if (l.sp > l.hw) l.hw = l.sp;
}
// one pass of pop()'s loop body: the word, or DONE from the empty stack (a word bounded by 0.0: never culled)
static uint32_t pop_word(const Tree& tr, Lane& l, Stats& st) {
  if (!l.sp) return tr.done;
  ++st.pops;
  return l.stack[--l.sp];
}
static uint32_t pop(const Tree& tr, Lane& l, Stats& st) {
  const float cap = l.h.t * 1.0000004f;
  const uint32_t km = tr.lay.key_mask;
  uint32_t x;
  for (;;) {
    x = pop_word(tr, l, st);
    if (!(stack_bound(x, km) > cap)) break;
    ++st.culled;
  }
  return stack_link(x, km);
}
// form b1: the one loop, whose condition is "culled, or parked"
static uint32_t pop_park(const Tree& tr, Lane& l, Stats& st) {
  const float cap = l.h.t * 1.0000004f;
  const uint32_t km = tr.lay.key_mask;
  uint32_t n;
  bool again;
  do {
    const uint32_t x = pop_word(tr, l, st);
    n = stack_link(x, km);
    again = stack_bound(x, km) > cap;
    if (again) ++st.culled;
    if (!again && (int32_t)n < 0 && l.leaf == tr.done) {
      l.leaf = n;
      again = true;
    }
  } while (again);
  return n;
}
static void leaf_closest(const Tree& tr, Lane& l, uint32_t link) {
  const uint32_t start = link & tr.lay.leaf_start_mask, count = ((link & 0x7fffffffu) >> tr.lay.leaf_shift) + 1u;  // leaf_range<true>
  l.visits.push_back(link);
  for (uint32_t k = 0; k < count; ++k) tri_closest(l.r, &tr.tris[12 * (size_t)(start + k)], l.h);
}

// variant 0: old, 1: b1, 2: b2
static void walk(const Tree& tr, Lane* L, int variant, Stats& st) {
  const uint32_t DONE = tr.done;
  auto interior = [&](uint32_t node) {
    if (variant == 0) return (int32_t)node >= 0 && node != DONE;
    return node < DONE;  // (leaves have bit 31; DONE is above every interior index)
  };
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
      // the four children's hit masks over the lanes in the loop (Box4::hm: ballots under exec)
      unsigned long long hm[4] = {0, 0, 0, 0};
      uint32_t c[64][4];
      float tn[64][4];
      for (int i = 0; i < 64; ++i) {
        if (!N[i]) continue;
        ++st.lane_nodes;
        L[i].visits.push_back(L[i].node);
        bool hit[4];
        box4(tr, L[i].r, L[i].node, L[i].h.t, hit, tn[i], c[i]);
        for (int j = 0; j < 4; ++j) hm[j] |= (unsigned long long)hit[j] << i;
      }
      const unsigned long long a01 = hm[0] & hm[1], o01 = hm[0] | hm[1], a23 = hm[2] & hm[3], o23 = hm[2] | hm[3];
      const unsigned long long anyc = o01 | o23, p3 = a01 & a23, p2 = (a01 & o23) | (o01 & a23), p1 = a01 | a23 | (o01 & o23);
      for (int i = 0; i < 64; ++i) {
        const unsigned long long bit = 1ull << i;
        if (!N[i]) {
          // (the masks' bits outside the loop's lanes would be stores by lanes that are not in it)
          if ((p1 | p2 | p3) & bit) push(tr, L[i], false, 0, 0.0f);
          continue;
        }
        Lane& l = L[i];
        bool need = !(anyc & bit);
        if (!need) {  // enter_box4 with a hit child: sorted, farthest pushed first
          auto cswap = [&](int a, int b) {
            if (tn[i][b] < tn[i][a]) { std::swap(tn[i][a], tn[i][b]); std::swap(c[i][a], c[i][b]); }
          };
          cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
          if (p3 & bit) push(tr, l, true, c[i][3], tn[i][3]);
          if (p2 & bit) push(tr, l, true, c[i][2], tn[i][2]);
          if (p1 & bit) push(tr, l, true, c[i][1], tn[i][1]);
          // (the masks count the hit children: what they push is a hit child, never an empty slot)
          for (int j = 1; j < 4; ++j)
            if ((((j == 1 ? p1 : j == 2 ? p2 : p3) & bit) != 0) != (tn[i][j] != INFINITY)) ++g_viol;
          l.node = c[i][0];
        }
        if (variant == 0) {
          if (need) l.node = pop(tr, l, st);  // (enter_box4's pop)
          if ((int32_t)l.node < 0 && l.leaf == DONE) {
            l.leaf = l.node;
            l.node = pop(tr, l, st);  // (the second site)
          }
        } else {
          if (!need && (int32_t)l.node < 0 && l.leaf == DONE) {
            l.leaf = l.node;
            need = true;
          }
          if (need) l.node = variant == 1 ? pop_park(tr, l, st) : pop(tr, l, st);
        }
      }
      // every lane of this iteration holds a leaf or is done (b2: or holds a popped leaf in `node`)
      bool all = true;
      for (int i = 0; i < 64; ++i)
        if (N[i] && !(L[i].leaf != DONE || (variant == 2 ? L[i].node >= DONE : L[i].node == DONE))) all = false;
      if (all) break;
      for (int i = 0; i < 64; ++i) N[i] = N[i] && interior(L[i].node);
    }
    bool any_leaf = false;
    for (int i = 0; i < 64; ++i) {
      Lane& l = L[i];
      if (!l.in) continue;
      if (l.leaf != DONE) {
        any_leaf = true;
        ++st.lane_leaves;
        leaf_closest(tr, l, l.leaf);
        l.leaf = DONE;
      }
      if ((int32_t)l.node < 0) {
        leaf_closest(tr, l, l.node);
        l.node = pop(tr, l, st);
      }
      if (l.node == DONE) l.in = false;
    }
    st.leaf_phases += any_leaf;
  }
}

static void reset(const Tree& tr, Lane* L) {
  for (int i = 0; i < 64; ++i) {
    Lane& l = L[i];
    l.in = l.active && tr.num > 0;
    l.h = HitH{l.r.tmax, 0xffffffffu};
    l.node = 0; l.leaf = tr.done; l.sp = 0; l.hw = 0;
    l.stack.assign(tr.need ? tr.need : 1, 0u);
    l.visits.clear();
  }
}

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: closest_walk_check tris.bin leaf fan depth waves\n"); return 2; }
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
      t.mesh = 0; t.prim = (uint32_t)i; t.gid = (uint32_t)i; t.flags = 0;
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
  }
  if (!make_traversal_nodes(tr.n4.data(), tr.num, -1, tr.n64, tr.lay)) {
    printf("closest_walk_check: conversion refused\n");
    return 1;
  }
  tr.done = 0x7fffffffu & ~tr.lay.key_mask;
  if (tr.num > tr.done) ++g_viol;  // no interior index reaches the sentinel: the unsigned loop test rests on it
  for (uint32_t i = 0; i < tr.num; ++i)
    for (int j = 0; j < 4; ++j) {
      const uint32_t p = tr.n64[PTGS_NODE64_DWORDS * (size_t)i + 12 + j];
      if ((int32_t)p >= 0 && p >= tr.done) ++g_viol;  // an interior link below DONE
      if ((int32_t)p < 0 && !(p > tr.done)) ++g_viol;  // a leaf link above it, as unsigned
    }

  const float ext[3] = {bhi[0] - blo[0], bhi[1] - blo[1], bhi[2] - blo[2]};
  Stats s[3];
  unsigned long long nrays = 0, nhit = 0, hw = 0, k = 0, seq_diff = 0, b2_seq_diff = 0;
  std::vector<Lane> lanes(64);
  Lane* L = lanes.data();
  std::vector<std::vector<uint32_t>> seq(64);
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
      const int mode = (int)(k % 4);  // 0, 1: general; 2: one axis-parallel component; 3: origin outside the bounds
      float len = 0.0f;
      for (int a = 0; a < 3; ++a) {
        const float u = mode == 3 ? (urand() * 3.0f - 1.0f) : urand();
        r.o[a] = blo[a] + u * ext[a];
        float d = urand() * 2.0f - 1.0f;
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
      r.tmax = 10000.0f;
      ++k;
      ++nrays;
    }
    HitH ref[64];
    for (int i = 0; i < 64; ++i)
      if (L[i].active) {
        ref[i] = brute(tr, L[i].r);
        nhit += ref[i].gid != 0xffffffffu;
      }
    for (int v = 0; v < 3; ++v) {
      reset(tr, L);
      walk(tr, L, v, s[v]);
      for (int i = 0; i < 64; ++i) {
        if (!L[i].active) continue;
        if (std::memcmp(&L[i].h.t, &ref[i].t, 4) != 0 || L[i].h.gid != ref[i].gid) ++g_viol;
        if (L[i].sp != 0 && tr.num > 0) ++g_viol;  // the walk ends on the empty stack
        if (L[i].hw > hw) hw = L[i].hw;
        if (v == 0) seq[i] = L[i].visits;
        if (v == 1 && L[i].visits != seq[i]) { ++seq_diff; ++g_viol; }
        if (v == 2 && L[i].visits != seq[i]) ++b2_seq_diff;  // (reported, allowed: the speculation differs)
      }
    }
  }
  printf("closest_walk_check nodes %u need %u key_bits %u waves %d rays %llu hits %llu high_water %llu "
         "node_steps_old %llu node_steps_b1 %llu node_steps_b2 %llu lane_nodes_old %llu lane_nodes_b1 %llu "
         "lane_nodes_b2 %llu leaf_phases_old %llu leaf_phases_b1 %llu leaf_phases_b2 %llu lane_leaves_old %llu "
         "lane_leaves_b1 %llu lane_leaves_b2 %llu pops_old %llu pops_b1 %llu pops_b2 %llu culled_old %llu "
         "culled_b1 %llu culled_b2 %llu seq_diff_b1 %llu seq_diff_b2 %llu violations %llu\n",
         tr.num, tr.need, tr.lay.key_bits, waves, nrays, nhit, hw, s[0].node_steps, s[1].node_steps, s[2].node_steps,
         s[0].lane_nodes, s[1].lane_nodes, s[2].lane_nodes, s[0].leaf_phases, s[1].leaf_phases, s[2].leaf_phases,
         s[0].lane_leaves, s[1].lane_leaves, s[2].lane_leaves, s[0].pops, s[1].pops, s[2].pops, s[0].culled,
         s[1].culled, s[2].culled, seq_diff, b2_seq_diff, g_viol);
  return g_viol ? 1 : 0;
}
