// stack_cull_check — stand-alone host check of the path tracer's packed stack word and its cull at pop
// (stack_key.h, bvh.h stack_layout / pack_links64, pt_device.h trace_closest<.., CULL>).
//
//   stack_cull_check <tris.bin> <leaf> <fan> <depth> <rays> <float-samples>
//
// tris.bin holds float32 triangles (9 floats each; an empty file: the empty tree). The program
//   - key: for every key width 0 .. 31 checks decode(encode(x)) <= x (and decode >= 0) at every binade
//     boundary in [0, 2^15], at its neighbours, at 0, the smallest denormal, FLT_MAX and +inf, and at
//     <float-samples> seeded floats (random bit patterns of non-negative floats); width 0 decodes to 0;
//   - links: builds the host tree as the scene upload does (build_bvh, collapse_bvh4, quantize_bvh4),
//     derives the layout, packs the compact nodes' links and checks every link: it round-trips to the
//     canonical link, the leaf flag is the sign, interior links stay, the link leaves the key's bits clear for
//     every width the layout can get (forced 0 .. 31, clamped to what the links leave);
//   - walk: restates one lane of the kernel's closest-hit walk on the compact nodes (box4_q's float
//     expressions, -ffp-contract=off and explicit fmaf; sorted pushes; postponed leaf) with and without the
//     cull, for the layout's own width and forced widths 0, 3 and 8, with seeded rays (general, one
//     axis-parallel component, origins outside the bounds, as node64_check): the hits must be identical in
//     (t, gid), and when an entry is culled no triangle of its subtree may be one the walk would accept with
//     the hit distance of that moment.
// Prints one line: "stack_cull_check nodes N link_bits R key_bits W floats F links L rays R pops P culled C
// steps_plain A steps_cull B violations V". Exit status 1 when V > 0.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"
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

// ---- key ------------------------------------------------------------------------------------------
static unsigned long long check_key_value(float x) {
  unsigned long long bad = 0;
  for (uint32_t w = 0; w <= 31; ++w) {
    const uint32_t m = stack_key_mask(w);
    const uint32_t word = stack_pack(0u, x, m);
    const float d = stack_bound(word, m);
    if (!(d <= x) || !(d >= 0.0f)) ++bad;
    if (w == 0 && d != 0.0f) ++bad;
    if (word & ~m) ++bad;                        // the key stays in its bits
    if (word & 0x80000000u) ++bad;               // never the leaf flag
    if (stack_link(word | 0x80000005u, m) != (0x80000005u & ~m)) ++bad;
  }
  return bad;
}
static unsigned long long check_keys(unsigned long long samples, unsigned long long& count) {
  unsigned long long bad = 0;
  auto one = [&](float x) { bad += check_key_value(x); ++count; };
  one(0.0f);
  one(stack_u2f(1u));
  one(FLT_MIN);
  one(FLT_MAX);
  one(INFINITY);
  for (int e = -149; e <= 15; ++e) {  // every binade boundary up to 2^15, denormal ones included
    const float b = std::ldexp(1.0f, e);
    one(b);
    one(std::nextafterf(b, 0.0f));
    one(std::nextafterf(b, INFINITY));
  }
  for (unsigned long long i = 0; i < samples; ++i) {
    // half of them anywhere among the non-negative floats, half in the walk's range [2^-10, 2^14)
    uint32_t u = urand32() & 0x7fffffffu;
    if (i & 1u) u = ((117u + urand32() % 24u) << 23) | (u & 0x007fffffu);
    if (u > 0x7f800000u) u = 0x7f800000u;  // (no NaN: tn is an fmaxf against tmin)
    one(stack_u2f(u));
  }
  return bad;
}

// ---- tree -----------------------------------------------------------------------------------------
struct Tree {
  std::vector<float> n4;
  std::vector<uint32_t> n64;  // packed links
  std::vector<float> tris;    // 12 floats per triangle
  uint32_t num = 0;
  StackLayout lay{};
};

static unsigned long long check_links(const Tree& t, unsigned long long& links) {
  unsigned long long bad = 0;
  for (int force = -1; force <= 31; ++force) {
    const StackLayout l = stack_layout(t.n4.data(), t.num, force);
    if (l.ref_bits + l.key_bits > 32u || l.ref_bits < 1u) ++bad;
    if (force >= 0 && l.key_bits != std::min((uint32_t)force, 32u - l.ref_bits)) ++bad;
    if (force < 0 && l.key_bits != 0u && l.key_bits < PTGS_STACK_KEY_MIN) ++bad;
    if (l.key_mask != stack_key_mask(l.key_bits) || l.leaf_start_mask != (1u << l.leaf_shift) - 1u) ++bad;
    if (l.leaf_shift != t.lay.leaf_shift || l.ref_bits != t.lay.ref_bits) ++bad;
    for (uint32_t i = 0; i < t.num; ++i)
      for (int j = 0; j < 4; ++j) {
        int32_t canon;
        std::memcpy(&canon, &t.n4[32 * (size_t)i + 24 + j], 4);
        const uint32_t p = t.n64[PTGS_NODE64_DWORDS * (size_t)i + 12 + j];
        if (force < 0) ++links;
        if (p != stack_link_pack(canon, l)) ++bad;
        if (stack_link_unpack(p, l) != canon) ++bad;
        if (((int32_t)p < 0) != (canon < 0)) ++bad;
        if (canon >= 0 && p != (uint32_t)canon) ++bad;
        if (p & l.key_mask) ++bad;
        if (l.ref_bits < 32u && (p & 0x7fffffffu) >> (l.ref_bits - 1u)) ++bad;  // payload within its bits
        if (p == (0x7fffffffu & ~l.key_mask)) ++bad;                            // never the walk's DONE
        // a word with any key round-trips to the link
        if (stack_link(stack_pack(p, 1234.5f, l.key_mask), l.key_mask) != p) ++bad;
      }
  }
  return bad;
}

// ---- walk -----------------------------------------------------------------------------------------
struct RayH {
  float o[3], d[3], inv[3], oinv[3], tmin, tmax;
};
struct HitH {
  float t;
  uint32_t gid;
};
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
static uint32_t tri_gid(const float* T) { uint32_t g; std::memcpy(&g, T + 11, 4); return g; }
static bool accepts(const RayH& r, const float* T, const HitH& h, float& t) {  // leaf_closest's tests
  if (!tri_isect(r, T, t)) return false;
  if (!(t >= r.tmin && t <= h.t)) return false;
  if (t == h.t && tri_gid(T) >= h.gid) return false;
  return true;
}
static void leaf(const Tree& tr, const StackLayout& l, const RayH& r, uint32_t link, HitH& h, unsigned long long& tt) {
  const uint32_t start = link & l.leaf_start_mask, count = ((link & 0x7fffffffu) >> l.leaf_shift) + 1u;  // leaf_range<true>
  for (uint32_t k = 0; k < count; ++k) {
    ++tt;
    float t;
    const float* T = &tr.tris[12 * (size_t)(start + k)];
    if (accepts(r, T, h, t)) { h.t = t; h.gid = tri_gid(T); }
  }
}
// a triangle under this packed link that the walk would accept now?
static bool subtree_accepts(const Tree& tr, const StackLayout& l, const RayH& r, uint32_t link, const HitH& h) {
  if ((int32_t)link < 0) {
    const uint32_t start = link & l.leaf_start_mask, count = ((link & 0x7fffffffu) >> l.leaf_shift) + 1u;
    for (uint32_t k = 0; k < count; ++k) {
      float t;
      if (accepts(r, &tr.tris[12 * (size_t)(start + k)], h, t)) return true;
    }
    return false;
  }
  const uint32_t* o = &tr.n64[PTGS_NODE64_DWORDS * (size_t)link];
  for (int j = 0; j < 4; ++j) {
    if (o[12 + j] == 0u) continue;  // (the root is never a child)
    if (subtree_accepts(tr, l, r, o[12 + j], h)) return true;
  }
  return false;
}

struct WalkStats {
  unsigned long long steps = 0, tris = 0, pops = 0, culled = 0;
};
static HitH walk(const Tree& tr, const StackLayout& l, const RayH& r, bool cull, WalkStats& ws) {
  HitH h{r.tmax, 0xffffffffu};
  if (tr.num == 0) return h;
  std::vector<uint32_t> stack;
  const uint32_t km = l.key_mask;
  // (the kernel's DONE: key bits clear, so the empty stack pops as an entry bounded by 0.0; never a link)
  const uint32_t DONE = cull ? (0x7fffffffu & ~km) : 0x7fffffffu;
  if (tr.num > DONE) ++g_viol;
  auto pop = [&]() -> uint32_t {
    if (!cull) {
      if (stack.empty()) return DONE;
      const uint32_t x = stack.back();
      stack.pop_back();
      return x;
    }
    const float cap = h.t * 1.0000004f;
    for (;;) {
      uint32_t x = DONE;
      const bool had = !stack.empty();
      if (had) { x = stack.back(); stack.pop_back(); ++ws.pops; }
      if (!(stack_bound(x, km) > cap)) return stack_link(x, km);
      if (!had) { ++g_viol; return DONE; }  // the sentinel itself is never culled
      ++ws.culled;
      if (subtree_accepts(tr, l, r, stack_link(x, km), h)) ++g_viol;
    }
  };
  uint32_t node = 0, parked = DONE;
  for (;;) {
    while ((int32_t)node >= 0 && node != DONE) {
      ++ws.steps;
      const uint32_t* o = &tr.n64[PTGS_NODE64_DWORDS * (size_t)node];
      float org[3], step[3];
      std::memcpy(org, o, 12);
      std::memcpy(step, o + 3, 12);
      float tn[4];
      uint32_t c[4];
      bool hit[4];
      for (int j = 0; j < 4; ++j) {  // box4_q
        float n = r.tmin, f = h.t;
        float q0[3], q1[3];
        for (int a = 0; a < 3; ++a) {
          const bool neg = r.inv[a] < 0.0f;
          const float s = step[a] * r.inv[a], cc = std::fmaf(org[a], r.inv[a], -r.oinv[a]);
          q0[a] = std::fmaf(qbyte(o[6 + 2 * a + (neg ? 1 : 0)], j), s, cc);
          q1[a] = std::fmaf(qbyte(o[6 + 2 * a + (neg ? 0 : 1)], j), s, cc);
        }
        n = std::fmax(std::fmax(q0[0], q0[1]), std::fmax(q0[2], r.tmin));
        f = std::fmin(std::fmin(std::fmin(q1[0], q1[1]), q1[2]), h.t);
        hit[j] = (n <= f * 1.0000004f) && (j < 2 || o[12 + j] != 0u);
        tn[j] = hit[j] ? n : INFINITY;
        c[j] = o[12 + j];
      }
      auto cswap = [&](int i, int j) {
        if (tn[j] < tn[i]) { std::swap(tn[i], tn[j]); std::swap(c[i], c[j]); }
      };
      if (!(hit[0] || hit[1] || hit[2] || hit[3])) {
        node = pop();
      } else {
        cswap(0, 1); cswap(2, 3); cswap(0, 2); cswap(1, 3); cswap(1, 2);
        for (int j = 3; j >= 1; --j)
          if (tn[j] != INFINITY) {
            if (!(tn[j] >= 0.0f)) ++g_viol;  // the key's precondition
            stack.push_back(cull ? stack_pack(c[j], tn[j], km) : c[j]);
          }
        node = c[0];
      }
      if ((int32_t)node < 0 && parked == DONE) {
        parked = node;
        node = pop();
      }
      if (parked != DONE || node == DONE) break;
    }
    if (parked != DONE) {
      leaf(tr, l, r, parked, h, ws.tris);
      parked = DONE;
    }
    if ((int32_t)node < 0) {
      leaf(tr, l, r, node, h, ws.tris);
      node = pop();
    }
    if (node == DONE) return h;
  }
}

int main(int argc, char** argv) {
  if (argc < 7) { fprintf(stderr, "usage: stack_cull_check tris.bin leaf fan depth rays float-samples\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leafsz = atoi(argv[2]), fan = atoi(argv[3]), rays = atoi(argv[5]);
  const uint32_t depth = (uint32_t)atoi(argv[4]);
  const unsigned long long samples = strtoull(argv[6], nullptr, 10);

  unsigned long long floats = 0;
  g_viol += check_keys(samples, floats);

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
    uint32_t need = 0, dep4 = 0;
    collapse_bvh4(bvh.nodes, tr.n4, tr.num, need, dep4, fan);
    tr.tris.swap(bvh.tris);
  }
  if (!make_traversal_nodes(tr.n4.data(), tr.num, -1, tr.n64, tr.lay)) {
    printf("stack_cull_check: conversion refused\n");
    return 1;
  }
  unsigned long long links = 0;
  g_viol += check_links(tr, links);
  if (tr.num == 0 && (tr.lay.ref_bits != 1u || tr.lay.key_bits != 31u || tr.lay.leaf_shift != 0u)) ++g_viol;

  WalkStats plain, own;
  unsigned long long nrays = 0;
  const int forced[4] = {-1, 0, 3, 8};
  for (int k = 0; k < rays; ++k) {
    ++nrays;
    RayH r;
    const int mode = k % 4;  // 0, 1: general; 2: one axis-parallel component; 3: origin outside the bounds
    float len = 0.0f;
    for (int a = 0; a < 3; ++a) {
      const float ext = bhi[a] - blo[a];
      const float u = mode == 3 ? (urand() * 3.0f - 1.0f) : urand();
      r.o[a] = blo[a] + u * ext;
      float d = urand() * 2.0f - 1.0f;
      if (mode == 2 && a == k / 4 % 3) d = (k & 8) ? 0.0f : -0.0f;
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
    const HitH ref = walk(tr, tr.lay, r, false, plain);
    for (int f = 0; f < 4; ++f) {
      const StackLayout l = forced[f] < 0 ? tr.lay : stack_layout(tr.n4.data(), tr.num, forced[f]);
      WalkStats tmp;
      const HitH got = walk(tr, l, r, true, forced[f] < 0 ? own : tmp);
      if (std::memcmp(&got.t, &ref.t, 4) != 0 || got.gid != ref.gid) ++g_viol;
      if (forced[f] == 0 && tmp.culled != 0) ++g_viol;  // zero key bits never cull
    }
  }
  printf("stack_cull_check nodes %u link_bits %u key_bits %u floats %llu links %llu rays %llu pops %llu culled %llu "
         "steps_plain %llu steps_cull %llu tris_plain %llu tris_cull %llu violations %llu\n",
         tr.num, tr.lay.ref_bits, tr.lay.key_bits, floats, links, nrays, own.pops, own.culled, plain.steps, own.steps,
         plain.tris, own.tris, g_viol);
  return g_viol ? 1 : 0;
}
