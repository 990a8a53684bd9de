// node64_check — stand-alone host check of the compact 64-B traversal nodes (bvh.h quantize_bvh4).
//
//   node64_check <tris.bin> <leaf> <fan> <depth> <rays-per-node>
//
// tris.bin holds float32 triangles (9 floats each). The program builds the host tree as the scene upload
// does (build_bvh, collapse_bvh4), converts it, and restates the kernel's decode (pt_device.h box4_q) with
// the same float expressions (compiled with -ffp-contract=off, explicit fmaf):
//   - unit ray (inv = 1, o = 0): the decoded planes fmaf(q, step, origin) contain the canonical box;
//   - seeded rays with origins in and around the scene's bounds, axis-parallel directions included: per
//     axis the compact near distance is <= the canonical one and the far distance >= it, so the slab
//     interval can only widen;
//   - empty slots hold the inverted planes and link 0 and the restated test (with its link compare) misses
//     them for every ray; the links equal the canonical links.
// Prints one line: "node64_check nodes N children C empty E rays R violations V". Exit status 1 when V > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"

using namespace ptgs;

static uint32_t g_rng = 12345u;
static float urand() {  // [0, 1)
  g_rng = g_rng * 747796405u + 2891336453u;
  uint32_t w = ((g_rng >> ((g_rng >> 28u) + 4u)) ^ g_rng) * 277803737u;
  w = (w >> 22u) ^ w;
  return (float)(w >> 8) * (1.0f / 16777216.0f);
}
static float safe_inv(float d) {  // pt_device.h
  const float eps = 1e-20f;
  float a = std::fabs(d) < eps ? (d < 0.0f ? -eps : eps) : d;
  return 1.0f / a;
}
static float qbyte(uint32_t w, int j) { return (float)((w >> (8 * j)) & 0xffu); }

int main(int argc, char** argv) {
  if (argc < 6) { fprintf(stderr, "usage: node64_check tris.bin leaf fan depth rays\n"); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<float> raw;
  float buf[9 * 256];
  size_t n;
  while ((n = fread(buf, sizeof(float), 9 * 256, fp)) > 0) raw.insert(raw.end(), buf, buf + n);
  fclose(fp);
  const int leaf = atoi(argv[2]), fan = atoi(argv[3]), rays = atoi(argv[5]);
  const uint32_t depth = (uint32_t)atoi(argv[4]);
  std::vector<BuildTri> tris(raw.size() / 9);
  float blo[3] = {1e30f, 1e30f, 1e30f}, bhi[3] = {-1e30f, -1e30f, -1e30f};
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
  build_bvh(tris, leaf, depth, bvh);
  std::vector<float> n4;
  uint32_t num4 = 0, need = 0, dep4 = 0;
  collapse_bvh4(bvh.nodes, n4, num4, need, dep4, fan);
  std::vector<uint32_t> n64;
  if (!quantize_bvh4(n4.data(), num4, n64)) { printf("node64_check: conversion refused\n"); return 1; }
  if (n64.size() != (size_t)num4 * PTGS_NODE64_DWORDS) { printf("node64_check: bad size\n"); return 1; }

  unsigned long long viol = 0, children = 0, empty = 0, nrays = 0;
  for (uint32_t i = 0; i < num4; ++i) {
    const float* f = &n4[32 * (size_t)i];
    const uint32_t* o = &n64[PTGS_NODE64_DWORDS * (size_t)i];
    float org[3], step[3];
    std::memcpy(org, o, 12);
    std::memcpy(step, o + 3, 12);
    if (std::memcmp(o + 12, f + 24, 16) != 0) ++viol;  // links
    bool is_empty[4];
    for (int j = 0; j < 4; ++j) {
      uint32_t link;
      std::memcpy(&link, &f[24 + j], 4);
      is_empty[j] = f[j] >= 1e29f;
      if (is_empty[j]) {
        ++empty;
        if (j < 2 || link != 0u) ++viol;  // (the kernel's link compare covers slots 2 and 3)
        for (int a = 0; a < 3; ++a)
          if (qbyte(o[6 + 2 * a], j) != 255.0f || qbyte(o[7 + 2 * a], j) != 0.0f) ++viol;
        continue;
      }
      ++children;
      for (int a = 0; a < 3; ++a) {  // the unit ray: the decoded planes themselves
        int e = 0;
        if (std::frexp(step[a], &e) != 0.5f) ++viol;  // a power of two
        const float dlo = std::fmaf(qbyte(o[6 + 2 * a], j), step[a], org[a]);
        const float dhi = std::fmaf(qbyte(o[7 + 2 * a], j), step[a], org[a]);
        if (!(dlo <= f[(2 * a) * 4 + j]) || !(dhi >= f[(2 * a + 1) * 4 + j])) ++viol;
      }
    }
    for (int k = 0; k < rays; ++k) {
      ++nrays;
      float ro[3], inv[3], oinv[3];
      const int mode = k % 4;  // 0, 1: general; 2: one axis-parallel component; 3: origin outside the bounds
      for (int a = 0; a < 3; ++a) {
        const float ext = bhi[a] - blo[a];
        const float u = mode == 3 ? (urand() * 3.0f - 1.0f) : urand();
        ro[a] = blo[a] + u * ext;
        float d = urand() * 2.0f - 1.0f;
        if (mode == 2 && a == k / 4 % 3) d = (k & 8) ? 0.0f : -0.0f;
        inv[a] = safe_inv(d);
        oinv[a] = ro[a] * inv[a];
      }
      const float tmin = 0.001f, tcap = 10000.0f;
      for (int j = 0; j < 4; ++j) {
        float tn = tmin, tf = tcap;
        for (int a = 0; a < 3; ++a) {
          const bool neg = inv[a] < 0.0f;
          const float s = step[a] * inv[a], c = std::fmaf(org[a], inv[a], -oinv[a]);
          const uint32_t wn = o[6 + 2 * a + (neg ? 1 : 0)], wf = o[6 + 2 * a + (neg ? 0 : 1)];
          const float qn = std::fmaf(qbyte(wn, j), s, c), qf = std::fmaf(qbyte(wf, j), s, c);
          tn = std::fmax(tn, qn);
          tf = std::fmin(tf, qf);
          if (is_empty[j]) continue;
          const float cn = std::fmaf(f[(2 * a + (neg ? 1 : 0)) * 4 + j], inv[a], -oinv[a]);
          const float cf = std::fmaf(f[(2 * a + (neg ? 0 : 1)) * 4 + j], inv[a], -oinv[a]);
          if (!(qn <= cn) || !(qf >= cf)) ++viol;
        }
        if (is_empty[j]) {
          uint32_t link;
          std::memcpy(&link, &o[12 + j], 4);
          const bool hit = (tn <= tf * 1.0000004f) && (j < 2 || link != 0u);
          if (hit) ++viol;
        }
      }
    }
  }
  printf("node64_check nodes %u children %llu empty %llu rays %llu violations %llu\n", num4, children, empty, nrays, viol);
  return viol ? 1 : 0;
}
