// canonical_tree_dump — the canonical 4-wide tree of the host build, for tests that model a walk on the CPU.
//
//   canonical_tree_dump <tris.bin> <leaf> <fan> <depth> <nodes.bin> <records.bin>
//
// tris.bin holds float32 triangles (9 floats each, at least two). The program builds what the scene upload's host
// path builds for one (leaf, fan, depth budget) try (api.cpp HostSahBuilder: build_bvh, then collapse_bvh4) and
// writes the 4-wide nodes (32 floats each: the layout ptgs_scene_get_bvh exposes) and the triangle records in
// leaf order (12 floats each). Prints one line of "name value" pairs: nodes, need (collapse_bvh4's worst-case
// stack need), depth4, bvh2_depth. Host code only (bvh.cpp); its own main.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "bvh.h"

using namespace ptgs;

static bool write_all(const char* path, const std::vector<float>& v) {
  FILE* fp = fopen(path, "wb");
  if (!fp) { perror(path); return false; }
  const bool ok = v.empty() || fwrite(v.data(), sizeof(float), v.size(), fp) == v.size();
  return fclose(fp) == 0 && ok;
}

int main(int argc, char** argv) {
  if (argc < 7) {
    fprintf(stderr, "usage: canonical_tree_dump <tris.bin> <leaf> <fan> <depth> <nodes.bin> <records.bin>\n");
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
    fprintf(stderr, "canonical_tree_dump: no BVH2 node (fewer than two leaves)\n");
    return 2;
  }
  std::vector<float> n4;
  uint32_t num4 = 0, need = 0, depth4 = 0;
  collapse_bvh4(bvh.nodes, n4, num4, need, depth4, fan);
  if (n4.size() != (size_t)num4 * 32 || bvh.tris.size() != tris.size() * 12) {
    fprintf(stderr, "canonical_tree_dump: unexpected sizes\n");
    return 1;
  }
  if (!write_all(argv[5], n4) || !write_all(argv[6], bvh.tris)) return 1;
  printf("canonical_tree_dump: nodes %u need %u depth4 %u bvh2_depth %u\n", num4, need, depth4, bvh.depth);
  return 0;
}
