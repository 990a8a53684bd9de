// scene_flatten.h — the scene upload's argument checks and triangle flattening (api.cpp ptgs_scene_upload):
// pure host code over a ptgs_scene_desc, which guards every host read of the description's arrays against
// an out-of-range count or index. No HIP include: tests/native/scene_flatten_check.cpp builds it with a
// host compiler alone. Both functions return PTGS_OK, or a PTGS_* code with the message for ptgs_last_error.
#pragma once

#include <stdint.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptgs/ptgs.h"
#include "bvh.h"

namespace ptgs {

inline int scene_reject(std::string& msg, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  msg = buf;
  return code;
}

// The description's arrays are there and the counts that must not be zero are not.
inline int validate_scene_desc(const ptgs_scene_desc* d, std::string& msg) {
  if (!d->vertices && d->num_vertices) return scene_reject(msg, PTGS_EINVAL, "vertices is null");
  if (!d->indices && d->num_indices) return scene_reject(msg, PTGS_EINVAL, "indices is null");
  if (d->num_meshes && (!d->meshes || !d->mesh_index_count)) return scene_reject(msg, PTGS_EINVAL, "meshes is null");
  if (!d->materials || d->num_materials == 0) return scene_reject(msg, PTGS_EINVAL, "at least one material is required");
  if (!d->light_triangles || !d->light_cdf || d->num_light_cdf == 0 || d->num_light_triangles == 0)
    return scene_reject(msg, PTGS_EINVAL, "light triangle / CDF buffers must hold >= 1 entry (engine.cpp:1766-1769 dummy)");
  if (!d->punctual_lights || !d->punctual_cdf || d->num_punctual_lights == 0 || d->num_punctual_cdf == 0)
    return scene_reject(msg, PTGS_EINVAL, "punctual light / CDF buffers must hold >= 1 entry (engine.cpp:1795-1797 dummy)");
  const uint32_t bn = d->blue_noise_size;
  if (!d->blue_noise_rgba32f || bn == 0 || (bn & (bn - 1)) != 0)
    return scene_reject(msg, PTGS_EINVAL, "blue noise must be a power-of-two square RGBA32F texture");
  if (d->num_textures && !d->textures) return scene_reject(msg, PTGS_EINVAL, "textures is null");
  return PTGS_OK;
}

struct FlatScene {
  std::vector<BuildTri> tris;    // in flattening order (gid)
  std::vector<uint32_t> hitrec;  // per gid: global vertex indices + material (closest_hit's one fetch)
  bool has_transparent = false;
};

// Gathers the triangles of a description that passed validate_scene_desc, skipping meshes with < 3 indices
// (engine.cpp:545-547), then checks the light CDFs and light triangles against the counts.
inline int flatten_scene(const ptgs_scene_desc* d, FlatScene& out, std::string& msg) {
  out = FlatScene{};
  for (uint32_t m = 0; m < d->num_meshes; ++m) {
    const ptgs_mesh_info& mi = d->meshes[m];
    uint32_t cnt = d->mesh_index_count[m];
    if (cnt < 3) continue;
    if (mi.material_index >= d->num_materials)
      return scene_reject(msg, PTGS_EINVAL, "mesh %u: material %u out of range", m, mi.material_index);
    if ((uint64_t)mi.index_offset + cnt > d->num_indices)
      return scene_reject(msg, PTGS_EINVAL, "mesh %u: index range out of bounds", m);
    const ptgs_material& mat = d->materials[mi.material_index];
    uint32_t flags = (mat.pad > 0.5f) ? 1u : 0u;  // non-opaque geometry (engine.cpp:562-567)
    out.has_transparent |= flags != 0;
    for (uint32_t p = 0; p < cnt / 3; ++p) {
      BuildTri t;
      for (int k = 0; k < 3; ++k) {
        uint32_t vi = d->indices[mi.index_offset + 3 * p + k] + mi.vertex_offset;
        if (vi >= d->num_vertices)
          return scene_reject(msg, PTGS_EINVAL, "mesh %u prim %u: vertex %u out of range", m, p, vi);
        float* dst = k == 0 ? t.v0 : (k == 1 ? t.v1 : t.v2);
        std::memcpy(dst, d->vertices[vi].pos, 12);
        out.hitrec.push_back(vi);
      }
      out.hitrec.push_back(mi.material_index);
      t.mesh = m; t.prim = p; t.gid = (uint32_t)out.tris.size(); t.flags = flags;
      out.tris.push_back(t);
    }
  }
  if (out.tris.size() >= (1u << 27)) return scene_reject(msg, PTGS_ERANGE, "too many triangles (%zu)", out.tris.size());
  if (d->num_punctual_cdf < d->num_punctual_lights)
    return scene_reject(msg, PTGS_EINVAL,
                        "punctual CDF shorter than the light list (binary search runs over the light count)");
  for (uint32_t i = 0; i < d->num_light_cdf; ++i)
    if (d->light_cdf[i].triangle_index >= d->num_light_triangles)
      return scene_reject(msg, PTGS_EINVAL, "light CDF entry %u: triangle %u out of range", i,
                          d->light_cdf[i].triangle_index);
  for (uint32_t i = 0; i < d->num_light_triangles; ++i) {
    const ptgs_light_triangle& lt = d->light_triangles[i];
    if (d->num_vertices == 0 || lt.v0 >= d->num_vertices || lt.v1 >= d->num_vertices || lt.v2 >= d->num_vertices) {
      if (d->num_light_triangles == 1 && lt.v0 == 0 && lt.v1 == 0 && lt.v2 == 0) continue;  // dummy
      return scene_reject(msg, PTGS_EINVAL, "light triangle %u references a vertex out of range", i);
    }
  }
  return PTGS_OK;
}

}  // namespace ptgs
