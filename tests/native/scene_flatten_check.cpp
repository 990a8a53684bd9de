// scene_flatten_check — stand-alone host check of the scene upload's argument checks and triangle
// flattening (csrc/scene_flatten.h). Every array of a description is a heap allocation of exactly its count,
// so a check that reads an array before the check that should have rejected the description is an
// AddressSanitizer report. A valid description (two meshes with triangles, one of a transparent material,
// and one mesh of fewer than 3 indices) must flatten to values written out here by hand; one malformed
// description per rejection must give the code and the message of ptgs_scene_upload.
// Prints "scene_flatten_check cases N violations V". Exit status 1 when V > 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scene_flatten.h"

using namespace ptgs;

static unsigned long long g_viol = 0, g_cases = 0;
#define CHECK(cond)                                \
  do {                                             \
    if (!(cond)) {                                 \
      ++g_viol;                                    \
      printf("  line %d: %s\n", __LINE__, #cond);  \
    }                                              \
  } while (0)

// A description that owns its arrays; desc() points at exact-size copies (a count of 0 gives a 0-length
// allocation, which no read may touch).
struct Scene {
  std::vector<ptgs_vertex> vertices;
  std::vector<uint32_t> indices, mesh_index_count;
  std::vector<ptgs_mesh_info> meshes;
  std::vector<ptgs_material> materials;
  std::vector<ptgs_light_triangle> light_triangles;
  std::vector<ptgs_light_cdf> light_cdf;
  std::vector<ptgs_punctual_light> punctual_lights;
  std::vector<ptgs_punctual_cdf> punctual_cdf;
  std::vector<float> blue_noise;
  uint32_t blue_noise_size = 2;
  std::vector<ptgs_texture> textures;
};

template <class T>
static const T* exact(const std::vector<T>& v, std::vector<void*>& held) {
  T* p = (T*)::operator new(v.size() * sizeof(T));
  if (!v.empty()) std::memcpy((void*)p, v.data(), v.size() * sizeof(T));
  held.push_back(p);
  return p;
}

struct Desc {
  ptgs_scene_desc d{};
  std::vector<void*> held;
  explicit Desc(const Scene& s) {
    d.vertices = exact(s.vertices, held);
    d.num_vertices = (uint32_t)s.vertices.size();
    d.indices = exact(s.indices, held);
    d.num_indices = (uint32_t)s.indices.size();
    d.meshes = exact(s.meshes, held);
    d.mesh_index_count = exact(s.mesh_index_count, held);
    d.num_meshes = (uint32_t)s.meshes.size();
    d.materials = exact(s.materials, held);
    d.num_materials = (uint32_t)s.materials.size();
    d.light_triangles = exact(s.light_triangles, held);
    d.num_light_triangles = (uint32_t)s.light_triangles.size();
    d.light_cdf = exact(s.light_cdf, held);
    d.num_light_cdf = (uint32_t)s.light_cdf.size();
    d.punctual_lights = exact(s.punctual_lights, held);
    d.num_punctual_lights = (uint32_t)s.punctual_lights.size();
    d.punctual_cdf = exact(s.punctual_cdf, held);
    d.num_punctual_cdf = (uint32_t)s.punctual_cdf.size();
    d.blue_noise_rgba32f = exact(s.blue_noise, held);
    d.blue_noise_size = s.blue_noise_size;
    d.textures = exact(s.textures, held);
    d.num_textures = (uint32_t)s.textures.size();
  }
  Desc(const Desc&) = delete;
  ~Desc() {
    for (void* p : held) ::operator delete(p);
  }
};

// vertex i sits at (i, 10 + i, 20 + i)
static Scene valid_scene() {
  Scene s;
  s.vertices.resize(7);
  for (int i = 0; i < 7; ++i) {
    std::memset(&s.vertices[i], 0, sizeof(ptgs_vertex));
    s.vertices[i].pos[0] = (float)i;
    s.vertices[i].pos[1] = 10.0f + (float)i;
    s.vertices[i].pos[2] = 20.0f + (float)i;
  }
  //           mesh 0 (6 indices)  mesh 1 (2)  mesh 2 (4: one triangle, vertex offset 3)
  s.indices = {0, 1, 2, 2, 1, 3,   9, 9,       0, 1, 3, 2};
  s.meshes = {{0, 0, 0, 0}, {99, 0, 6, 0}, {1, 3, 8, 0}};  // (mesh 1 is skipped before its material is looked at)
  s.mesh_index_count = {6, 2, 4};
  s.materials.resize(2);
  std::memset(s.materials.data(), 0, 2 * sizeof(ptgs_material));
  s.materials[1].pad = 1.0f;  // transparent
  s.light_triangles = {{0, 1, 2, 0}, {4, 5, 6, 1}};
  s.light_cdf = {{0.5f, 0, {0, 0}}, {1.0f, 1, {0, 0}}};
  s.punctual_lights.resize(2);
  std::memset(s.punctual_lights.data(), 0, 2 * sizeof(ptgs_punctual_light));
  s.punctual_cdf = {{0.5f, 0, {0, 0}}, {1.0f, 1, {0, 0}}};
  s.blue_noise.assign(2 * 2 * 4, 0.25f);
  return s;
}

// both stages, as ptgs_scene_upload runs them (the texture pool is built between them)
static int run(const ptgs_scene_desc& d, FlatScene& flat, std::string& msg) {
  msg.clear();
  int rc = validate_scene_desc(&d, msg);
  if (rc == PTGS_OK) rc = flatten_scene(&d, flat, msg);
  return rc;
}

static void check_valid() {
  ++g_cases;
  const Scene s = valid_scene();
  Desc desc(s);
  FlatScene f;
  std::string msg;
  CHECK(run(desc.d, f, msg) == PTGS_OK && msg.empty());
  CHECK(f.has_transparent);
  const uint32_t hitrec[12] = {0, 1, 2, 0, 2, 1, 3, 0, 3, 4, 6, 1};
  CHECK(f.hitrec.size() == 12u && std::memcmp(f.hitrec.data(), hitrec, sizeof(hitrec)) == 0);
  struct { int v[3]; uint32_t mesh, prim, flags; } want[3] = {{{0, 1, 2}, 0, 0, 0}, {{2, 1, 3}, 0, 1, 0}, {{3, 4, 6}, 2, 0, 1}};
  CHECK(f.tris.size() == 3u);
  for (size_t i = 0; i < f.tris.size() && i < 3; ++i) {
    const BuildTri& t = f.tris[i];
    const float* v[3] = {t.v0, t.v1, t.v2};
    for (int k = 0; k < 3; ++k) {
      const float x = (float)want[i].v[k];
      CHECK(v[k][0] == x && v[k][1] == 10.0f + x && v[k][2] == 20.0f + x);
    }
    CHECK(t.mesh == want[i].mesh && t.prim == want[i].prim && t.gid == (uint32_t)i && t.flags == want[i].flags);
  }
  // without the transparent mesh
  ++g_cases;
  Scene o = s;
  o.meshes.pop_back();
  o.mesh_index_count.pop_back();
  Desc od(o);
  CHECK(run(od.d, f, msg) == PTGS_OK && !f.has_transparent && f.tris.size() == 2u && f.hitrec.size() == 8u);
}

template <class Edit>
static void reject(int code, const char* want, Edit edit) {
  ++g_cases;
  Scene s = valid_scene();
  edit(s);
  Desc desc(s);
  FlatScene f;
  std::string msg;
  const int rc = run(desc.d, f, msg);
  if (rc != code || msg != want) {
    ++g_viol;
    printf("  want %d \"%s\"\n  got  %d \"%s\"\n", code, want, rc, msg.c_str());
  }
}

// a null array with a non-zero count (the arrays the description may leave out when the count is zero)
template <class Null>
static void reject_null(const char* want, Null null) {
  ++g_cases;
  Desc desc(valid_scene());
  null(desc.d);
  FlatScene f;
  std::string msg;
  const int rc = run(desc.d, f, msg);
  if (rc != PTGS_EINVAL || msg != want) {
    ++g_viol;
    printf("  want %d \"%s\"\n  got  %d \"%s\"\n", PTGS_EINVAL, want, rc, msg.c_str());
  }
}

static const char* kLight = "light triangle / CDF buffers must hold >= 1 entry (engine.cpp:1766-1769 dummy)";
static const char* kPunctual = "punctual light / CDF buffers must hold >= 1 entry (engine.cpp:1795-1797 dummy)";
static const char* kNoise = "blue noise must be a power-of-two square RGBA32F texture";

static void check_rejections() {
  reject_null("vertices is null", [](ptgs_scene_desc& d) { d.vertices = nullptr; });
  reject_null("indices is null", [](ptgs_scene_desc& d) { d.indices = nullptr; });
  reject_null("meshes is null", [](ptgs_scene_desc& d) { d.meshes = nullptr; });
  reject_null("meshes is null", [](ptgs_scene_desc& d) { d.mesh_index_count = nullptr; });
  reject_null("at least one material is required", [](ptgs_scene_desc& d) { d.materials = nullptr; });
  reject_null(kLight, [](ptgs_scene_desc& d) { d.light_triangles = nullptr; });
  reject_null(kLight, [](ptgs_scene_desc& d) { d.light_cdf = nullptr; });
  reject_null(kPunctual, [](ptgs_scene_desc& d) { d.punctual_lights = nullptr; });
  reject_null(kPunctual, [](ptgs_scene_desc& d) { d.punctual_cdf = nullptr; });
  reject_null(kNoise, [](ptgs_scene_desc& d) { d.blue_noise_rgba32f = nullptr; });
  reject_null("textures is null", [](ptgs_scene_desc& d) { d.textures = nullptr; d.num_textures = 1; });

  reject(PTGS_EINVAL, "at least one material is required", [](Scene& s) { s.materials.clear(); });
  reject(PTGS_EINVAL, kLight, [](Scene& s) { s.light_triangles.clear(); });
  reject(PTGS_EINVAL, kLight, [](Scene& s) { s.light_cdf.clear(); });
  reject(PTGS_EINVAL, kPunctual, [](Scene& s) { s.punctual_lights.clear(); });
  reject(PTGS_EINVAL, kPunctual, [](Scene& s) { s.punctual_cdf.clear(); });
  reject(PTGS_EINVAL, kNoise, [](Scene& s) { s.blue_noise_size = 0; s.blue_noise.clear(); });
  reject(PTGS_EINVAL, kNoise, [](Scene& s) { s.blue_noise_size = 3; s.blue_noise.assign(3 * 3 * 4, 0.0f); });

  reject(PTGS_EINVAL, "mesh 0: material 2 out of range", [](Scene& s) { s.meshes[0].material_index = 2; });
  reject(PTGS_EINVAL, "mesh 2: index range out of bounds", [](Scene& s) { s.mesh_index_count[2] = 5; });
  reject(PTGS_EINVAL, "mesh 2: index range out of bounds", [](Scene& s) { s.meshes[2].index_offset = 0xfffffffeu; });
  reject(PTGS_EINVAL, "mesh 0 prim 1: vertex 7 out of range", [](Scene& s) { s.indices[5] = 7; });
  reject(PTGS_EINVAL, "mesh 2 prim 0: vertex 7 out of range", [](Scene& s) { s.meshes[2].vertex_offset = 4; });
  reject(PTGS_EINVAL, "punctual CDF shorter than the light list (binary search runs over the light count)",
         [](Scene& s) { s.punctual_cdf.pop_back(); });
  reject(PTGS_EINVAL, "light CDF entry 1: triangle 2 out of range", [](Scene& s) { s.light_cdf[1].triangle_index = 2; });
  reject(PTGS_EINVAL, "light triangle 1 references a vertex out of range", [](Scene& s) { s.light_triangles[1].v2 = 7; });
  reject(PTGS_EINVAL, "light triangle 0 references a vertex out of range", [](Scene& s) { s.light_triangles[0].v0 = 7; });

  // several faults: the first in the upload's order is reported
  reject(PTGS_EINVAL, "mesh 2: material 2 out of range", [](Scene& s) {
    s.meshes[2].material_index = 2;
    s.punctual_cdf.pop_back();
    s.light_cdf[0].triangle_index = 9;
  });
  reject(PTGS_EINVAL, "punctual CDF shorter than the light list (binary search runs over the light count)", [](Scene& s) {
    s.punctual_cdf.pop_back();
    s.light_cdf[0].triangle_index = 9;
    s.light_triangles[0].v0 = 7;
  });
  reject(PTGS_EINVAL, "light CDF entry 0: triangle 9 out of range", [](Scene& s) {
    s.light_cdf[0].triangle_index = 9;
    s.light_triangles[0].v0 = 7;
  });
  reject(PTGS_EINVAL, kLight, [](Scene& s) { s.light_cdf.clear(); s.blue_noise_size = 3; s.meshes[0].material_index = 2; });
}

// a scene without geometry: the single all-zero light triangle is the reference's dummy and passes; a second
// one, or a dummy that is not all zero, is a light triangle out of range
static void check_dummy_light() {
  auto empty = [] {
    Scene s = valid_scene();
    s.vertices.clear();
    s.indices.clear();
    s.meshes.clear();
    s.mesh_index_count.clear();
    s.light_triangles = {{0, 0, 0, 0}};
    s.light_cdf = {{1.0f, 0, {0, 0}}};
    return s;
  };
  {
    ++g_cases;
    Desc desc(empty());
    FlatScene f;
    std::string msg;
    CHECK(run(desc.d, f, msg) == PTGS_OK && f.tris.empty() && f.hitrec.empty() && !f.has_transparent);
    desc.d.vertices = nullptr;  // (with their counts at zero the arrays may be null)
    desc.d.indices = nullptr;
    desc.d.meshes = nullptr;
    desc.d.mesh_index_count = nullptr;
    desc.d.textures = nullptr;
    ++g_cases;
    CHECK(run(desc.d, f, msg) == PTGS_OK && f.tris.empty());
  }
  for (int variant = 0; variant < 2; ++variant) {
    ++g_cases;
    Scene s = empty();
    if (variant == 0) s.light_triangles.push_back({0, 0, 0, 0});
    else s.light_triangles[0].v1 = 1;
    Desc desc(s);
    FlatScene f;
    std::string msg;
    CHECK(run(desc.d, f, msg) == PTGS_EINVAL && msg == "light triangle 0 references a vertex out of range");
  }
}

int main() {
  check_valid();
  check_rejections();
  check_dummy_light();
  printf("scene_flatten_check cases %llu violations %llu\n", g_cases, g_viol);
  return g_viol ? 1 : 0;
}
