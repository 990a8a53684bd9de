// api.cpp — the C-ABI boundary (include/ptgs/ptgs.h): context, scene upload, trace dispatch.
//
// Replaces, on the reference side (Vulkan_Engine/engine.cpp):
//   createGlobalBindlessBuffers uploads :1658-1860 and buildBlas/initStaticTlas :534-655, :1385-1520
//       -> ptgs_scene_upload (host BVH build + hipMemcpy of the reference-layout arrays)
//   recordCommandBuffer's vkCmdTraceRaysKHR :1971-1976 + rt_output_image running mean
//       -> ptgs_trace_camera
//   torus trace :1893-1900 / :2787-2794 -> ptgs_trace_torus
//
// Map: struct ptgs_ctx; the helpers every entry point shares (fail, HIPCHK, hip_rc, the argument checks);
// the scene upload's builders and stages; context, communicator, trace and memory entry points; then the
// rasterizers: the splat frame calls (splat_check_args, splat_render, splat_overlap_resources / _begin,
// splat_finish over the context's SplatFrames: splat_frames.h owns, splat_run.h decides), the Gaussian
// preparation, backward, densify and loss entry points, the splat's status / reserve / accessors, points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptgs/ptgs.h"
#include "bvh.h"
#include "bvh_gpu.h"
#include "bvh_opt.h"
#include "bvh_tries.h"
#include "knn.h"
#include "hostmath.h"
#include "pt_launch.h"
#include "pt_wavefront.h"
#include "scene_flatten.h"
#include "comm.h"
#include "dev_buf.h"
#include "splat.h"
#include "splat_adam.h"
#include "splat_adam_math.h"
#include "splat_backward.h"
#include "splat_densify.h"
#include "splat_frames.h"
#include "splat_loss.h"
#include "splat_sh.h"
#include "splat_train.h"
#include "textures.h"

using namespace ptgs;

static_assert(kSplatReportIncomplete == SPLAT_REPORT_INCOMPLETE && kSplatReportBadIds == SPLAT_REPORT_BAD_IDS,
              "splat_run.h names the bits of SplatReport");

struct ptgs_ctx {
  int device = 0;
  std::string err;
  uint32_t flags = 0;
  bool has_scene = false;
  DevScene dsc{};
  std::vector<void*> scene_allocs;
  ptgs_scene_info info{};
  ptgs_scene_build build{};  // which builder's tree is resident (ptgs_scene_get_build)
  ptgs_scene_tree_opt tree_opt{};  // the megakernel's traversal copy of it (ptgs_scene_get_tree_opt)
  uint32_t pt_walked_need = 0;     // that copy's stack need, optimised or not (ptgs_scene_get_pt_stack)
  unsigned long long* counters = nullptr;  // 8 x u64
  SplatFrames frames;  // the splat frame calls' workspaces, streams, events, run and pending reports
  DensifyWorkspace* densify = nullptr;  // the densification plan (ptgs_gaussians_densify_plan / _apply)
  LossWorkspace* loss = nullptr;  // the partial maps and sums of ptgs_image_loss_l1_dssim
  ptgs::DevBuf sh_eye_partials;  // per-workgroup partial sums of ptgs_gaussians_sh_colors_backward_eye
  ptgs::DevBuf mse_partials;  // per-workgroup sums of ptgs_image_mse: a fixed TRAIN_MSE_MAX_WG doubles, from ptgs_create
  ptgs::WfWorkspace wf;  // wavefront path tracer buffers (PTGS_FLAG_PT_WAVEFRONT)
  ptgs::PtSched pt_sched;  // megakernel tile schedule (heavy tiles first)
  void* comm = nullptr;  // RCCL communicator (ptgs_comm_create)
  int comm_ranks = 0, comm_rank = 0;
};

namespace {

int fail(ptgs_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  if (c) c->err = buf;
  return code;
}

#define HIPCHK(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) return fail(ctx, PTGS_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

int hip_rc(ptgs_ctx* c, hipError_t e, const char* what) {
  if (e != hipSuccess) return fail(c, PTGS_EHIP, "%s: %s", what, hipGetErrorString(e));
  return PTGS_OK;
}

int check_image_size(ptgs_ctx* c, uint32_t w, uint32_t h) {
  if (w == 0 || h == 0 || w > 32768 || h > 32768) return fail(c, PTGS_EINVAL, "bad image size %ux%u", w, h);
  return PTGS_OK;
}

// row_ranges: [begin, end) per rank of the communicator, inside the image
int check_row_ranges(ptgs_ctx* c, const uint32_t* row_ranges, uint32_t height) {
  for (int g = 0; g < c->comm_ranks; ++g)
    if (row_ranges[2 * g] > row_ranges[2 * g + 1] || row_ranges[2 * g + 1] > height)
      return fail(c, PTGS_EINVAL, "bad row range of rank %d", g);
  return PTGS_OK;
}

void free_scene(ptgs_ctx* c) {
  for (void* p : c->scene_allocs) (void)hipFree(p);
  c->scene_allocs.clear();
  c->has_scene = false;
  c->dsc = DevScene{};
}

template <typename T>
int upload(ptgs_ctx* c, const T* src, size_t count, const T** dst) {
  if (count == 0) { *dst = nullptr; return PTGS_OK; }
  void* p = nullptr;
  HIPCHK(c, hipMalloc(&p, count * sizeof(T)));
  c->scene_allocs.push_back(p);
  HIPCHK(c, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
  c->info.device_bytes += count * sizeof(T);
  *dst = (const T*)p;
  return PTGS_OK;
}

bool is_device_ptr(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged || a.devicePointer != nullptr;
}

int fill_cam(ptgs_ctx* c, const ptgs_ubo* ubo, CamParams& cp) {
  if (!inverse4(ubo->view, cp.inv_view)) return fail(c, PTGS_EINVAL, "ubo.view is singular");
  if (!inverse4(ubo->proj, cp.inv_proj)) return fail(c, PTGS_EINVAL, "ubo.proj is singular");
  for (int k = 0; k < 4; ++k) cp.ambient[k] = ubo->ambient_light[k];
  cp.emissive_flux = ubo->emissive_flux;
  cp.punctual_flux = ubo->punctual_flux;
  cp.p_emissive = ubo->p_emissive;
  cp.fov = ubo->fov;
  cp.win_height = ubo->height;
  cp.use_lod = ubo->use_lod;
  cp.lod_factor = ubo->lod_factor;
  return PTGS_OK;
}

// ---- scene upload: the three BVH builders, run under run_bvh_tries (bvh_tries.h), and the stages ----

void bvh_log(const char* how, const BvhTry& t, uint32_t depth, uint32_t need) {
  if (getenv("PTGS_BVH_LOG"))
    fprintf(stderr, "[ptgs] %s tree: leaf %d fan %d depth budget %u -> depth %u, stack need %u%s\n", how, t.leaf, t.fan,
            t.depth, depth, need, need >= PTGS_STACK ? (need < PTGS_STACK_TOTAL ? " (DEEP)" : " (does not fit)") : "");
}

double ms_between(std::chrono::steady_clock::time_point t0, std::chrono::steady_clock::time_point t1) {
  return std::chrono::duration<double, std::milli>(t1 - t0).count();
}

// bytes of a triangle on the device: its record (3 float4, bvh.h) and its flag word
constexpr size_t kTriDeviceBytes = 3 * sizeof(float4) + sizeof(uint32_t);

// The host binned-SAH build (bvh.cpp). A BVH2 as deep as the LDS stack ends the tries: a 2-wide "collapse"
// needs the BVH2's depth, so no fan-out would fit it.
struct HostSahBuilder {
  const std::vector<BuildTri>& tris;
  BvhOut bvh;             // the latest BVH2; its tris / tri_flags are the records of every collapse of it
  std::vector<float> n4;  // the latest collapse
  uint32_t num4 = 0;
  BvhStep build(int leaf, uint32_t depth, uint32_t stack_lds) {
    build_bvh(tris, leaf, depth, bvh);
    return bvh.depth >= stack_lds ? BvhStep::TooDeep : BvhStep::Ok;
  }
  BvhStep collapse(int fan, uint32_t& need, uint32_t& depth4) {
    need = 0;
    collapse_bvh4(bvh.nodes, n4, num4, need, depth4, fan);
    return BvhStep::Ok;
  }
};

// What a GPU builder holds on the device: the latest BVH2 with its triangle records, and the latest
// collapse. All of it is freed with the builder unless hand_over() gave the tree to the scene; a build that
// returned hipErrorNotSupported with `g` filled (bvh_gpu.h) is freed the same way.
struct GpuTree {
  GpuBvh g;
  float4* n4 = nullptr;
  uint32_t num4 = 0;
  float ms = 0.0f;               // the builds' device time + the host-clock span of each collapse
  hipError_t err = hipSuccess;   // the latest step's
  GpuTree() = default;
  GpuTree(const GpuTree&) = delete;
  GpuTree& operator=(const GpuTree&) = delete;
  ~GpuTree() {
    release_bvh2();
    (void)hipFree(n4);
  }
  void release_bvh2() {
    (void)hipFree(g.nodes);
    (void)hipFree(g.tris);
    (void)hipFree(g.tri_flags);
    g = GpuBvh{};
  }
  BvhStep step(hipError_t e) {
    err = e;
    return e == hipSuccess ? BvhStep::Ok : e == hipErrorNotSupported ? BvhStep::NotSupported : BvhStep::Error;
  }
  BvhStep collapse(int fan, uint32_t& need, uint32_t& depth4) {
    const auto t0 = std::chrono::steady_clock::now();
    (void)hipFree(n4);
    n4 = nullptr;
    const hipError_t e = collapse_bvh4_gpu(g.nodes, g.num_nodes, fan, &n4, &num4, &need, &depth4);
    ms += (float)ms_between(t0, std::chrono::steady_clock::now());  // build_ms includes it
    return step(e);
  }
  // the collapsed nodes and the triangle records become the scene's; the BVH2's nodes are done with
  void hand_over(std::vector<void*>& allocs, DevScene& s) {
    (void)hipFree(g.nodes);
    for (void* p : {(void*)n4, (void*)g.tris, (void*)g.tri_flags}) allocs.push_back(p);
    s.nodes = n4;
    s.tris = g.tris;
    s.tri_flags = g.tri_flags;
    n4 = nullptr;
    g = GpuBvh{};
  }
};
// the GPU binned-SAH build (bvh_sah_gpu.hip): the host builder's trees
struct GpuSahBuilder : GpuTree {
  static constexpr uint32_t kId = PTGS_BUILDER_GPU_SAH;
  const std::vector<BuildTri>& tris;
  explicit GpuSahBuilder(const std::vector<BuildTri>& t) : tris(t) {}
  BvhStep build(int leaf, uint32_t depth, uint32_t) {
    release_bvh2();
    float bms = 0.0f;
    const hipError_t e = build_bvh_sah_gpu(tris, leaf, depth, g, &bms);
    ms += bms;
    return step(e);
  }
  uint32_t max_leaf() const { return g.max_leaf; }
};
// the GPU LBVH (bvh_gpu.hip): fixed leaves of up to 4 triangles, one build (lbvh_bvh_tries)
struct GpuLbvhBuilder : GpuTree {
  static constexpr uint32_t kId = PTGS_BUILDER_GPU_LBVH;
  const std::vector<BuildTri>& tris;
  explicit GpuLbvhBuilder(const std::vector<BuildTri>& t) : tris(t) {}
  BvhStep build(int, uint32_t depth, uint32_t) {
    release_bvh2();
    float bms = 0.0f;
    const hipError_t e = build_bvh_gpu(tris, depth, g, &bms);
    ms += bms;
    return step(e);
  }
  uint32_t max_leaf() const { return 4u; }
};

void publish_tree(ptgs_ctx* c, DevScene& s, uint32_t builder, const BvhTriesResult& r, uint32_t num4, uint32_t max_leaf,
                  double build_ms) {
  s.deep_stack = r.need >= PTGS_STACK ? 1 : 0;
  c->info.num_bvh_nodes = num4;
  c->info.bvh_depth = r.depth4;
  c->info.max_leaf_size = max_leaf;
  c->info.build_ms = build_ms;
  c->build = ptgs_scene_build{builder, (uint32_t)r.kept.leaf, (uint32_t)r.kept.fan, r.kept.depth, r.need,
                              (uint32_t)s.deep_stack};
}

// A tree of one of the GPU builders. *built stays false, with PTGS_OK, when the builder does not support the
// input or none of its trees fits the stack: the host builds then (whatever the builder held goes with it).
template <class Builder>
int build_tree_gpu(ptgs_ctx* c, const std::vector<BuildTri>& tris, const std::vector<BvhTry>& tries, DevScene& s,
                   bool* built) {
  Builder b(tris);
  const BvhTriesResult r =
      run_bvh_tries(b, tries, PTGS_STACK, PTGS_STACK_TOTAL,
                    [](const BvhTry& t, uint32_t depth4, uint32_t need) { bvh_log("GPU", t, depth4, need); });
  if (r.fit == BvhFit::Error) return fail(c, PTGS_EHIP, "GPU BVH build: %s", hipGetErrorString(b.err));
  if (r.fit != BvhFit::Fits) return PTGS_OK;
  publish_tree(c, s, Builder::kId, r, b.num4, b.max_leaf(), b.ms);
  c->info.device_bytes += (size_t)b.num4 * PTGS_NODE4_BYTES + tris.size() * kTriDeviceBytes;
  b.hand_over(c->scene_allocs, s);
  *built = true;
  return PTGS_OK;
}

// The host's tree; host_n4 gets its final 4-wide nodes (upload_traversal_nodes reads them).
int build_tree_host(ptgs_ctx* c, const std::vector<BuildTri>& tris, DevScene& s, std::vector<float>& host_n4) {
  const auto t0 = std::chrono::steady_clock::now();
  HostSahBuilder b{tris};
  const BvhTriesResult r =
      run_bvh_tries(b, parse_bvh_tries(getenv("PTGS_BVH_TRIES"), PTGS_STACK), PTGS_STACK, PTGS_STACK_TOTAL,
                    [](const BvhTry& t, uint32_t depth4, uint32_t need) { bvh_log("host", t, depth4, need); });
  const auto t1 = std::chrono::steady_clock::now();
  if (r.fit != BvhFit::Fits) return fail(c, PTGS_ERANGE, "BVH depth %u exceeds the traversal stack", b.bvh.depth);
  int rc;
  if ((rc = upload(c, (const float4*)b.n4.data(), b.n4.size() / 4, &s.nodes))) return rc;
  if ((rc = upload(c, (const float4*)b.bvh.tris.data(), b.bvh.tris.size() / 4, &s.tris))) return rc;
  if ((rc = upload(c, b.bvh.tri_flags.data(), b.bvh.tri_flags.size(), &s.tri_flags))) return rc;
  publish_tree(c, s, PTGS_BUILDER_HOST_SAH, r, b.num4, b.bvh.max_leaf, ms_between(t0, t1));
  host_n4.swap(b.n4);
  return PTGS_OK;
}

// The traversal reads 4-wide nodes through a buffer descriptor with 32-bit byte offsets (node << 7,
// num_records 0x7fffffff: pt_device.h box4): nodes past 2 GiB would read as zeros (no boxes, child
// link 0) without a fault. Such a tree (~16.7M nodes, some 50M triangles) is refused here.
int check_node_window(ptgs_ctx* c) {
  const uint32_t limit = bvh_node_limit(getenv("PTGS_BVH_NODE_LIMIT"));
  if (c->info.num_bvh_nodes > limit)
    return fail(c, PTGS_ERANGE, "BVH of %u 4-wide nodes exceeds the traversal's 2 GiB node window (%u nodes)",
                c->info.num_bvh_nodes, limit);
  return PTGS_OK;
}

// The megakernel's traversal reads a compact 64-B copy of the final nodes (bvh.h make_traversal_nodes; one
// conversion for the host SAH, GPU SAH and LBVH trees: a GPU-built tree is read back for it). Their links
// are re-encoded into the fewest bits this tree needs, so that a stack entry of the closest-hit walk
// carries the child's entry distance in the bits left (bvh.h stack_layout, stack_key.h).
// PTGS_PT_STACK_KEY_BITS forces the key's width (tests: 0 = never cull).
// The copy's topology is its own: the trees of the two SAH builders (the same canonical tree) are rebuilt by
// reinsertion for fewer node steps per ray (bvh_opt.h), held to the megakernel's own LDS stack (PTGS_PT_STACK) or,
// failing that, to LDS + overflow; the LBVH, whose point is rebuild time, is converted as it is.
// PTGS_PT_TREE_OPT=0 / 1 forces it off / on. The megakernel's instantiation follows the need of the copy it
// walks (pt_deep_stack), not the canonical need (deep_stack: the torus, depth and wavefront kernels). The
// canonical nodes, scene_info and scene_build describe the canonical tree either way.
int upload_traversal_nodes(ptgs_ctx* c, std::vector<float>& host_n4, DevScene& s) {
  const size_t nf = (size_t)c->info.num_bvh_nodes * 32;
  if (host_n4.size() != nf) {
    host_n4.resize(nf);
    HIPCHK(c, hipMemcpy(host_n4.data(), s.nodes, nf * sizeof(float), hipMemcpyDeviceToHost));
  }
  int force = -1;
  if (const char* e = getenv("PTGS_PT_STACK_KEY_BITS")) force = std::max(0, atoi(e));
  bool optimise = c->build.builder != PTGS_BUILDER_GPU_LBVH;
  if (const char* e = getenv("PTGS_PT_TREE_OPT")) optimise = atoi(e) != 0;
  std::vector<uint32_t> n64;
  StackLayout sl;
  TreeOptInfo oi;
  // the copy's need is held below the megakernel's own LDS stack (the budgeted collapse, bvh_opt.h); only a
  // tree whose reinserted BVH2 is too high for that is held to LDS + overflow and walked by the DEEP megakernel
  const uint32_t limits[2] = {PTGS_PT_STACK, PTGS_STACK_TOTAL};
  if (!make_opt_traversal_nodes(host_n4.data(), c->info.num_bvh_nodes, (int)c->build.fan, limits, 2, optimise, force,
                                n64, sl, oi))
    return fail(c, PTGS_ERANGE, "BVH node extents beyond the compact nodes' step range (2^-100 .. 2^100)");
  c->tree_opt = ptgs_scene_tree_opt{oi.applied, oi.num_nodes, oi.need, oi.depth, oi.fan, oi.passes,
                                    oi.area_before, oi.area_after, oi.ms};
  // the launch rule: the need of the copy that is walked (the canonical tree's when it was converted as it is)
  c->pt_walked_need = oi.applied ? oi.need : c->build.stack_need;
  s.pt_deep_stack = c->pt_walked_need >= PTGS_PT_STACK ? 1 : 0;
  s.stk_key_mask = sl.key_mask;
  s.leaf_shift = sl.leaf_shift;
  s.leaf_start_mask = sl.leaf_start_mask;
  if (getenv("PTGS_BVH_LOG")) {
    if (optimise)
      fprintf(stderr, "[ptgs] traversal tree: %s in %.1f ms (%u passes): nodes %u -> %u, stack need %u -> %u, depth %u -> %u, "
              "fan %u, area sum %.3f -> %.3f\n", oi.applied ? "optimised" : "not applied", oi.ms, oi.passes,
              c->info.num_bvh_nodes, oi.num_nodes, c->build.stack_need, oi.need, c->info.bvh_depth, oi.depth, oi.fan,
              oi.area_before, oi.area_after);
    fprintf(stderr, "[ptgs] megakernel: walked need %u, LDS stack %u%s\n", c->pt_walked_need, (uint32_t)PTGS_PT_STACK,
            s.pt_deep_stack ? " (DEEP)" : "");
    fprintf(stderr, "[ptgs] stack word:%u link bits, %u key bits (mask %08x), leaf shift %u\n", sl.ref_bits, sl.key_bits,
            sl.key_mask, sl.leaf_shift);
  }
  return upload(c, (const uint4*)n64.data(), n64.size() / 4, &s.nodes64);
}

// the description's arrays, the hit records and the texture pool
int upload_scene_arrays(ptgs_ctx* c, const ptgs_scene_desc* d, const FlatScene& flat, const TexturePool& texpool,
                        DevScene& s) {
  int rc;
  // a zero vertex/index count still needs valid (never dereferenced) pointers
  ptgs_vertex dummy_v{};
  uint32_t dummy_i = 0;
  ptgs_mesh_info dummy_m{};
  if ((rc = upload(c, d->num_vertices ? d->vertices : &dummy_v, d->num_vertices ? d->num_vertices : 1, &s.vertices))) return rc;
  if ((rc = upload(c, d->num_indices ? d->indices : &dummy_i, d->num_indices ? d->num_indices : 1, &s.indices))) return rc;
  if ((rc = upload(c, d->num_meshes ? d->meshes : &dummy_m, d->num_meshes ? d->num_meshes : 1, &s.meshes))) return rc;
  if ((rc = upload(c, d->materials, d->num_materials, &s.materials))) return rc;
  const std::vector<uint32_t>& hitrec = flat.hitrec;
  const uint32_t zero4[4] = {0, 0, 0, 0};
  if ((rc = upload(c, (const uint4*)(hitrec.empty() ? zero4 : hitrec.data()), hitrec.empty() ? 1 : hitrec.size() / 4,
                   &s.hitrec)))
    return rc;
  if ((rc = upload(c, d->light_triangles, d->num_light_triangles, &s.light_tris))) return rc;
  if ((rc = upload(c, d->light_cdf, d->num_light_cdf, &s.light_cdf))) return rc;
  if ((rc = upload(c, d->punctual_lights, d->num_punctual_lights, &s.plights))) return rc;
  if ((rc = upload(c, d->punctual_cdf, d->num_punctual_cdf, &s.pcdf))) return rc;
  const size_t bn = d->blue_noise_size;
  if ((rc = upload(c, (const float4*)d->blue_noise_rgba32f, bn * bn, &s.blue_noise))) return rc;
  if ((rc = upload(c, texpool.texels.data(), texpool.texels.size(), &s.tex.texels))) return rc;
  if ((rc = upload(c, texpool.info.data(), texpool.info.size(), &s.tex.info))) return rc;
  return upload(c, texpool.lut.data(), texpool.lut.size(), &s.tex.lut);
}

// the scalars of the device scene, and the scene becomes the context's
void publish_scene(ptgs_ctx* c, const ptgs_scene_desc* d, const FlatScene& flat, DevScene& s) {
  s.tex.count = d->num_textures;
  s.uses_textures = 0;
  for (uint32_t i = 0; i < d->num_materials; ++i) {
    const ptgs_material& m = d->materials[i];
    if (m.albedo_texture_index > 0 || m.normal_texture_index > 0 || m.metallic_roughness_texture_index > 0 ||
        m.emissive_texture_index > 0 || m.clearcoat_texture_index > 0 || m.clearcoat_roughness_texture_index > 0 ||
        m.sg_id > 0)
      s.uses_textures = 1;
  }
  s.num_light_cdf = d->num_light_cdf;
  s.num_plights = d->num_punctual_lights;
  s.bn_size = (int32_t)d->blue_noise_size;
  s.has_transparent = flat.has_transparent ? 1 : 0;
  c->dsc = s;
  c->has_scene = true;
  c->info.num_triangles = (uint32_t)flat.tris.size();
}

}  // namespace

extern "C" {

int ptgs_abi_version(void) { return PTGS_ABI_VERSION; }
const char* ptgs_device_arch(void) { return "gfx950"; }

int ptgs_create(int hip_device, ptgs_ctx** out) {
  if (!out) return PTGS_EINVAL;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return PTGS_EHIP;
  if (hip_device < 0 || hip_device >= n) return PTGS_EINVAL;
  ptgs_ctx* c = new ptgs_ctx();
  c->device = hip_device;
  if (hipSetDevice(hip_device) != hipSuccess) { delete c; return PTGS_EHIP; }
  if (hipMalloc(&c->counters, 8 * sizeof(unsigned long long)) != hipSuccess) { delete c; return PTGS_EHIP; }
  if (hipMemset(c->counters, 0, 8 * sizeof(unsigned long long)) != hipSuccess) { delete c; return PTGS_EHIP; }
  c->densify = densify_workspace_create();
  c->loss = loss_workspace_create();
  if (c->mse_partials.ensure(TRAIN_MSE_MAX_WG * sizeof(double), 0) != hipSuccess) {
    ptgs_destroy(c);
    return PTGS_EHIP;
  }
  *out = c;
  return PTGS_OK;
}

void ptgs_destroy(ptgs_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  free_scene(c);
  if (c->counters) (void)hipFree(c->counters);
  ptgs::wf_workspace_free(c->wf);
  ptgs::free_pt_sched(c->pt_sched);
  densify_workspace_destroy(c->densify);
  loss_workspace_destroy(c->loss);
  if (c->comm) (void)comm_destroy(c->comm);
  delete c;  // (~SplatFrames: the splat workspaces, streams, events and signal word)
}

int ptgs_comm_unique_id(uint8_t id[PTGS_COMM_ID_BYTES]) {
  if (!id) return PTGS_EINVAL;
  if (!comm_available()) return PTGS_EHIP;
  return comm_unique_id(id) == 0 ? PTGS_OK : PTGS_EHIP;
}

int ptgs_comm_create(ptgs_ctx* c, const uint8_t id[PTGS_COMM_ID_BYTES], int nranks, int rank) {
  if (!c || !id) return PTGS_EINVAL;
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(c, PTGS_EINVAL, "bad rank %d of %d", rank, nranks);
  if (!comm_available()) return fail(c, PTGS_EHIP, "RCCL (librccl.so.1) could not be loaded");
  HIPCHK(c, hipSetDevice(c->device));
  if (c->comm) {
    (void)comm_destroy(c->comm);
    c->comm = nullptr;
  }
  int e = comm_create(id, nranks, rank, &c->comm);
  if (e) return fail(c, PTGS_EHIP, "ncclCommInitRank: %s", comm_error(e));
  c->comm_ranks = nranks;
  c->comm_rank = rank;
  return PTGS_OK;
}

int ptgs_comm_destroy(ptgs_ctx* c) {
  if (!c) return PTGS_EINVAL;
  if (c->comm) {
    int e = comm_destroy(c->comm);
    c->comm = nullptr;
    if (e) return fail(c, PTGS_EHIP, "ncclCommDestroy: %s", comm_error(e));
  }
  return PTGS_OK;
}

static int reduce_common(ptgs_ctx* c, float* accum, size_t n, int root, bool all, void* stream) {
  if (!c || !accum) return PTGS_EINVAL;
  if (!c->comm) return fail(c, PTGS_EINVAL, "no communicator (ptgs_comm_create)");
  if (!is_device_ptr(accum)) return fail(c, PTGS_EINVAL, "accum is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  int e = all ? comm_allreduce_sum(c->comm, accum, n, (hipStream_t)stream)
              : comm_reduce_sum(c->comm, accum, n, root, (hipStream_t)stream);
  if (e) return fail(c, PTGS_EHIP, "%s: %s", all ? "ncclAllReduce" : "ncclReduce", comm_error(e));
  return PTGS_OK;
}

int ptgs_reduce_radiance(ptgs_ctx* c, float* accum, size_t n_floats, int root, void* stream) {
  return reduce_common(c, accum, n_floats, root, false, stream);
}

int ptgs_allreduce_radiance(ptgs_ctx* c, float* accum, size_t n_floats, void* stream) {
  return reduce_common(c, accum, n_floats, 0, true, stream);
}

int ptgs_gather_rows(ptgs_ctx* c, float* image, uint32_t width, uint32_t height, const uint32_t* row_ranges,
                     int root, void* stream) {
  if (!c || !image || !row_ranges) return PTGS_EINVAL;
  if (!c->comm) return fail(c, PTGS_EINVAL, "no communicator (ptgs_comm_create)");
  if (root < 0 || root >= c->comm_ranks) return fail(c, PTGS_EINVAL, "bad root %d", root);
  if (!is_device_ptr(image)) return fail(c, PTGS_EINVAL, "image is not a device pointer");
  if (const int bad = check_row_ranges(c, row_ranges, height)) return bad;
  HIPCHK(c, hipSetDevice(c->device));
  int e = comm_gather_rows(c->comm, image, (size_t)width * 4u, row_ranges, c->comm_ranks, c->comm_rank, root,
                           (hipStream_t)stream);
  if (e) return fail(c, PTGS_EHIP, "ncclSend/ncclRecv: %s", comm_error(e));
  return PTGS_OK;
}

int ptgs_reduce_scatter_rows(ptgs_ctx* c, float* image, uint32_t width, uint32_t height, const uint32_t* row_ranges,
                             void* stream) {
  if (!c || !image || !row_ranges) return PTGS_EINVAL;
  if (!c->comm) return fail(c, PTGS_EINVAL, "no communicator (ptgs_comm_create)");
  if (!is_device_ptr(image)) return fail(c, PTGS_EINVAL, "image is not a device pointer");
  if (const int bad = check_row_ranges(c, row_ranges, height)) return bad;
  HIPCHK(c, hipSetDevice(c->device));
  int e = comm_reduce_rows(c->comm, image, (size_t)width * 4u, row_ranges, c->comm_ranks, (hipStream_t)stream);
  if (e) return fail(c, PTGS_EHIP, "ncclReduce: %s", comm_error(e));
  return PTGS_OK;
}

const char* ptgs_last_error(const ptgs_ctx* c) { return c ? c->err.c_str() : "null context"; }

int ptgs_scene_upload(ptgs_ctx* c, const ptgs_scene_desc* d) {
  if (!c || !d) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  int rc;
  std::string msg;
  if ((rc = validate_scene_desc(d, msg))) return fail(c, rc, "%s", msg.c_str());
  TexturePool texpool;
  if (!build_texture_pool(d->textures, d->num_textures, texpool, msg)) return fail(c, PTGS_EINVAL, "%s", msg.c_str());
  if (texpool.texels.size() >= (1ull << 32)) return fail(c, PTGS_ERANGE, "texture pool exceeds 2^32 texels");
  FlatScene flat;
  if ((rc = flatten_scene(d, flat, msg))) return fail(c, rc, "%s", msg.c_str());

  free_scene(c);
  c->info = ptgs_scene_info{};
  c->build = ptgs_scene_build{};
  c->tree_opt = ptgs_scene_tree_opt{};
  DevScene s{};
  // BVH: the host binned-SAH build (default), or with PTGS_FLAG_GPU_BVH one of the GPU builders (the SAH
  // build with the host's tries, or with PTGS_FLAG_GPU_LBVH the LBVH), falling back to the host build when
  // the GPU builder does not support the input or none of its trees fits the traversal stack
  bool built = false;
  if ((c->flags & PTGS_FLAG_GPU_BVH) && flat.tris.size() >= 16) {
    rc = (c->flags & PTGS_FLAG_GPU_LBVH)
             ? build_tree_gpu<GpuLbvhBuilder>(c, flat.tris, lbvh_bvh_tries(PTGS_STACK), s, &built)
             : build_tree_gpu<GpuSahBuilder>(c, flat.tris, parse_bvh_tries(getenv("PTGS_BVH_TRIES"), PTGS_STACK), s,
                                             &built);
    if (rc) return rc;
  }
  std::vector<float> host_n4;  // the final 4-wide nodes when the host built them
  if (!built && (rc = build_tree_host(c, flat.tris, s, host_n4))) return rc;
  if ((rc = check_node_window(c))) return rc;
  if ((rc = upload_traversal_nodes(c, host_n4, s))) return rc;
  if ((rc = upload_scene_arrays(c, d, flat, texpool, s))) return rc;
  publish_scene(c, d, flat, s);
  return PTGS_OK;
}

int ptgs_scene_get_info(const ptgs_ctx* c, ptgs_scene_info* out) {
  if (!c || !out) return PTGS_EINVAL;
  if (!c->has_scene) return PTGS_ENOSCENE;
  *out = c->info;
  return PTGS_OK;
}

int ptgs_scene_get_build(const ptgs_ctx* c, ptgs_scene_build* out) {
  if (!c || !out) return PTGS_EINVAL;
  if (!c->has_scene) return PTGS_ENOSCENE;
  *out = c->build;
  return PTGS_OK;
}

int ptgs_scene_get_tree_opt(const ptgs_ctx* c, ptgs_scene_tree_opt* out) {
  if (!c || !out) return PTGS_EINVAL;
  if (!c->has_scene) return PTGS_ENOSCENE;
  *out = c->tree_opt;
  return PTGS_OK;
}

int ptgs_scene_get_pt_stack(const ptgs_ctx* c, uint32_t* lds_depth, uint32_t* walked_need, uint32_t* deep) {
  if (!c) return PTGS_EINVAL;
  if (!c->has_scene) return PTGS_ENOSCENE;
  if (lds_depth) *lds_depth = c->dsc.pt_deep_stack ? PTGS_STACK : PTGS_PT_STACK;  // (pt_kernels.hip pt_lds_stack)
  if (walked_need) *walked_need = c->pt_walked_need;
  if (deep) *deep = c->dsc.pt_deep_stack ? 1u : 0u;
  return PTGS_OK;
}

int ptgs_scene_get_bvh(const ptgs_ctx* c, ptgs_bvh_buffers* out) {
  if (!c || !out) return PTGS_EINVAL;
  if (!c->has_scene) return PTGS_ENOSCENE;
  out->nodes = (const float*)c->dsc.nodes;
  out->num_nodes = c->info.num_bvh_nodes;
  out->triangles = (const float*)c->dsc.tris;
  out->num_triangles = c->info.num_triangles;
  return PTGS_OK;
}

int ptgs_trace_camera_rows(ptgs_ctx* c, const ptgs_ubo* ubo, uint32_t w, uint32_t h, uint32_t row_begin,
                           uint32_t row_end, float* accum, uint32_t spp, uint32_t frame_stride,
                           uint32_t accum_mode, void* stream) {
  if (!c || !ubo || !accum) return fail(c, PTGS_EINVAL, "null argument");
  if (!c->has_scene) return fail(c, PTGS_ENOSCENE, "no scene uploaded");
  if (const int bad = check_image_size(c, w, h)) return bad;
  if (row_end > h) row_end = h;
  if (row_begin > row_end) return fail(c, PTGS_EINVAL, "bad row range");
  if (frame_stride == 0) return fail(c, PTGS_EINVAL, "frame_stride must be >= 1");
  if (accum_mode > PTGS_ACCUM_SUM) return fail(c, PTGS_EINVAL, "bad accum mode");
  if (!is_device_ptr(accum)) return fail(c, PTGS_EINVAL, "accum is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  CamParams cp;
  int rc = fill_cam(c, ubo, cp);
  if (rc) return rc;
  const bool stats = (c->flags & PTGS_FLAG_COUNT_TRAVERSAL) != 0;
  hipError_t e;
  if (c->flags & PTGS_FLAG_PT_WAVEFRONT) {
    e = ptgs::launch_pt_wavefront(c->wf, c->dsc, cp, accum, w, h, row_begin, row_end, spp, ubo->frame_count,
                                  frame_stride, accum_mode, c->counters, stats, (hipStream_t)stream);
    return hip_rc(c, e, "wavefront path tracer");
  }
  e = launch_pt_camera(c->dsc, cp, accum, w, h, row_begin, row_end, spp, ubo->frame_count, frame_stride, accum_mode,
                       c->counters, stats, &c->pt_sched, (hipStream_t)stream);
  return hip_rc(c, e, "pt_camera launch");
}

int ptgs_trace_camera(ptgs_ctx* c, const ptgs_ubo* ubo, uint32_t w, uint32_t h, float* accum, uint32_t spp,
                      uint32_t frame_stride, uint32_t accum_mode, void* stream) {
  return ptgs_trace_camera_rows(c, ubo, w, h, 0, h, accum, spp, frame_stride, accum_mode, stream);
}

int ptgs_trace_depth(ptgs_ctx* c, const ptgs_ubo* ubo, uint32_t w, uint32_t h, float* depth, void* stream) {
  return ptgs_trace_depth_rows(c, ubo, w, h, 0, h, depth, stream);
}

int ptgs_trace_depth_rows(ptgs_ctx* c, const ptgs_ubo* ubo, uint32_t w, uint32_t h, uint32_t row_begin,
                          uint32_t row_end, float* depth, void* stream) {
  if (!c || !ubo || !depth) return fail(c, PTGS_EINVAL, "null argument");
  if (!c->has_scene) return fail(c, PTGS_ENOSCENE, "no scene uploaded");
  if (const int bad = check_image_size(c, w, h)) return bad;
  if (!is_device_ptr(depth)) return fail(c, PTGS_EINVAL, "depth is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  CamParams cp;
  int rc = fill_cam(c, ubo, cp);
  if (rc) return rc;
  ViewMat vm;
  std::memcpy(vm.m, ubo->view, sizeof(vm.m));
  hipError_t e = launch_pt_depth(c->dsc, cp, vm, depth, w, h, row_begin, row_end, ubo->frame_count, (hipStream_t)stream);
  return hip_rc(c, e, "pt_depth launch");
}

int ptgs_trace_torus(ptgs_ctx* c, const ptgs_ubo* ubo, const ptgs_ray_push* push, const ptgs_ray_sample* samples,
                     uint32_t n, ptgs_hitdata* hits, void* stream) {
  if (!c || !ubo || !push) return fail(c, PTGS_EINVAL, "null argument");
  if (!c->has_scene) return fail(c, PTGS_ENOSCENE, "no scene uploaded");
  if (n == 0) return PTGS_OK;
  if (!is_device_ptr(samples) || !is_device_ptr(hits)) return fail(c, PTGS_EINVAL, "samples/hits must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  CamParams cp;
  int rc = fill_cam(c, ubo, cp);
  if (rc) return rc;
  TorusParams tp;
  std::memcpy(tp.model, push->model, sizeof(tp.model));
  tp.major_radius = push->major_radius;
  tp.minor_radius = push->minor_radius;
  tp.height = push->height;
  // side = ceil(sqrt(n)) (engine.cpp:2786)
  uint32_t side = (uint32_t)std::ceil(std::sqrt((double)n));
  while ((uint64_t)side * side < n) side++;
  hipError_t e = launch_pt_torus(c->dsc, cp, tp, samples, n, side, ubo->frame_count, hits, c->counters,
                                 (c->flags & PTGS_FLAG_COUNT_TRAVERSAL) != 0, (hipStream_t)stream);
  return hip_rc(c, e, "pt_torus launch");
}

int ptgs_set_flags(ptgs_ctx* c, uint32_t flags) {
  if (!c) return PTGS_EINVAL;
  c->flags = flags;
  return PTGS_OK;
}

int ptgs_stats_reset(ptgs_ctx* c, void* stream) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMemsetAsync(c->counters, 0, 8 * sizeof(unsigned long long), (hipStream_t)stream));
  return PTGS_OK;
}

int ptgs_stats_read(ptgs_ctx* c, ptgs_trace_stats* out) {
  if (!c || !out) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipDeviceSynchronize());
  unsigned long long v[8];
  HIPCHK(c, hipMemcpy(v, c->counters, sizeof(v), hipMemcpyDeviceToHost));
  out->extension_rays = v[0];
  out->shadow_rays = v[1];
  out->samples = v[2];
  out->node_visits = v[3];
  out->tri_tests = v[4];
  out->closest_hits = v[5];
  return PTGS_OK;
}

int ptgs_device_alloc(ptgs_ctx* c, size_t bytes, void** out) {
  if (!c || !out) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipMalloc(out, bytes ? bytes : 16));
  return PTGS_OK;
}
int ptgs_device_free(ptgs_ctx* c, void* p) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipFree(p));
  return PTGS_OK;
}
int ptgs_memcpy_h2d(ptgs_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return PTGS_OK;
}
int ptgs_memcpy_d2h(ptgs_ctx* c, void* dst, const void* src, size_t bytes) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return PTGS_OK;
}
int ptgs_memset_d32(ptgs_ctx* c, void* dst, uint32_t value, size_t count, void* stream) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)dst, (int)value, count, (hipStream_t)stream));
  return PTGS_OK;
}
int ptgs_synchronize(ptgs_ctx* c) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipDeviceSynchronize());
  return PTGS_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// rasterizers
// ---------------------------------------------------------------------------------------------
#include "raster.h"

extern "C" {

// The argument checks of a splat frame that need no device work. Every entry point runs them before it
// changes any state of the context (the overlap ring above all: a rejected call must leave the current
// workspace, the ring position and the run's blend ordinals as the latest rendered frame left them).
static int splat_check_args(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                            const float* depth, const float* under, const float* out) {
  if (const int bad = check_image_size(c, w, h)) return bad;
  if (g->count && (!is_device_ptr(g->means) || !is_device_ptr(g->scales) || !is_device_ptr(g->rotations) ||
                   !is_device_ptr(g->opacities) || !is_device_ptr(g->colors) || (g->ids && !is_device_ptr(g->ids))))
    return fail(c, PTGS_EINVAL, "gaussian arrays must be device pointers");
  if (!is_device_ptr(out)) return fail(c, PTGS_EINVAL, "out is not a device pointer");
  if ((depth && !is_device_ptr(depth)) || (under && !is_device_ptr(under)))
    return fail(c, PTGS_EINVAL, "depth / under must be device pointers");
  if (ubo->proj[0] == 0.0f || ubo->proj[5] == 0.0f) return fail(c, PTGS_EINVAL, "degenerate projection");
  return PTGS_OK;
}

// Renders one frame whose arguments passed splat_check_args into workspace ws; PTGS_OK means it was enqueued
// completely. *report (SplatReport: an earlier frame was left incomplete / met ids >= count) is about
// EARLIER frames of the workspace: the caller turns it into PTGS_EINCOMPLETE / PTGS_EBADIDS (splat_finish)
// once everything it renders is enqueued.
static int splat_render(ptgs_ctx* c, SplatWorkspace* ws, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w,
                        uint32_t h, const float bg[3], const float* depth, const float* under, uint32_t tile_row_begin,
                        uint32_t tile_row_end, float* out, ptgs_splat_stats* stats, void* stream, uint32_t* report,
                        const SplatOverlap* ov = nullptr, SplatSeq* seq = nullptr) {
  *report = 0;
  HIPCHK(c, hipSetDevice(c->device));
  float mvp[16];
  mat4_mul(ubo->proj, ubo->view, mvp);
  SplatArgs a;
  a.g = g;
  a.view = ubo->view;
  a.mvp = mvp;
  a.p00 = ubo->proj[0];
  a.p11 = ubo->proj[5];
  a.W = w;
  a.H = h;
  a.bg = bg;
  a.depth = depth;
  a.under = under;
  a.tile_row_begin = tile_row_begin;
  a.tile_row_end = tile_row_end;
  a.out = out;
  a.stats = stats;
  a.time_stages = (c->flags & PTGS_FLAG_TIME_STAGES) != 0;
  a.publish = (c->flags & PTGS_FLAG_SPLAT_PUBLISH) != 0;
  a.publish_tight = (c->flags & PTGS_FLAG_SPLAT_PUBLISH_TIGHT) != 0;
  a.stream = (hipStream_t)stream;
  a.ov = ov;
  a.seq = seq;
  hipError_t e = splat_gaussians(ws, a, report);
  return hip_rc(c, e, "splat_gaussians");
}

// The reports a call collected (earlier frames' flags, consumed from the workspaces) and its own result rc:
// which code the call returns and what is kept for the next call is latch_report's (splat_run.h).
// (the frames of this call are rendered; the two report codes are about earlier frames of the workspace(s))
static int splat_finish(ptgs_ctx* c, int rc, uint32_t report) {
  const SplatLatch l = latch_report(c->frames.pending_report, rc == PTGS_OK, report);
  c->frames.pending_report = l.pending;
  switch (l.code) {
    case SplatCode::BadIds:
      return fail(c, PTGS_EBADIDS, "an earlier splat frame met ptgs_gaussians.ids entries >= count");
    case SplatCode::Incomplete:
      return fail(c, PTGS_EINCOMPLETE, "an earlier splat frame left tiles incomplete (spill pool exhausted; grown)");
    default:
      return rc;  // (SplatCode::Ok: rc is PTGS_OK; SplatCode::Own: the call's own code)
  }
}

// PTGS_FLAG_SPLAT_OVERLAP: the call takes the ring's next workspace (the one of the call depth calls back)
// and, for a stream-ordered frame, its front end runs on the context's second stream. The first call of a
// run of overlapped calls starts it after everything the caller's stream holds; later calls' front ends
// wait on the device for the earlier blends of their workspace only (gs_done_wait), so inputs the caller
// writes during a run are not seen by it. A call without the flag ends the run (end_run).
//
// What an overlapped call needs, created when a context first overlaps: the ring's other workspaces (their
// number is fixed then: PTGS_GS_OV_DEPTH, A/B switch), the front-end stream, the two events, the signal word.
static int splat_overlap_resources(ptgs_ctx* c) {
  SplatFrames& f = c->frames;
  if (!f.run.depth) f.run.depth = splat_ring_depth(getenv("PTGS_GS_OV_DEPTH"));
  for (uint32_t i = 1; i < f.run.depth; ++i)
    if (!f.ring[i]) f.ring[i] = splat_workspace_create();
  if (!f.fe) {
    // the front end's queue at the highest priority, so its workgroups take the CU slots of the blend's
    // retiring workgroups early instead of waiting for the blend's tail (PTGS_GS_OV_PRIO=normal: A/B switch)
    int least = 0, greatest = 0, prio = 0;
    const char* pv = getenv("PTGS_GS_OV_PRIO");
    if (!(pv && !strcmp(pv, "normal")) && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess)
      prio = greatest;
    HIPCHK(c, hipStreamCreateWithPriority(&f.fe, hipStreamNonBlocking, prio));
  }
  // (device-scope events: both streams are on this device, so no system-scope release (an L2 write-back)
  // is needed at the record; PTGS_GS_OV_FENCE=1 restores it: A/B switch)
  static const unsigned ev_flags = [] {
    const char* v = getenv("PTGS_GS_OV_FENCE");
    return (unsigned)(hipEventDisableTiming | (v && !strcmp(v, "1") ? 0u : (unsigned)hipEventDisableSystemFence));
  }();
  for (hipEvent_t* ev : {&f.marker, &f.done})
    if (!*ev) HIPCHK(c, hipEventCreateWithFlags(ev, ev_flags));
  if (!f.signal) {  // (signal memory for the front end's wait-value packet; zero before any blend stores)
    HIPCHK(c, hipExtMallocWithFlags((void**)&f.signal, 8, hipMallocSignalMemory));
    HIPCHK(c, hipMemset(f.signal, 0, 8));
  }
  return PTGS_OK;
}

static int splat_overlap_begin(ptgs_ctx* c, hipStream_t s, SplatOverlap* ov, SplatSeq* seq) {
  HIPCHK(c, hipSetDevice(c->device));
  if (const int rc = splat_overlap_resources(c)) return rc;
  SplatFrames& f = c->frames;
  // the next ring slot; the workspace there was last used depth calls ago (call k - depth). Its blend ran
  // before the blend of call k - depth + 1 on the caller's stream, so once THAT blend has started (its
  // ordinal in the signal word, SplatSeq) the workspace is free: the front end's queue waits for that value
  // and the caller's queue carries no marker (a marker beside the cross-queue barrier had cost it ~3-5 us per
  // frame: tools/micro/queue_sync.hip, wait + marker 28.0 vs wait alone 25.1 us on a 22 us kernel; kernel
  // trace 10.5 vs 6.0 us between two blends). When that is not known the front end waits for a marker of the
  // caller's stream instead (next_wait, splat_run.h, has the rule).
  f.advance();
  const SplatWait wait = next_wait(f.run, s);
  if (wait.kind == SplatWait::NewMarker) HIPCHK(c, hipEventRecord(f.marker, s));
  const bool by_ordinal = wait.kind == SplatWait::Ordinal;
  ov->fe = f.fe;
  ov->done = f.done;
  ov->wait = by_ordinal ? nullptr : f.marker;
  ov->wait_flag = by_ordinal ? f.signal : nullptr;
  ov->wait_ordinal = wait.ordinal;
  seq->flag = f.signal;
  seq->ordinal = f.run.next_ordinal;
  seq->launched = false;
  // the blend's tile order: the front end's order workgroup from the workspace's previous frame (default),
  // or PTGS_GS_OV_ORDER=own: a launch behind the front end from the frame's own counts (A/B switch;
  // measured slower at C2 static, 0.0531 vs 0.0521 ms, and not faster on the orbit: DESIGN §5 round 6)
  static const bool own_order = [] {
    const char* v = getenv("PTGS_GS_OV_ORDER");
    return v && !strcmp(v, "own");
  }();
  ov->own_order = own_order;
  return PTGS_OK;
}

static int splat_common(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                        const float bg[3], const float* depth, const float* under, uint32_t tile_row_begin,
                        uint32_t tile_row_end, float* out, ptgs_splat_stats* stats, void* stream) {
  uint32_t report = 0;
  SplatOverlap ov{};
  SplatSeq seq{};
  const SplatOverlap* ovp = nullptr;
  // (before the ring advances: after a rejected call ptgs_splat_get_buffers / _get_tile_rows / _status_read
  // still describe the latest rendered frame, and the run goes on as if the call had not been made: nothing
  // is recorded in the run, so the next front end's wait value is still the ordinal of a blend that a call
  // recorded as launched, or the marker)
  const int bad = splat_check_args(c, g, ubo, w, h, depth, under, out);
  if (bad != PTGS_OK) return bad;
  SplatFrames& f = c->frames;
  if (c->flags & PTGS_FLAG_SPLAT_OVERLAP) {
    const int rc = splat_overlap_begin(c, (hipStream_t)stream, &ov, &seq);
    if (rc != PTGS_OK) return rc;
    ovp = &ov;  // (splat_gaussians runs a frame with stats / publish / stage timing serially anyway)
  } else {
    end_run(f.run);
  }
  const int rc = splat_render(c, f.current(), g, ubo, w, h, bg, depth, under, tile_row_begin, tile_row_end, out, stats,
                              stream, &report, ovp, ovp ? &seq : nullptr);
  if (ovp) record(f.run, stream, seq.launched, seq.ordinal);  // (its blend's ordinal and stream: next_wait)
  return splat_finish(c, rc, report);
}

int ptgs_splat_gaussians(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                         const float bg[3], uint32_t tile_row_begin, uint32_t tile_row_end, float* out,
                         ptgs_splat_stats* stats, void* stream) {
  if (!c || !g || !ubo || !out || !bg) return fail(c, PTGS_EINVAL, "null argument");
  return splat_common(c, g, ubo, w, h, bg, nullptr, nullptr, tile_row_begin, tile_row_end, out, stats, stream);
}

int ptgs_splat_gaussians_over(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                              const float* depth, const float* under_rgba32f, uint32_t tile_row_begin,
                              uint32_t tile_row_end, float* out, ptgs_splat_stats* stats, void* stream) {
  if (!c || !g || !ubo || !out || !depth || !under_rgba32f) return fail(c, PTGS_EINVAL, "null argument");
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  return splat_common(c, g, ubo, w, h, zero, depth, under_rgba32f, tile_row_begin, tile_row_end, out, stats, stream);
}

int ptgs_splat_gaussians_views(ptgs_ctx* c, const ptgs_gaussians* g, uint32_t n_views, const ptgs_ubo* ubos,
                               uint32_t w, uint32_t h, const float bg[3], float* const* outs, void* stream) {
  if (!c || !g || !ubos || !outs || !bg) return fail(c, PTGS_EINVAL, "null argument");
  if (n_views == 0 || n_views > PTGS_MAX_VIEWS) return fail(c, PTGS_EINVAL, "n_views %u not in [1, %d]", n_views, PTGS_MAX_VIEWS);
  for (uint32_t v = 0; v < n_views; ++v)
    if (!outs[v]) return fail(c, PTGS_EINVAL, "null output of view %u", v);
  if (n_views == 1) return splat_common(c, g, &ubos[0], w, h, bg, nullptr, nullptr, 0, ~0u, outs[0], nullptr, stream);
  for (uint32_t v = 0; v < n_views; ++v) {  // (every view's arguments before any view is forked)
    const int bad = splat_check_args(c, g, &ubos[v], w, h, nullptr, nullptr, outs[v]);
    if (bad != PTGS_OK) return bad;
  }
  HIPCHK(c, hipSetDevice(c->device));
  SplatFrames& f = c->frames;
  end_run(f.run);  // (view 0 renders serially on the caller's stream with the latest workspace)
  const hipStream_t s = (hipStream_t)stream;
  if (!f.fork) HIPCHK(c, hipEventCreateWithFlags(&f.fork, hipEventDisableTiming));
  // every view's pair buffer starts from the largest pair count any slot has seen (views of one
  // Gaussian set have similar counts): a fresh view workspace would otherwise start at 8 pairs per
  // Gaussian and skip its first over-capacity frame (reported by ptgs_splat_status_read)
  uint32_t hint = splat_pair_hint(f.current());
  for (uint32_t v = 1; v < n_views; ++v) {
    SplatFrames::View& vw = f.view(v);
    if (!vw.ws) vw.ws = splat_workspace_create();
    if (!vw.stream) HIPCHK(c, hipStreamCreateWithFlags(&vw.stream, hipStreamNonBlocking));
    if (!vw.join) HIPCHK(c, hipEventCreateWithFlags(&vw.join, hipEventDisableTiming));
    hint = std::max(hint, splat_pair_hint(vw.ws));
  }
  if (hint) {
    const uint32_t want = hint + hint / 8u;  // headroom for the views' differences
    for (uint32_t v = 1; v < n_views; ++v) HIPCHK(c, splat_reserve(f.view(v).ws, want));
  }
  HIPCHK(c, hipEventRecord(f.fork, s));  // the views start after the caller's earlier work
  // on any failure after a view was forked, the views already launched are joined back into the
  // caller's stream before returning (later work there must not race them)
  uint32_t launched = 1;
  uint32_t report = 0;  // the views' reports about their earlier frames (PTGS_EINCOMPLETE / PTGS_EINVAL)
  auto join = [&]() {
    for (uint32_t v = 1; v < launched; ++v) (void)hipStreamWaitEvent(s, f.view(v).join, 0);
  };
  for (uint32_t v = 1; v < n_views; ++v) {
    const SplatFrames::View& vw = f.view(v);
    hipError_t e = hipStreamWaitEvent(vw.stream, f.fork, 0);
    if (e != hipSuccess) {
      join();
      return splat_finish(c, hip_rc(c, e, "hipStreamWaitEvent"), report);
    }
    uint32_t rep = 0;
    const int rc = splat_render(c, vw.ws, g, &ubos[v], w, h, bg, nullptr, nullptr, 0, ~0u, outs[v], nullptr, vw.stream,
                                &rep);
    report |= rep;  // (about earlier frames of view v's workspace: returned once every view is enqueued)
    // (record the join even after a failed view: kernels it did enqueue must be waited for)
    e = hipEventRecord(vw.join, vw.stream);
    if (e == hipSuccess) launched = v + 1;
    if (rc != PTGS_OK) { join(); return splat_finish(c, rc, report); }
    if (e != hipSuccess) { join(); return splat_finish(c, hip_rc(c, e, "hipEventRecord"), report); }
  }
  uint32_t rep = 0;
  const int rc = splat_render(c, f.current(), g, &ubos[0], w, h, bg, nullptr, nullptr, 0, ~0u, outs[0], nullptr, stream,
                              &rep);
  join();
  return splat_finish(c, rc, report | rep);
}

int ptgs_gaussians_sort_spatial(ptgs_ctx* c, const ptgs_gaussians* g, float* means, float* scales, float* rotations,
                                float* opacities, float* colors, uint32_t* ids, void* stream) {
  if (!c || !g) return fail(c, PTGS_EINVAL, "null argument");
  if (g->count) {
    const void* all[] = {g->means, g->scales, g->rotations, g->opacities, g->colors, means, scales, rotations,
                         opacities, colors, ids};
    for (const void* p : all)
      if (!is_device_ptr(p)) return fail(c, PTGS_EINVAL, "gaussian arrays must be device pointers");
    if (g->ids && !is_device_ptr(g->ids)) return fail(c, PTGS_EINVAL, "ids must be a device pointer");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_sort_spatial(g, means, scales, rotations, opacities, colors, ids, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_sort_spatial");
}

int ptgs_gaussians_chunk_bounds(ptgs_ctx* c, const ptgs_gaussians* g, float* bounds, void* stream) {
  if (!c || !g || !bounds) return fail(c, PTGS_EINVAL, "null argument");
  if (g->count && (!is_device_ptr(g->means) || !is_device_ptr(g->scales) || !is_device_ptr(bounds)))
    return fail(c, PTGS_EINVAL, "means / scales / bounds must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_chunk_bounds(g, bounds, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_chunk_bounds");
}

int ptgs_gaussians_sh_colors(ptgs_ctx* c, const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                             uint32_t active_degree, const float camera_pos[3], float* colors, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (sh_degree > 3) return fail(c, PTGS_EINVAL, "sh_degree %u above 3", sh_degree);
  if (active_degree > sh_degree)
    return fail(c, PTGS_EINVAL, "active_degree %u above the stored sh_degree %u", active_degree, sh_degree);
  if (count == 0) return PTGS_OK;  // (empty arrays may be null)
  if (!means || !sh || !camera_pos || !colors) return fail(c, PTGS_EINVAL, "null argument");
  // (a per-frame call: one pointer query, of the array that is written, like the other frame entry points)
  if (!is_device_ptr(colors)) return fail(c, PTGS_EINVAL, "colors is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e =
      splat_sh_colors(means, sh, count, sh_degree, active_degree, camera_pos, colors, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_sh_colors");
}

int ptgs_gaussians_activate(ptgs_ctx* c, const float* log_scales, const float* opacity_logits, uint32_t count,
                            float* scales, float* opacities, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (count == 0) return PTGS_OK;
  if (!log_scales || !opacity_logits || !scales || !opacities) return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(log_scales) || !is_device_ptr(opacity_logits) || !is_device_ptr(scales) ||
      !is_device_ptr(opacities))
    return fail(c, PTGS_EINVAL, "log_scales / opacity_logits / scales / opacities must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_sh_activate(log_scales, opacity_logits, count, scales, opacities, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_activate");
}

// ptgs_gaussians_sh_colors_backward and _backward_eye (eye: dL_dcamera_pos is written as well)
static int sh_backward_call(ptgs_ctx* c, const float* means, const float* sh, uint32_t count, uint32_t sh_degree,
                            uint32_t active_degree, const float camera_pos[3], const float* dL_dcolors, float* dL_dsh,
                            float* dL_dmeans, bool eye, float* dL_dcamera_pos, void* stream, const char* name) {
  if (!c) return PTGS_EINVAL;
  if (sh_degree > 3) return fail(c, PTGS_EINVAL, "sh_degree %u above 3", sh_degree);
  if (active_degree > sh_degree)
    return fail(c, PTGS_EINVAL, "active_degree %u above the stored sh_degree %u", active_degree, sh_degree);
  if (eye && !dL_dcamera_pos) return fail(c, PTGS_EINVAL, "null argument (dL_dcamera_pos)");
  if (eye && !is_device_ptr(dL_dcamera_pos)) return fail(c, PTGS_EINVAL, "dL_dcamera_pos is not a device pointer");
  if (count == 0) {  // (empty arrays may be null)
    if (!eye) return PTGS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return hip_rc(c, hipMemsetAsync(dL_dcamera_pos, 0, 3 * sizeof(float), (hipStream_t)stream), name);
  }
  if (!means || !sh || !camera_pos || !dL_dcolors || !dL_dsh) return fail(c, PTGS_EINVAL, "null argument");
  if (dL_dsh == sh) return fail(c, PTGS_EINVAL, "dL_dsh must not alias sh");
  if (!is_device_ptr(dL_dsh)) return fail(c, PTGS_EINVAL, "dL_dsh is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  if (!eye)
    return hip_rc(c, splat_sh_colors_backward(means, sh, count, sh_degree, active_degree, camera_pos, dL_dcolors,
                                              dL_dsh, dL_dmeans, (hipStream_t)stream), name);
  // (growth frees the old buffer, which waits for the device)
  const size_t bytes = (size_t)splat_sh_eye_rows(count) * 3 * sizeof(float);
  HIPCHK(c, c->sh_eye_partials.ensure(bytes, bytes / 4));
  return hip_rc(c, splat_sh_colors_backward_eye(means, sh, count, sh_degree, active_degree, camera_pos, dL_dcolors,
                                                dL_dsh, dL_dmeans, c->sh_eye_partials.as<float>(), dL_dcamera_pos,
                                                (hipStream_t)stream), name);
}

int ptgs_gaussians_sh_colors_backward(ptgs_ctx* c, const float* means, const float* sh, uint32_t count,
                                      uint32_t sh_degree, uint32_t active_degree, const float camera_pos[3],
                                      const float* dL_dcolors, float* dL_dsh, float* dL_dmeans, void* stream) {
  return sh_backward_call(c, means, sh, count, sh_degree, active_degree, camera_pos, dL_dcolors, dL_dsh, dL_dmeans,
                          false, nullptr, stream, "ptgs_gaussians_sh_colors_backward");
}

int ptgs_gaussians_sh_colors_backward_eye(ptgs_ctx* c, const float* means, const float* sh, uint32_t count,
                                          uint32_t sh_degree, uint32_t active_degree, const float camera_pos[3],
                                          const float* dL_dcolors, float* dL_dsh, float* dL_dmeans,
                                          float* dL_dcamera_pos, void* stream) {
  return sh_backward_call(c, means, sh, count, sh_degree, active_degree, camera_pos, dL_dcolors, dL_dsh, dL_dmeans,
                          true, dL_dcamera_pos, stream, "ptgs_gaussians_sh_colors_backward_eye");
}

int ptgs_gaussians_activate_backward(ptgs_ctx* c, const float* scales, const float* opacities, uint32_t count,
                                     const float* dL_dscales, const float* dL_dopacities, float* dL_dlog_scales,
                                     float* dL_dlogits, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (count == 0) return PTGS_OK;
  if (!scales || !opacities || !dL_dscales || !dL_dopacities || !dL_dlog_scales || !dL_dlogits)
    return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(dL_dlog_scales) || !is_device_ptr(dL_dlogits))
    return fail(c, PTGS_EINVAL, "dL_dlog_scales / dL_dlogits must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_sh_activate_backward(scales, opacities, count, dL_dscales, dL_dopacities, dL_dlog_scales,
                                                  dL_dlogits, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_activate_backward");
}

int ptgs_gaussians_permute_sh(ptgs_ctx* c, const float* sh, uint32_t sh_degree, const uint32_t* ids, uint32_t count,
                              float* out, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (sh_degree > 3) return fail(c, PTGS_EINVAL, "sh_degree %u above 3", sh_degree);
  if (count == 0) return PTGS_OK;
  if (!sh || !ids || !out) return fail(c, PTGS_EINVAL, "null argument");
  if (out == sh) return fail(c, PTGS_EINVAL, "out must not alias sh");
  if (!is_device_ptr(sh) || !is_device_ptr(ids) || !is_device_ptr(out))
    return fail(c, PTGS_EINVAL, "sh / ids / out must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_sh_permute(sh, sh_degree, ids, count, out, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_permute_sh");
}

// ptgs_splat_gaussians_backward (depth == false: dL_dinvdepth is not looked at), _backward_depth and
// _backward_pose (pose: dL_dview is written as well; a null or non-device dL_dview is refused before
// anything is enqueued, and an empty set of Gaussians gives sixteen zeros)
static int splat_backward_call(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                               const float bg[3], const float* dL_dout, bool depth, const float* dL_dinvdepth,
                               const ptgs_gaussian_grads* grads, void* stream, const char* name, bool pose = false,
                               float* dL_dview = nullptr) {
  if (!c) return PTGS_EINVAL;
  if (!g || !ubo || !bg || !dL_dout || !grads || (depth && !dL_dinvdepth)) return fail(c, PTGS_EINVAL, "null argument");
  if (pose && !dL_dview) return fail(c, PTGS_EINVAL, "null argument (dL_dview)");
  if (g->ids) return fail(c, PTGS_EINVAL, "the backward pass takes the Gaussians in their original order (ids must be NULL)");
  if (pose && !is_device_ptr(dL_dview)) return fail(c, PTGS_EINVAL, "dL_dview must be a device pointer");
  if (g->count == 0) {  // (empty arrays may be null)
    if (!pose) return PTGS_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return hip_rc(c, splat_pose_finish(nullptr, 0, dL_dview, (hipStream_t)stream), name);
  }
  if (!g->means || !g->scales || !g->rotations || !g->opacities || !g->colors)
    return fail(c, PTGS_EINVAL, "null gaussian array");
  if (!grads->means || !grads->scales || !grads->rotations || !grads->opacities || !grads->colors)
    return fail(c, PTGS_EINVAL, "null gradient array (means2d and conics alone are optional)");
  if (!is_device_ptr(dL_dout) || !is_device_ptr(grads->means))
    return fail(c, PTGS_EINVAL, "dL_dout / gradient arrays must be device pointers");
  if (depth && !is_device_ptr(dL_dinvdepth)) return fail(c, PTGS_EINVAL, "dL_dinvdepth must be a device pointer");
  if (ubo->proj[0] == 0.0f || ubo->proj[5] == 0.0f) return fail(c, PTGS_EINVAL, "degenerate projection");
  SplatFrame f;
  splat_last_frame(c->frames.current(), &f);
  if (!f.valid)
    return fail(c, PTGS_EINVAL,
                "no frame to differentiate: the latest splat call must be a full-frame ptgs_splat_gaussians with "
                "PTGS_FLAG_SPLAT_PUBLISH and stats");
  if (f.n != g->count || f.W != w || f.H != h)
    return fail(c, PTGS_EINVAL, "the latest frame has %u gaussians at %ux%u, the backward call %u at %ux%u", f.n, f.W,
                f.H, g->count, w, h);
  HIPCHK(c, hipSetDevice(c->device));
  float* acc = nullptr;
  float* partials = nullptr;
  HIPCHK(c, splat_backward_scratch(c->frames.current(), f.n, depth ? GS_BWD_ACC_DEPTH : GS_BWD_ACC, &acc));
  if (pose) HIPCHK(c, splat_backward_pose_scratch(c->frames.current(), f.n, &partials));
  float mvp[16];
  mat4_mul(ubo->proj, ubo->view, mvp);
  const hipError_t e = splat_gaussians_backward(f, acc, g, ubo->view, mvp, ubo->proj[0], ubo->proj[5], bg, dL_dout,
                                                depth ? dL_dinvdepth : nullptr, grads, (hipStream_t)stream,
                                                ubo->proj, partials, pose ? dL_dview : nullptr);
  return hip_rc(c, e, name);
}

int ptgs_splat_gaussians_backward(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w, uint32_t h,
                                  const float bg[3], const float* dL_dout, const ptgs_gaussian_grads* grads,
                                  void* stream) {
  return splat_backward_call(c, g, ubo, w, h, bg, dL_dout, false, nullptr, grads, stream, "ptgs_splat_gaussians_backward");
}

int ptgs_splat_gaussians_backward_depth(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w,
                                        uint32_t h, const float bg[3], const float* dL_dout, const float* dL_dinvdepth,
                                        const ptgs_gaussian_grads* grads, void* stream) {
  return splat_backward_call(c, g, ubo, w, h, bg, dL_dout, true, dL_dinvdepth, grads, stream,
                             "ptgs_splat_gaussians_backward_depth");
}

int ptgs_splat_gaussians_backward_pose(ptgs_ctx* c, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t w,
                                       uint32_t h, const float bg[3], const float* dL_dout, const float* dL_dinvdepth,
                                       const ptgs_gaussian_grads* grads, float* dL_dview, void* stream) {
  return splat_backward_call(c, g, ubo, w, h, bg, dL_dout, dL_dinvdepth != nullptr, dL_dinvdepth, grads, stream,
                             "ptgs_splat_gaussians_backward_pose", true, dL_dview);
}

int ptgs_splat_gaussians_invdepth(ptgs_ctx* c, uint32_t w, uint32_t h, float* out_invdepth, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!out_invdepth) return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(out_invdepth)) return fail(c, PTGS_EINVAL, "out_invdepth must be a device pointer");
  SplatFrame f;
  splat_last_frame(c->frames.current(), &f);
  if (!f.valid)
    return fail(c, PTGS_EINVAL,
                "no frame to render the inverse depth of: the latest splat call must be a full-frame "
                "ptgs_splat_gaussians with PTGS_FLAG_SPLAT_PUBLISH and stats");
  if (f.W != w || f.H != h)
    return fail(c, PTGS_EINVAL, "the latest frame is %ux%u, the inverse-depth call %ux%u", f.W, f.H, w, h);
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = splat_gaussians_invdepth(f, out_invdepth, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_splat_gaussians_invdepth");
}

// An array of a call as a byte range (densify apply, Adam step); out: the call writes it.
struct Span {
  const char* p;
  size_t bytes;
  bool out;
};

// does the written span i overlap another span? (two written spans are compared once, from the earlier one)
static bool span_overlaps(const Span* sp, uint32_t ns, uint32_t i) {
  for (uint32_t j = 0; j < ns; ++j)
    if (j != i && (j > i || !sp[j].out) && sp[i].p < sp[j].p + sp[j].bytes && sp[j].p < sp[i].p + sp[i].bytes) return true;
  return false;
}

int ptgs_densify_accumulate(ptgs_ctx* c, const float* g2d, const int32_t* radii, uint32_t n, uint32_t w, uint32_t h,
                            float* accum, float* denom, float* max_radii, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (n == 0) return PTGS_OK;  // (empty arrays may be null)
  if (!g2d || !radii || !accum || !denom || !max_radii) return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(accum) || !is_device_ptr(denom) || !is_device_ptr(max_radii))
    return fail(c, PTGS_EINVAL, "accum / denom / max_radii must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = densify_accumulate(g2d, radii, n, w, h, accum, denom, max_radii, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_densify_accumulate");
}

int ptgs_gaussians_densify_plan(ptgs_ctx* c, const float* scales, const float* opacities, const float* accum,
                                const float* denom, const float* max_radii, uint32_t n,
                                const ptgs_densify_params* params, ptgs_densify_counts* out, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!params || !out) return fail(c, PTGS_EINVAL, "null argument");
  *out = ptgs_densify_counts{};
  if (n == 0) {  // (empty arrays may be null)
    densify_plan_empty(c->densify);
    return PTGS_OK;
  }
  if (!scales || !opacities || !accum || !denom || !max_radii) return fail(c, PTGS_EINVAL, "null argument");
  if (n > (1u << 30))
    return fail(c, PTGS_EINVAL, "%u gaussians: the source map holds indices below 2^30 beside the kind", n);
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = densify_plan(c->densify, scales, opacities, accum, denom, max_radii, n, *params, out,
                                    (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_densify_plan");
}

int ptgs_gaussians_densify_apply(ptgs_ctx* c, uint32_t n, uint32_t n_out, const float* means, const float* log_scales,
                                 const float* rotations, const float* scales, const float* noise, float* means_out,
                                 float* log_scales_out, const ptgs_densify_rows* rows, uint32_t n_rows,
                                 uint32_t* source_out, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (n_rows > PTGS_DENSIFY_MAX_ROWS)
    return fail(c, PTGS_EINVAL, "n_rows %u above %d", n_rows, PTGS_DENSIFY_MAX_ROWS);
  if (n_rows && !rows) return fail(c, PTGS_EINVAL, "null argument");
  uint32_t pn = 0, pn_out = 0;
  if (!densify_last_plan(c->densify, &pn, &pn_out))
    return fail(c, PTGS_EINVAL, "no plan: ptgs_gaussians_densify_plan must come first");
  if (pn != n || pn_out != n_out)
    return fail(c, PTGS_EINVAL, "the latest plan takes %u gaussians to %u, the apply call %u to %u", pn, pn_out, n,
                n_out);
  for (uint32_t k = 0; k < n_rows; ++k)
    if (rows[k].width == 0) return fail(c, PTGS_EINVAL, "rows[%u] has width 0", k);
  if (n_out == 0) return PTGS_OK;  // everything pruned (or n == 0): nothing to write
  if (!means || !log_scales || !rotations || !scales || !noise || !means_out || !log_scales_out)
    return fail(c, PTGS_EINVAL, "null argument");
  // every input and output as a byte range: an output may overlap nothing else
  Span sp[7 + 2 * PTGS_DENSIFY_MAX_ROWS + 1];
  uint32_t ns = 0;
  auto span = [&](const void* p, size_t count, size_t width, bool out) {
    sp[ns++] = Span{(const char*)p, count * width * sizeof(float), out};
  };
  span(means, n, 3, false);
  span(log_scales, n, 3, false);
  span(rotations, n, 4, false);
  span(scales, n, 3, false);
  span(noise, (size_t)n * 2, 3, false);
  span(means_out, n_out, 3, true);
  span(log_scales_out, n_out, 3, true);
  for (uint32_t k = 0; k < n_rows; ++k) {
    if (!rows[k].src || !rows[k].dst) return fail(c, PTGS_EINVAL, "rows[%u] has a null src / dst", k);
    span(rows[k].src, n, rows[k].width, false);
    span(rows[k].dst, n_out, rows[k].width, true);
  }
  if (source_out) span(source_out, n_out, 1, true);
  for (uint32_t i = 0; i < ns; ++i) {
    if (!sp[i].out) continue;
    if (span_overlaps(sp, ns, i))
      return fail(c, PTGS_EINVAL, "an output aliases an input or another output (every dst differs from every src)");
    if (!is_device_ptr(sp[i].p)) return fail(c, PTGS_EINVAL, "an output is not a device pointer");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = densify_apply(c->densify, means, log_scales, rotations, scales, noise, means_out, log_scales_out,
                                     rows, n_rows, source_out, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(c, PTGS_ERANGE, "ptgs_gaussians_densify_apply: more elements than one launch holds");
  return hip_rc(c, e, "ptgs_gaussians_densify_apply");
}

int ptgs_image_loss_l1_dssim(ptgs_ctx* c, const float* image, const float* target, uint32_t target_channels,
                             uint32_t w, uint32_t h, float lambda, float grad_scale, float* loss_out,
                             float* dL_dimage, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!image || !target || !loss_out) return fail(c, PTGS_EINVAL, "null argument");
  if (w == 0 || h == 0 || w > LOSS_MAX_SIDE || h > LOSS_MAX_SIDE)
    return fail(c, PTGS_EINVAL, "image of %u x %u: each side is 1 .. %u", w, h, LOSS_MAX_SIDE);
  if (target_channels != 3 && target_channels != 4)
    return fail(c, PTGS_EINVAL, "target_channels %u: 3 or 4", target_channels);
  if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(c, PTGS_EINVAL, "lambda must be in [0, 1]");
  if (!std::isfinite(grad_scale)) return fail(c, PTGS_EINVAL, "grad_scale must be finite");
  const size_t pixels = (size_t)w * h;
  if (dL_dimage) {
    const char *g = (const char*)dL_dimage, *a = (const char*)image, *b = (const char*)target;
    const size_t gb = pixels * 4 * sizeof(float), bb = pixels * target_channels * sizeof(float);
    if ((g < a + gb && a < g + gb) || (g < b + bb && b < g + gb))
      return fail(c, PTGS_EINVAL, "dL_dimage overlaps image or target");
    if (!is_device_ptr(dL_dimage)) return fail(c, PTGS_EINVAL, "dL_dimage is not a device pointer");
  }
  if (!is_device_ptr(loss_out)) return fail(c, PTGS_EINVAL, "loss_out is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = image_loss_l1_dssim(c->loss, image, target, target_channels, w, h, lambda, grad_scale, loss_out,
                                           dL_dimage, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_image_loss_l1_dssim");
}

int ptgs_image_loss_invdepth_l1(ptgs_ctx* c, const float* invdepth, const float* target_depth, uint32_t w, uint32_t h,
                                float weight, float grad_scale, float* terms, float* dL_dinvdepth, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!invdepth || !target_depth || !terms) return fail(c, PTGS_EINVAL, "null argument");
  if (w == 0 || h == 0 || w > LOSS_MAX_SIDE || h > LOSS_MAX_SIDE)
    return fail(c, PTGS_EINVAL, "map of %u x %u: each side is 1 .. %u", w, h, LOSS_MAX_SIDE);
  if (!std::isfinite(weight)) return fail(c, PTGS_EINVAL, "weight must be finite");
  if (!std::isfinite(grad_scale)) return fail(c, PTGS_EINVAL, "grad_scale must be finite");
  if (dL_dinvdepth) {
    const char *g = (const char*)dL_dinvdepth, *a = (const char*)invdepth, *b = (const char*)target_depth;
    const size_t bytes = (size_t)w * h * sizeof(float);
    if ((g < a + bytes && a < g + bytes) || (g < b + bytes && b < g + bytes))
      return fail(c, PTGS_EINVAL, "dL_dinvdepth overlaps invdepth or target_depth");
    if (!is_device_ptr(dL_dinvdepth)) return fail(c, PTGS_EINVAL, "dL_dinvdepth is not a device pointer");
  }
  if (!is_device_ptr(invdepth) || !is_device_ptr(target_depth))
    return fail(c, PTGS_EINVAL, "invdepth / target_depth must be device pointers");
  if (!is_device_ptr(terms)) return fail(c, PTGS_EINVAL, "terms is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = image_loss_invdepth_l1(c->loss, invdepth, target_depth, w, h, weight, grad_scale, terms,
                                              dL_dinvdepth, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_image_loss_invdepth_l1");
}

int ptgs_gaussians_adam_step(ptgs_ctx* c, uint32_t n, const ptgs_adam_rows* rows, uint32_t n_rows,
                             const ptgs_adam_params* params, const int32_t* radii, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!rows || !params) return fail(c, PTGS_EINVAL, "null argument");
  if (n_rows == 0 || n_rows > PTGS_ADAM_MAX_ROWS)
    return fail(c, PTGS_EINVAL, "n_rows %u: 1 .. %d", n_rows, PTGS_ADAM_MAX_ROWS);
  if (params->step == 0) return fail(c, PTGS_EINVAL, "step 0: the first step is 1");
  if (!(params->beta1 >= 0.0f && params->beta1 < 1.0f) || !(params->beta2 >= 0.0f && params->beta2 < 1.0f))
    return fail(c, PTGS_EINVAL, "beta1 and beta2 must be in [0, 1)");
  if (!(params->eps >= 0.0f) || !std::isfinite(params->eps)) return fail(c, PTGS_EINVAL, "eps must be finite and >= 0");
  for (uint32_t k = 0; k < n_rows; ++k) {
    if (rows[k].width == 0) return fail(c, PTGS_EINVAL, "rows[%u] has width 0", k);
    if (rows[k].head > rows[k].width)
      return fail(c, PTGS_EINVAL, "rows[%u] has head %u above its width %u", k, rows[k].head, rows[k].width);
    if (!std::isfinite(rows[k].lr) || !std::isfinite(rows[k].lr_head))
      return fail(c, PTGS_EINVAL, "rows[%u] has an lr / lr_head that is not finite", k);
  }
  if (n == 0) return PTGS_OK;  // (empty arrays may be null)
  // every array as a byte range: a written one may overlap nothing else
  Span sp[4 * PTGS_ADAM_MAX_ROWS + 1];
  uint32_t ns = 0;
  for (uint32_t k = 0; k < n_rows; ++k) {
    const ptgs_adam_rows& r = rows[k];
    if (!r.param || !r.grad || !r.exp_avg || !r.exp_avg_sq)
      return fail(c, PTGS_EINVAL, "rows[%u] has a null param / grad / exp_avg / exp_avg_sq", k);
    const size_t bytes = (size_t)n * r.width * sizeof(float);
    sp[ns++] = Span{(const char*)r.param, bytes, true};
    sp[ns++] = Span{(const char*)r.grad, bytes, false};
    sp[ns++] = Span{(const char*)r.exp_avg, bytes, true};
    sp[ns++] = Span{(const char*)r.exp_avg_sq, bytes, true};
  }
  if (radii) sp[ns++] = Span{(const char*)radii, (size_t)n * sizeof(int32_t), false};
  for (uint32_t i = 0; i < ns; ++i) {
    if (!sp[i].out) continue;
    if (span_overlaps(sp, ns, i))
      return fail(c, PTGS_EINVAL, "a written array (param, exp_avg, exp_avg_sq) overlaps another array of the call");
    if (!is_device_ptr(sp[i].p)) return fail(c, PTGS_EINVAL, "a written array is not a device pointer");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = adam_step(n, rows, n_rows, *params, radii, (hipStream_t)stream);
  if (e == hipErrorInvalidValue) return fail(c, PTGS_ERANGE, "ptgs_gaussians_adam_step: more elements than one launch holds");
  return hip_rc(c, e, "ptgs_gaussians_adam_step");
}

int ptgs_gaussians_opacity_reset(ptgs_ctx* c, float* logits, uint32_t n, float max_opacity, float* exp_avg,
                                 float* exp_avg_sq, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (!(max_opacity > 0.0f && max_opacity < 1.0f)) return fail(c, PTGS_EINVAL, "max_opacity must be in (0, 1)");
  if (n == 0) return PTGS_OK;  // (empty arrays may be null)
  if (!logits) return fail(c, PTGS_EINVAL, "null argument");
  const char* a[3] = {(const char*)logits, (const char*)exp_avg, (const char*)exp_avg_sq};
  const size_t bytes = (size_t)n * sizeof(float);
  for (int i = 0; i < 3; ++i) {
    if (!a[i]) continue;
    for (int j = i + 1; j < 3; ++j)
      if (a[j] && a[i] < a[j] + bytes && a[j] < a[i] + bytes)
        return fail(c, PTGS_EINVAL, "opacity_logits, exp_avg and exp_avg_sq overlap");
    if (!is_device_ptr(a[i])) return fail(c, PTGS_EINVAL, "an output is not a device pointer");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = opacity_reset(logits, n, adam_reset_cap(max_opacity), exp_avg, exp_avg_sq, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_opacity_reset");
}

int ptgs_gaussians_checkpoint_init(ptgs_ctx* c, const float* scales, const float* opacities, const float* colors,
                                   uint32_t n, uint32_t sh_degree, float* log_scales, float* opacity_logits, float* sh,
                                   void* stream) {
  if (!c) return PTGS_EINVAL;
  if (sh_degree > 3) return fail(c, PTGS_EINVAL, "sh_degree %u above 3", sh_degree);
  if (n == 0) return PTGS_OK;  // (empty arrays may be null)
  if (!scales || !opacities || !colors || !log_scales || !opacity_logits || !sh)
    return fail(c, PTGS_EINVAL, "null argument");
  // log_scales / opacity_logits may be their own inputs; every other pair of a written array and another array is apart
  const size_t f = sizeof(float), row = 3u * (sh_degree + 1u) * (sh_degree + 1u);
  Span sp[6] = {{(const char*)log_scales, (size_t)n * 3 * f, true}, {(const char*)opacity_logits, (size_t)n * f, true},
                {(const char*)sh, (size_t)n * row * f, true},       {(const char*)scales, (size_t)n * 3 * f, false},
                {(const char*)opacities, (size_t)n * f, false},     {(const char*)colors, (size_t)n * 3 * f, false}};
  for (uint32_t i = 0; i < 3; ++i) {
    for (uint32_t j = 0; j < 6; ++j) {
      if (j == i || (i < 2 && j == i + 3 && sp[j].p == sp[i].p)) continue;  // (sh's rows are not colors' rows)
      if (sp[i].p < sp[j].p + sp[j].bytes && sp[j].p < sp[i].p + sp[i].bytes)
        return fail(c, PTGS_EINVAL, "an output overlaps another array (in place: log_scales == scales, "
                                    "opacity_logits == opacities)");
    }
    if (!is_device_ptr(sp[i].p)) return fail(c, PTGS_EINVAL, "an output is not a device pointer");
  }
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = train_checkpoint_init(scales, opacities, colors, n, sh_degree, log_scales, opacity_logits, sh,
                                             (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_gaussians_checkpoint_init");
}

int ptgs_image_mse(ptgs_ctx* c, const float* image, const float* target, uint32_t target_channels, uint32_t w,
                   uint32_t h, double* out_sum, void* stream) {
  if (!c) return PTGS_EINVAL;
  if (target_channels != 3 && target_channels != 4)
    return fail(c, PTGS_EINVAL, "target_channels %u: 3 or 4", target_channels);
  if ((uint64_t)w * h == 0) return PTGS_OK;  // (an empty image may be null; out_sum is not written)
  if (!image || !target || !out_sum) return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(out_sum)) return fail(c, PTGS_EINVAL, "out_sum is not a device pointer");
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = train_image_mse(image, target, target_channels, (uint64_t)w * h, c->mse_partials.as<double>(),
                                       out_sum, (hipStream_t)stream);
  return hip_rc(c, e, "ptgs_image_mse");
}

int ptgs_splat_status_read(ptgs_ctx* c, ptgs_splat_status* out, void* stream) {
  if (!c || !out) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
  SplatFrames& f = c->frames;
  for (const SplatFrames::View& vw : f.views)
    if (vw.stream) HIPCHK(c, hipStreamSynchronize(vw.stream));
  if (f.fe) HIPCHK(c, hipStreamSynchronize(f.fe));
  *out = ptgs_splat_status{};
  out->pair_capacity = 0xFFFFFFFFu;
  // (slot 0 is the whole ring: the current workspace, then the other ring workspaces of PTGS_FLAG_SPLAT_OVERLAP)
  const hipError_t e = f.for_each_workspace([out](SplatRole role, uint32_t view, SplatWorkspace* ws) {
    SplatStatusOut so;
    if (const hipError_t e = splat_status(ws, true, &so)) return e;
    out->views[view] += so.incomplete;
    out->frames += so.incomplete;
    out->spilled_tiles += so.spilled_tiles;
    out->incomplete_tiles += so.incomplete_tiles;
    if (role != SplatRole::OtherRing || so.last_pairs) out->pair_capacity = std::min(out->pair_capacity, so.capacity);
    // the latest frame's pairs: the current workspace's, else any view's
    if (role != SplatRole::OtherRing) out->last_pairs = std::max(out->last_pairs, so.last_pairs);
    if (role != SplatRole::View) {
      out->spill_capacity =
          role == SplatRole::Current ? so.spill_capacity : std::min(out->spill_capacity, so.spill_capacity);
      out->spill_demand = std::max(out->spill_demand, so.spill_demand);
    }
    return hipSuccess;
  });
  if (e != hipSuccess) return hip_rc(c, e, "splat_status(ws, true, &so)");
  splat_front_end_info(f.current(), &out->touched_runs, &out->fused);
  return PTGS_OK;
}

int ptgs_splat_reserve(ptgs_ctx* c, uint32_t pairs) {
  if (!c) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  const hipError_t e = c->frames.for_each_workspace(
      [pairs](SplatRole, uint32_t, SplatWorkspace* ws) { return splat_reserve(ws, pairs); });
  return hip_rc(c, e, "splat_reserve(ws, pairs)");
}

int ptgs_splat_get_buffers(const ptgs_ctx* c, ptgs_splat_buffers* out) {
  if (!c || !out) return PTGS_EINVAL;
  splat_get_buffers(c->frames.current(), out);
  return PTGS_OK;
}

int ptgs_splat_get_tile_rows(const ptgs_ctx* c, const uint64_t** rows, uint32_t* row_capacity) {
  if (!c || !rows || !row_capacity) return PTGS_EINVAL;
  const unsigned long long* r = nullptr;
  splat_get_tile_rows(c->frames.current(), &r, row_capacity);
  *rows = (const uint64_t*)r;
  return PTGS_OK;
}

int ptgs_splat_stage_ms(ptgs_ctx* c, float out_ms[6]) {
  if (!c || !out_ms) return PTGS_EINVAL;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, splat_stage_ms(c->frames.current(), out_ms));
  return PTGS_OK;
}

int ptgs_splat_points(ptgs_ctx* c, const ptgs_ubo* ubo, const ptgs_ray_push* push, const ptgs_hitdata* hits,
                      const ptgs_ray_sample* samples, uint32_t n, uint32_t w, uint32_t h, uint32_t* rgba8,
                      float* depth, void* stream) {
  if (!c || !ubo || !push || !rgba8 || !depth) return fail(c, PTGS_EINVAL, "null argument");
  if (const int bad = check_image_size(c, w, h)) return bad;
  if (n && (!is_device_ptr(hits) || (push->mode == 1 && !is_device_ptr(samples))))
    return fail(c, PTGS_EINVAL, "hits/samples must be device pointers");
  if (!is_device_ptr(rgba8) || !is_device_ptr(depth)) return fail(c, PTGS_EINVAL, "rgba8/depth must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  float mvp[16];
  mat4_mul(ubo->proj, ubo->view, mvp);
  unsigned long long* keys = nullptr;
  HIPCHK(c, splat_point_keys(c->frames.current(), (size_t)w * h, &keys));
  hipError_t e = launch_splat_points(mvp, push->model, push->major_radius, push->minor_radius, push->height,
                                     push->mode, hits, samples, n, w, h, keys, depth, rgba8, (hipStream_t)stream);
  return hip_rc(c, e, "splat_points");
}

int ptgs_encode_srgb8(ptgs_ctx* c, const float* rgba32f, uint32_t w, uint32_t h, uint32_t* rgba8, void* stream) {
  if (!c || !rgba32f || !rgba8) return fail(c, PTGS_EINVAL, "null argument");
  if (!is_device_ptr(rgba32f) || !is_device_ptr(rgba8)) return fail(c, PTGS_EINVAL, "buffers must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  hipError_t e = launch_encode_srgb8(rgba32f, rgba8, w * h, (hipStream_t)stream);
  return hip_rc(c, e, "encode_srgb8");
}

int ptgs_knn3_mean_dist2(ptgs_ctx* c, const float* xyz, uint32_t n, float* dist2, void* stream) {
  if (!c || (n && (!xyz || !dist2))) return fail(c, PTGS_EINVAL, "null argument");
  if (n == 0) return PTGS_OK;
  if (!is_device_ptr(xyz) || !is_device_ptr(dist2)) return fail(c, PTGS_EINVAL, "buffers must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  hipError_t e = ptgs::knn3_mean_dist2(xyz, n, dist2, (hipStream_t)stream, nullptr);
  return hip_rc(c, e, "knn3_mean_dist2");
}

int ptgs_gaussians_from_points(ptgs_ctx* c, const float* xyz, const uint8_t* rgb, uint32_t n, float* means,
                               float* scales, float* rotations, float* opacities, float* colors, void* stream) {
  if (!c || (n && (!xyz || !means || !scales || !rotations || !opacities || !colors)))
    return fail(c, PTGS_EINVAL, "null argument");
  if (n == 0) return PTGS_OK;
  const void* ptrs[] = {xyz, means, scales, rotations, opacities, colors};
  for (const void* p : ptrs)
    if (!is_device_ptr(p)) return fail(c, PTGS_EINVAL, "buffers must be device pointers");
  if (rgb && !is_device_ptr(rgb)) return fail(c, PTGS_EINVAL, "buffers must be device pointers");
  HIPCHK(c, hipSetDevice(c->device));
  hipError_t e = ptgs::gaussians_from_points(xyz, rgb, n, means, scales, rotations, opacities, colors,
                                             (hipStream_t)stream);
  return hip_rc(c, e, "gaussians_from_points");
}

}  // extern "C"
