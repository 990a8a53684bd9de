/*
 * ptgs.h — C-ABI of the MI355X-native path tracer / Gaussian-splat renderer.
 *
 * This is the drop-in boundary for the two data-parallel hot paths of
 * FedericoCos/PathTracer_GaussianSplatting (reference tree: /root/reference, read-only).
 * The reference has no FFI; its hot path sits behind the Vulkan RT pipeline:
 *   - descriptor set bindings 0-14           Vulkan_Engine/engine.cpp:2169-2224, shaders/rt_render/raytracing.glsl:109-138
 *   - push constant RayPushConstant (80 B)   Helpers/GeneralHeaders.h:526-532
 *   - launch vkCmdTraceRaysKHR(W, H, 1)      Vulkan_Engine/engine.cpp:1971-1976 (camera), :2789 (torus)
 *   - per-frame protocol ubo.frame_count     Vulkan_Engine/engine.cpp:2134, :2070-2072
 * Every struct below is byte-compatible with Helpers/GeneralHeaders.h so the reference's
 * Engine can hand its host arrays straight to ptgs_scene_upload() and replace
 * vkCmdTraceRaysKHR + the running-mean image with ptgs_trace_camera().
 *
 * Conventions:
 *   - every entry point returns 0 (PTGS_OK) or a negative PTGS_E* code; no exceptions cross the ABI,
 *     nothing aborts; ptgs_last_error() returns a message for the last failure on a context.
 *   - compute entry points are stream-ordered (hipStream_t passed as void*); the caller synchronises.
 *   - "device pointer" arguments must be device-accessible memory of the context's HIP device.
 *   - a context is not thread-safe (thread-compatible): one host thread at a time per context.
 *   - a context owns device scratch its calls reuse (the splat workspace; the path tracer's tile
 *     schedule: per-tile times of the last ptgs_trace_camera launch and the order built from them):
 *     calls of one context on different streams must be ordered by the caller (events), or use one
 *     context per stream (ptgs_splat_gaussians_views has its own per-view workspaces).
 */
#ifndef PTGS_H_
#define PTGS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTGS_ABI_VERSION 4  /* 3: ptgs_gaussians.ids, ptgs_splat_stats.fused, ptgs_splat_status spill fields;
                             * 4: PTGS_EBADIDS, PTGS_FLAG_SPLAT_OVERLAP. Added since, without a version
                             * change (new functions only): ptgs_gaussians_sh_colors, ptgs_gaussians_activate,
                             * ptgs_gaussians_permute_sh, ptgs_splat_gaussians_backward (with the struct
                             * ptgs_gaussian_grads), ptgs_gaussians_sh_colors_backward,
                             * ptgs_gaussians_activate_backward, ptgs_densify_accumulate,
                             * ptgs_gaussians_densify_plan, ptgs_gaussians_densify_apply (with their three
                             * structs), ptgs_image_loss_l1_dssim, ptgs_gaussians_adam_step,
                             * ptgs_gaussians_opacity_reset (with the structs ptgs_adam_rows and
                             * ptgs_adam_params), ptgs_splat_gaussians_invdepth,
                             * ptgs_splat_gaussians_backward_depth, ptgs_image_loss_invdepth_l1,
                             * ptgs_splat_gaussians_backward_pose, ptgs_gaussians_sh_colors_backward_eye,
                             * ptgs_gaussians_checkpoint_init, ptgs_image_mse; ptgs_read_gaussian_ply and
                             * ptgs_write_gaussian_ply in ptgs_host.h */

/* ---------------- error codes ---------------- */
#define PTGS_OK 0
#define PTGS_EINVAL (-1)   /* bad argument / null pointer / size mismatch */
#define PTGS_EHIP (-2)     /* HIP runtime error (allocation, launch, copy) */
#define PTGS_ENOSCENE (-3) /* trace before ptgs_scene_upload */
#define PTGS_ERANGE (-4)   /* size exceeds an implementation limit */
#define PTGS_EIO (-5)      /* file could not be read/parsed (host helpers) */
#define PTGS_EINCOMPLETE (-6) /* an EARLIER stream-ordered splat frame of this context could not be completed
                               * (its spill pool was exhausted: some tiles were left at the background).
                               * Returned once, by the first splat call that starts after that frame has
                               * finished on the device; that call has grown the pool to 1.25x the largest
                               * pair count any frame of the workspace has had (which bounds the reported
                               * frame's spilled pairs) and
                               * rendered its own frame completely unless its own spilled tiles need more.
                               * ptgs_splat_gaussians_views renders every view before it returns the code.
                               * ptgs_splat_reserve prevents it (see there). */
#define PTGS_EBADIDS (-7) /* an EARLIER stream-ordered splat frame of this context met ptgs_gaussians.ids
                           * entries >= count (those Gaussians were dropped). Returned once, like
                           * PTGS_EINCOMPLETE, by a call that has rendered its own frame; a code of its
                           * own so a caller can tell it from this call's PTGS_EINVAL.
                           * Order of the reports: a call returns one code. When earlier frames left both
                           * reports (one frame may: ids >= count and an exhausted pool), the first call
                           * after them returns PTGS_EBADIDS, the call after that PTGS_EINCOMPLETE, the
                           * third PTGS_OK; each of the two has rendered its own frame completely. A
                           * call that fails for a reason of its own (PTGS_EINVAL, PTGS_EHIP) returns
                           * that code and leaves the reports to the calls after it. */

/* ---------------- reference struct layouts (Appendix B of SURVEY.md) ---------------- */

/* Vertex, GeneralHeaders.h:65-97 / InputVertex raytracing.glsl:7-17 — 80 B */
typedef struct ptgs_vertex {
    float pos[3];
    float pad1;
    float normal[3];
    float pad2;
    float color[3];
    float pad3;
    float tangent[4];
    float tex_coord[2];
    float tex_coord_1[2];
} ptgs_vertex;

/* MaterialPushConstant, GeneralHeaders.h:236-269 / MaterialData raytracing.glsl:20-45 — 308 B.
 * use_specular_glossiness_workflow is a float on the host but read as an int by the shaders
 * (SURVEY Appendix A.2); the kernels reproduce that bit-pun. */
typedef struct ptgs_material {
    float base_color_factor[4];
    float uv_normal[16];
    float uv_emissive[16];
    float uv_albedo[16];
    float emissive_factor_and_pad[4];
    float metallic_factor;
    float roughness_factor;
    float occlusion_strength;
    float specular_factor;
    float specular_color_factor[3];
    float alpha_cutoff;
    float transmission_factor;
    float clearcoat_factor;
    float clearcoat_roughness_factor;
    float pad; /* 1.0 = is_transparent (BLEND), engine.cpp:1706 */
    int32_t albedo_texture_index;
    int32_t normal_texture_index;
    int32_t metallic_roughness_texture_index;
    int32_t emissive_texture_index;
    int32_t occlusion_texture_index;
    int32_t clearcoat_texture_index;
    int32_t clearcoat_roughness_texture_index;
    int32_t sg_id;
    float use_specular_glossiness_workflow;
} ptgs_material;

/* UniformBufferObject, GeneralHeaders.h:300-318 (std140) — 192 B */
typedef struct ptgs_ubo {
    float view[16]; /* column-major (glm) */
    float proj[16]; /* column-major, Vulkan ZO, [1][1] negated (camera.cpp:186-187) */
    float camera_pos[3];
    uint32_t frame_count;
    float ambient_light[4]; /* xyz = sky radiance / 2, w = emissive-NEE scale */
    float emissive_flux;
    float punctual_flux;
    float total_flux;
    float p_emissive;
    float fov; /* radians */
    float height;
    float use_lod;
    float lod_factor;
} ptgs_ubo;

/* PunctualLight, GeneralHeaders.h:287-297 — 64 B; type 0 point, 1 directional, 2 spot */
typedef struct ptgs_punctual_light {
    float position[3];
    float intensity;
    float color[3];
    float range;
    float direction[3];
    float outer_cone_cos;
    float inner_cone_cos;
    int32_t type;
    float padding[2];
} ptgs_punctual_light;

/* MeshInfo GeneralHeaders.h:515-520, LightTriangle :594-597, LightCDF :599-603,
 * PunctualLightCDF :605-609 — 16 B each */
typedef struct ptgs_mesh_info {
    uint32_t material_index;
    uint32_t vertex_offset;
    uint32_t index_offset;
    uint32_t _pad1;
} ptgs_mesh_info;

typedef struct ptgs_light_triangle {
    uint32_t v0, v1, v2;
    uint32_t material_index;
} ptgs_light_triangle;

typedef struct ptgs_light_cdf {
    float cumulative_probability;
    uint32_t triangle_index;
    float padding[2];
} ptgs_light_cdf;

typedef struct ptgs_punctual_cdf {
    float cumulative_probability;
    uint32_t light_index;
    float padding[2];
} ptgs_punctual_cdf;

/* HitDataGPU GeneralHeaders.h:565-576 / HitData rt_datacollect/raytracing.glsl:102-108 — 48 B */
typedef struct ptgs_hitdata {
    float pos[3];
    float flag;
    float color[4];
    float normal[3];
    float padding;
} ptgs_hitdata;

/* RaySample GeneralHeaders.h:522-524 — 8 B */
typedef struct ptgs_ray_sample {
    float uv[2];
} ptgs_ray_sample;

/* RayPushConstant / PC GeneralHeaders.h:526-540 — 80 B */
typedef struct ptgs_ray_push {
    float model[16];
    int32_t mode;
    float major_radius;
    float minor_radius;
    float height;
} ptgs_ray_push;

/* Layout contract: every size / offset of the structs above against Helpers/GeneralHeaders.h (glm's
 * vec3 is 12 B, vec4 16 B with no over-alignment on the host: GeneralHeaders.h:65-97 Vertex, :236-269
 * MaterialPushConstant, :287-297 PunctualLight, :300-318 UniformBufferObject, :515-540 MeshInfo /
 * RaySample / RayPushConstant / PC, :565-576 HitDataGPU, :594-609 LightTriangle / LightCDF /
 * PunctualLightCDF). Any translation unit that includes this header (the library's C++ sources, a C
 * caller, tests/native/abi_layout.c) fails to compile on a drift. */
#if defined(__cplusplus)
#define PTGS_LAYOUT_ASSERT(cond, msg) static_assert(cond, msg)
#else
#define PTGS_LAYOUT_ASSERT(cond, msg) _Static_assert(cond, msg)
#endif
#define PTGS_AT(T, f, off) PTGS_LAYOUT_ASSERT(offsetof(T, f) == (off), #T "." #f " at " #off)
PTGS_LAYOUT_ASSERT(sizeof(ptgs_vertex) == 80, "Vertex is 80 B");
PTGS_AT(ptgs_vertex, pos, 0);
PTGS_AT(ptgs_vertex, pad1, 12);
PTGS_AT(ptgs_vertex, normal, 16);
PTGS_AT(ptgs_vertex, pad2, 28);
PTGS_AT(ptgs_vertex, color, 32);
PTGS_AT(ptgs_vertex, pad3, 44);
PTGS_AT(ptgs_vertex, tangent, 48);
PTGS_AT(ptgs_vertex, tex_coord, 64);
PTGS_AT(ptgs_vertex, tex_coord_1, 72);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_material) == 308, "MaterialPushConstant is 308 B");
PTGS_AT(ptgs_material, base_color_factor, 0);
PTGS_AT(ptgs_material, uv_normal, 16);
PTGS_AT(ptgs_material, uv_emissive, 80);
PTGS_AT(ptgs_material, uv_albedo, 144);
PTGS_AT(ptgs_material, emissive_factor_and_pad, 208);
PTGS_AT(ptgs_material, metallic_factor, 224);
PTGS_AT(ptgs_material, roughness_factor, 228);
PTGS_AT(ptgs_material, occlusion_strength, 232);
PTGS_AT(ptgs_material, specular_factor, 236);
PTGS_AT(ptgs_material, specular_color_factor, 240);
PTGS_AT(ptgs_material, alpha_cutoff, 252);
PTGS_AT(ptgs_material, transmission_factor, 256);
PTGS_AT(ptgs_material, clearcoat_factor, 260);
PTGS_AT(ptgs_material, clearcoat_roughness_factor, 264);
PTGS_AT(ptgs_material, pad, 268);
PTGS_AT(ptgs_material, albedo_texture_index, 272);
PTGS_AT(ptgs_material, normal_texture_index, 276);
PTGS_AT(ptgs_material, metallic_roughness_texture_index, 280);
PTGS_AT(ptgs_material, emissive_texture_index, 284);
PTGS_AT(ptgs_material, occlusion_texture_index, 288);
PTGS_AT(ptgs_material, clearcoat_texture_index, 292);
PTGS_AT(ptgs_material, clearcoat_roughness_texture_index, 296);
PTGS_AT(ptgs_material, sg_id, 300);
PTGS_AT(ptgs_material, use_specular_glossiness_workflow, 304);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_ubo) == 192, "UniformBufferObject is 192 B");
PTGS_AT(ptgs_ubo, view, 0);
PTGS_AT(ptgs_ubo, proj, 64);
PTGS_AT(ptgs_ubo, camera_pos, 128);
PTGS_AT(ptgs_ubo, frame_count, 140);
PTGS_AT(ptgs_ubo, ambient_light, 144);
PTGS_AT(ptgs_ubo, emissive_flux, 160);
PTGS_AT(ptgs_ubo, punctual_flux, 164);
PTGS_AT(ptgs_ubo, total_flux, 168);
PTGS_AT(ptgs_ubo, p_emissive, 172);
PTGS_AT(ptgs_ubo, fov, 176);
PTGS_AT(ptgs_ubo, height, 180);
PTGS_AT(ptgs_ubo, use_lod, 184);
PTGS_AT(ptgs_ubo, lod_factor, 188);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_punctual_light) == 64, "PunctualLight is 64 B");
PTGS_AT(ptgs_punctual_light, position, 0);
PTGS_AT(ptgs_punctual_light, intensity, 12);
PTGS_AT(ptgs_punctual_light, color, 16);
PTGS_AT(ptgs_punctual_light, range, 28);
PTGS_AT(ptgs_punctual_light, direction, 32);
PTGS_AT(ptgs_punctual_light, outer_cone_cos, 44);
PTGS_AT(ptgs_punctual_light, inner_cone_cos, 48);
PTGS_AT(ptgs_punctual_light, type, 52);
PTGS_AT(ptgs_punctual_light, padding, 56);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_mesh_info) == 16, "MeshInfo is 16 B");
PTGS_AT(ptgs_mesh_info, material_index, 0);
PTGS_AT(ptgs_mesh_info, vertex_offset, 4);
PTGS_AT(ptgs_mesh_info, index_offset, 8);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_light_triangle) == 16, "LightTriangle is 16 B");
PTGS_AT(ptgs_light_triangle, material_index, 12);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_light_cdf) == 16, "LightCDF is 16 B");
PTGS_AT(ptgs_light_cdf, triangle_index, 4);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_punctual_cdf) == 16, "PunctualLightCDF is 16 B");
PTGS_AT(ptgs_punctual_cdf, light_index, 4);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_hitdata) == 48, "HitDataGPU is 48 B");
PTGS_AT(ptgs_hitdata, pos, 0);
PTGS_AT(ptgs_hitdata, flag, 12);
PTGS_AT(ptgs_hitdata, color, 16);
PTGS_AT(ptgs_hitdata, normal, 32);
PTGS_AT(ptgs_hitdata, padding, 44);
PTGS_LAYOUT_ASSERT(sizeof(ptgs_ray_sample) == 8, "RaySample is 8 B");
PTGS_LAYOUT_ASSERT(sizeof(ptgs_ray_push) == 80, "RayPushConstant / PC is 80 B");
PTGS_AT(ptgs_ray_push, model, 0);
PTGS_AT(ptgs_ray_push, mode, 64);
PTGS_AT(ptgs_ray_push, major_radius, 68);
PTGS_AT(ptgs_ray_push, minor_radius, 72);
PTGS_AT(ptgs_ray_push, height, 76);
#undef PTGS_AT

/* ---------------- scene ---------------- */

/* Host arrays in the reference layouts, as produced by Engine::createGlobalBindlessBuffers
 * (engine.cpp:1658-1860). mesh_index_count[i] is the index count of the primitive behind
 * meshes[i] (Primitive::index_count, used by buildBlas engine.cpp:545-560); the reference keeps
 * it in the BLAS geometry, so it travels beside MeshInfo here. Meshes with fewer than 3
 * indices are skipped exactly like buildBlas does.
 * The context copies everything; the caller keeps ownership. */
/* One texture of global_textures[] (binding 14, raytracing.glsl:138): RGBA8 level 0. The library
 * builds the mip chain as Image::generateMipmaps does (image.cpp:203-290: linear blits, each level
 * max(1, w/2) x max(1, h/2), floor(log2(max(w, h))) + 1 levels, image.cpp:35) and samples it as the
 * reference's sampler does (image.cpp:124-138: linear min/mag/mip filtering, repeat addressing,
 * LOD clamped to the chain). Formats follow Gameobject::scanTextureFormats (gameobject.cpp:284-345):
 * base colour, emissive, spec-gloss and diffuse are sRGB; normal, metal-rough, occlusion, clearcoat
 * and transmission UNORM. Material texture indices index this array (0 = the default white). */
typedef struct ptgs_texture {
    const uint8_t* rgba8; /* width * height * 4 bytes, row-major; row 0 holds v in [0, 1/height) */
    uint32_t width;
    uint32_t height;
    uint32_t srgb;        /* 1 = VK_FORMAT_R8G8B8A8_SRGB, 0 = VK_FORMAT_R8G8B8A8_UNORM */
    uint32_t reserved;
} ptgs_texture;

typedef struct ptgs_scene_desc {
    const ptgs_vertex* vertices;
    uint32_t num_vertices;
    const uint32_t* indices;
    uint32_t num_indices;
    const ptgs_mesh_info* meshes;
    const uint32_t* mesh_index_count;
    uint32_t num_meshes;
    const ptgs_material* materials;
    uint32_t num_materials;
    const ptgs_light_triangle* light_triangles;
    uint32_t num_light_triangles;
    const ptgs_light_cdf* light_cdf;
    uint32_t num_light_cdf;
    const ptgs_punctual_light* punctual_lights;
    uint32_t num_punctual_lights;
    const ptgs_punctual_cdf* punctual_cdf;
    uint32_t num_punctual_cdf;
    /* blue-noise texture (binding 12): RGBA32F, size x size texels, size a power of two,
     * values already decoded with the stbi_loadf convention (RGB^2.2, A linear). */
    const float* blue_noise_rgba32f;
    uint32_t blue_noise_size;
    /* textures (binding 14); may be empty: every texture index then samples as white */
    const ptgs_texture* textures;
    uint32_t num_textures;
} ptgs_scene_desc;

typedef struct ptgs_scene_info {
    uint32_t num_triangles;   /* triangles in the acceleration structure */
    uint32_t num_bvh_nodes;   /* interior nodes (each holds two child boxes) */
    uint32_t bvh_depth;       /* max depth of the tree */
    uint32_t max_leaf_size;
    double build_ms;          /* host BVH build time */
    uint64_t device_bytes;    /* bytes resident on the device for the scene */
} ptgs_scene_info;

/* ---------------- context ---------------- */

typedef struct ptgs_ctx ptgs_ctx;

int ptgs_create(int hip_device, ptgs_ctx** out);
void ptgs_destroy(ptgs_ctx* ctx);
const char* ptgs_last_error(const ptgs_ctx* ctx);
int ptgs_abi_version(void);
/* device the library was compiled for, e.g. "gfx950" */
const char* ptgs_device_arch(void);

/* Replaces buildBlas/initStaticTlas (engine.cpp:534-655, :1385-1520) + the descriptor uploads. */
int ptgs_scene_upload(ptgs_ctx* ctx, const ptgs_scene_desc* desc);
int ptgs_scene_get_info(const ptgs_ctx* ctx, ptgs_scene_info* out);
/* Debug / parity access to the uploaded acceleration structure (device pointers owned by the
 * context, valid until the next upload): 4-wide nodes (bvh.h layout, 128 B each) and the triangle
 * records in leaf order (48 B each: (v0, mesh) (v1 - v0, prim) (v2 - v0, gid)). */
typedef struct ptgs_bvh_buffers {
    const float* nodes;
    uint32_t num_nodes;
    const float* triangles;
    uint32_t num_triangles;
} ptgs_bvh_buffers;
int ptgs_scene_get_bvh(const ptgs_ctx* ctx, ptgs_bvh_buffers* out);
/* Which builder produced the resident tree. With PTGS_FLAG_GPU_BVH the upload falls back to the host
 * build for scenes under 16 triangles and when the GPU build or collapse does not fit its budgets;
 * `builder` tells the two apart (ptgs_scene_info is the same either way). */
#define PTGS_BUILDER_HOST_SAH 0u
#define PTGS_BUILDER_GPU_SAH 1u
#define PTGS_BUILDER_GPU_LBVH 2u
typedef struct ptgs_scene_build {
    uint32_t builder;       /* PTGS_BUILDER_*: the one whose tree is resident */
    uint32_t leaf, fan;     /* the (leaf size, fan-out) try that was kept (leaf 0 for the LBVH) */
    uint32_t depth_budget;  /* that try's depth budget */
    uint32_t stack_need;    /* worst-case traversal stack entries of the resident tree */
    uint32_t deep_stack;    /* 1 when the deep-stack kernel is launched for it */
} ptgs_scene_build;
int ptgs_scene_get_build(const ptgs_ctx* ctx, ptgs_scene_build* out);
/* The path-tracer megakernel walks a compact copy of the resident tree whose topology is its own: for the
 * two SAH builders' trees it is rebuilt by reinsertion for fewer node steps per ray (hits do not depend on the
 * tree); PTGS_PT_TREE_OPT=0 / 1 in the environment at upload forces that off / on. ptgs_scene_get_bvh,
 * ptgs_scene_info and ptgs_scene_build describe the canonical tree either way; this describes the copy. */
typedef struct ptgs_scene_tree_opt {
    uint32_t applied;       /* 1: the megakernel walks the optimised copy; 0: the canonical tree's conversion */
    uint32_t num_nodes;     /* the optimised copy's 4-wide nodes, worst-case stack entries and depth */
    uint32_t stack_need;    /*   (0 when not applied) */
    uint32_t depth;
    uint32_t fan;           /* the fan-out it was collapsed at */
    uint32_t passes;        /* reinsertion passes run */
    double area_before;     /* sum of the 4-wide nodes' box areas over the root's: canonical, */
    double area_after;      /*   and optimised (0 when not applied) */
    double ms;              /* host time the optimiser took at upload */
} ptgs_scene_tree_opt;
int ptgs_scene_get_tree_opt(const ptgs_ctx* ctx, ptgs_scene_tree_opt* out);
/* The megakernel's traversal stack for the resident scene (each pointer may be NULL): the entries it keeps in
 * LDS per lane, the worst-case stack entries of the copy it walks (optimised or not), and 1 when that need
 * reaches the LDS depth, so that the instantiation with the private overflow is launched. ptgs_scene_build's
 * deep_stack says the same of the canonical tree and the kernels that walk it (torus, depth, wavefront). */
int ptgs_scene_get_pt_stack(const ptgs_ctx* ctx, uint32_t* lds_depth, uint32_t* walked_need, uint32_t* deep);

/* ---------------- path tracer (raygen_camera.rgen + closesthit/miss/shadow) ---------------- */

#define PTGS_ACCUM_RUNNING_MEAN 0u /* reference semantics: mix(prev, cur, 1/(frame+1)), restart at frame 0 */
#define PTGS_ACCUM_SUM 1u          /* accum.rgb += radiance, accum.a += 1 (for sample-sharded multi-GPU) */

/* Renders `spp` consecutive samples per pixel, frame counts ubo->frame_count .. +spp-1, into
 * accum (device, W*H RGBA32F, row-major, caller-owned, read-modify-write). One call with spp=1
 * is exactly one vkCmdTraceRaysKHR(W,H,1) of the reference (engine.cpp:1971).
 * `frame_stride` (>=1) spaces the frame counts: sample s uses frame_count + s*frame_stride —
 * the sample-index shard of §8e (rank g of G: frame_count=g, frame_stride=G, mode SUM). */
int ptgs_trace_camera(ptgs_ctx* ctx, const ptgs_ubo* ubo, uint32_t width, uint32_t height,
                      float* accum_rgba32f, uint32_t spp, uint32_t frame_stride, uint32_t accum_mode,
                      void* hip_stream);

/* Same, restricted to pixel rows [row_begin, row_end) — screen-space sharding of a frame. */
int ptgs_trace_camera_rows(ptgs_ctx* ctx, const ptgs_ubo* ubo, uint32_t width, uint32_t height,
                           uint32_t row_begin, uint32_t row_end, float* accum_rgba32f, uint32_t spp,
                           uint32_t frame_stride, uint32_t accum_mode, void* hip_stream);

/* Primary-hit depth for compositing (hybrid C4): per pixel the camera ray of
 * raygen_camera.rgen:25-41 through the pixel centre (no jitter), closest hit (any-hit seed from
 * ubo->frame_count), view-space depth -(view * hit).z; +inf where the ray misses. depth: device
 * float[W*H]. */
int ptgs_trace_depth(ptgs_ctx* ctx, const ptgs_ubo* ubo, uint32_t width, uint32_t height, float* depth,
                     void* hip_stream);
/* The same for pixel rows [row_begin, row_end) only (the tile-row shard of the hybrid frame: each rank
 * traces the depth of its own rows); the other rows of depth are left untouched. */
int ptgs_trace_depth_rows(ptgs_ctx* ctx, const ptgs_ubo* ubo, uint32_t width, uint32_t height, uint32_t row_begin,
                          uint32_t row_end, float* depth, void* hip_stream);

/* Toroidal data-collection tracer (shaders/rt_datacollect/raygen.rgen:31-141): one ray per
 * RaySample (device array, n entries), launch grid side x side with side = ceil(sqrt(n))
 * (engine.cpp:2786), HitData running mean written in place (device array, n entries). */
int ptgs_trace_torus(ptgs_ctx* ctx, const ptgs_ubo* ubo, const ptgs_ray_push* push,
                     const ptgs_ray_sample* samples, uint32_t n, ptgs_hitdata* hits,
                     void* hip_stream);

/* Ray counters of the most recent trace call(s) since the last reset (device-side atomics,
 * read back synchronously). */
typedef struct ptgs_trace_stats {
    uint64_t extension_rays; /* closest-hit traversals (primary + bounces) */
    uint64_t shadow_rays;    /* any-hit traversals (NEE visibility) */
    uint64_t samples;        /* pixel samples completed */
    uint64_t node_visits;    /* child-box tests (only with PTGS_FLAG_COUNT_TRAVERSAL) */
    uint64_t tri_tests;      /* ray-triangle tests (only with PTGS_FLAG_COUNT_TRAVERSAL) */
    uint64_t closest_hits;   /* extension rays that hit a surface (only with PTGS_FLAG_COUNT_TRAVERSAL) */
} ptgs_trace_stats;

#define PTGS_FLAG_COUNT_TRAVERSAL 1u /* instrumented kernels: node / triangle / hit counters */
#define PTGS_FLAG_TIME_STAGES 2u     /* hipEvent timing of the splat pipeline stages */
#define PTGS_FLAG_GPU_BVH 4u         /* ptgs_scene_upload builds the BVH on the GPU: the host builder's
                                      * binned SAH run on the device (the same tree: same node boxes and
                                      * leaf ranges, so the same traversal cost); falls back to the host
                                      * build for inputs it does not handle */
#define PTGS_FLAG_SPLAT_PUBLISH 8u   /* ptgs_splat_gaussians also writes the sorted keys / values of every
                                      * tile (ptgs_splat_get_buffers; parity tests): off in production,
                                      * the blend needs neither */
#define PTGS_FLAG_SPLAT_PUBLISH_TIGHT 64u /* with PTGS_FLAG_SPLAT_PUBLISH (tests): published frames bin each
                                      * Gaussian like the stream-ordered frames do — only to the tiles its
                                      * alpha >= 1/255 box overlaps, not its whole 3-sigma rectangle — so the
                                      * timed path's keys / values / ranges can be compared with the oracle's
                                      * tight mode (oracle_splat_gaussians_tight). Same image either way. */
#define PTGS_FLAG_PT_WAVEFRONT 16u  /* ptgs_trace_camera runs the wavefront path tracer (raygen / extend /
                                      * shade / shadow / accumulate stages over compacted ray queues)
                                      * instead of the one-kernel-per-frame path loop; same image, same
                                      * ray counts */
#define PTGS_FLAG_GPU_LBVH 32u       /* with PTGS_FLAG_GPU_BVH: a linear BVH (Morton order, Karras 2012)
                                      * instead: fastest rebuilds, slower traversal; host fallback when it
                                      * exceeds the traversal stack depth */
#define PTGS_FLAG_SPLAT_OVERLAP 128u /* frames in flight for the splat (the viewer's loop: a new camera per
                                      * call, Gaussians unchanged): the front end of a stream-ordered
                                      * ptgs_splat_gaussians / _over call (no stats, not published, not timed)
                                      * runs on a second stream of the context, concurrently with the blend
                                      * of the previous call, which still runs on hip_stream; the two calls
                                      * use a ring of three workspaces. The blend, i.e. everything written to
                                      * out_rgba32f, stays ordered on hip_stream exactly as without the flag.
                                      * Contract: a run of overlapped calls (the first call with the flag, or
                                      * the first after a splat call without it) starts after the work enqueued
                                      * on hip_stream before it; the front ends of the later calls of the run
                                      * wait only for the earlier frames of their workspaces (on the device),
                                      * so inputs (Gaussians, ids, chunk bounds) written on the stream during a
                                      * run must be followed by one call without this flag — like a Vulkan frame
                                      * in flight, whose resources the application does not touch. Same image,
                                      * keys and counts as without the flag. A call rejected with PTGS_EINVAL
                                      * (with or without the flag) enqueues nothing and is no part of a run: it
                                      * neither ends one nor takes a workspace, and ptgs_splat_get_buffers /
                                      * ptgs_splat_get_tile_rows / ptgs_splat_status_read go on describing the
                                      * latest rendered frame. */
int ptgs_set_flags(ptgs_ctx* ctx, uint32_t flags);
int ptgs_stats_reset(ptgs_ctx* ctx, void* hip_stream);
int ptgs_stats_read(ptgs_ctx* ctx, ptgs_trace_stats* out); /* synchronises the context's device */

/* ---------------- rasterizers ---------------- */

/* Point-cloud view (shaders/pointcloud/pointcloud.vert:44-89 + .frag:1-11; pipeline state
 * pipeline.cpp:29-82): point i with hits[i].flag > 0 is projected by proj*view (mode 0: hit pos,
 * mode 1: torus(u,v) + 0.01 n through push->model), drawn as a 2-px point sprite with depth test
 * LESS against `depth` (device W*H f32, caller clears to 1.0), no blending, colour = linear
 * hits[i].color.rgb encoded to sRGB8 into rgba8 (device W*H u32, R in the low byte). */
int ptgs_splat_points(ptgs_ctx* ctx, const ptgs_ubo* ubo, const ptgs_ray_push* push,
                      const ptgs_hitdata* hits, const ptgs_ray_sample* samples, uint32_t n,
                      uint32_t width, uint32_t height, uint32_t* rgba8_srgb, float* depth,
                      void* hip_stream);

/* 3D Gaussian splatting forward (Kerbl et al. 2023; absent from the reference).
 * SoA device arrays, N Gaussians: means xyz, scales xyz (linear, post-activation),
 * rotations (w,x,y,z) un-normalised, opacities [0,1], colors linear RGB. */
typedef struct ptgs_gaussians {
    const float* means;     /* 3N */
    const float* scales;    /* 3N */
    const float* rotations; /* 4N */
    const float* opacities; /* N  */
    const float* colors;    /* 3N */
    uint32_t count;
    /* NULL, or ids[i] = the caller's index of Gaussian i (u32 N, device): a reordered copy (e.g. from
     * ptgs_gaussians_sort_spatial) then renders exactly like the original order (sorted values, the
     * depth tie rule and the per-Gaussian buffers use the ids). ids must be a permutation of [0, N):
     * a Gaussian whose id is >= N is dropped (never written out of bounds) and the next splat call
     * returns PTGS_EINVAL; duplicate ids are not detected (their keys collide: undefined order) */
    const uint32_t* ids;
    /* NULL, or per chunk of 256 consecutive Gaussians (ptgs_gaussians_chunk_bounds, 8 floats each): a
     * frame restricted to tile rows skips whole chunks whose conservative screen bound misses them,
     * before loading any of their Gaussians (the tile-row shard of several GPUs: each rank preprocesses
     * the chunks that reach its rows instead of all N). Outputs are unchanged. */
    const float* chunk_bounds;
} ptgs_gaussians;

typedef struct ptgs_splat_stats {
    uint32_t num_rendered; /* K = (gaussian, tile) pairs */
    uint32_t tiles_x, tiles_y;
    uint32_t num_visible;  /* not counted: always 0 (count radii > 0 from ptgs_splat_get_buffers) */
    uint32_t fused;        /* 1: the frame ran the single-launch front end (gs_bin_fused_kernel), 0: count +
                            * column scan + scatter */
} ptgs_splat_stats;

/* out_rgba32f (device W*H): rgb = sum c_i a_i T_i + T_final * bg, a = 1 - T_final.
 * Camera = ubo->view / ubo->proj (reference conventions). Tiles 16x16. Rows of tiles
 * [tile_row_begin, tile_row_end) are rendered (full frame: 0, ~0u) — screen-tile sharding of §8e;
 * pixels outside are left untouched.
 * Stream-ordered when stats == NULL: no host synchronisation, so a frame can be captured into and
 * replayed from a hipGraph. PTGS_OK means the frame is rendered completely, whatever the camera did
 * since the previous frame: the (Gaussian, tile) pair buffer of the context's workspace (three-launch
 * front end: 8 pairs per Gaussian or ptgs_splat_reserve's size, grown from the pair counts of earlier
 * frames) and the per-tile rows of the fused front end (sized from an earlier frame's largest tile)
 * are hints: a tile whose pairs did not fit them is gathered again and sorted by its own blend
 * workgroup on the device, in the same launch, through a spill pool (max(2^20, N) pairs, grown from
 * the demand of earlier frames) — same keys, same order, same image (ptgs_splat_status_read counts
 * these spilled tiles). Only a frame whose spilled tiles exceed the spill pool is incomplete: those
 * tiles are left at the background and the next call returns PTGS_EINCOMPLETE (see there);
 * ptgs_splat_reserve(K) rules it out for frames of at most K pairs. Growth frees buffers, which
 * waits for the device and invalidates graphs captured before it (reserve first).
 * stats != NULL: the call waits for the earlier frames and for this frame's pair count; a frame with
 * spilled tiles or above the pair buffer is re-run after growing the buffer (the exact published
 * layout), and stats is filled. */
int ptgs_splat_gaussians(ptgs_ctx* ctx, const ptgs_gaussians* g, const ptgs_ubo* ubo,
                         uint32_t width, uint32_t height, const float bg[3],
                         uint32_t tile_row_begin, uint32_t tile_row_end, float* out_rgba32f,
                         ptgs_splat_stats* stats, void* hip_stream);

/* Several views of the same Gaussians in one call (the capture loop renders views of one scene):
 * view v = ptgs_splat_gaussians(ctx, g, &ubos[v], width, height, bg, 0, ~0u, outs[v], NULL, ...),
 * identical output. Stream-ordered: the views start after the work already on hip_stream, run
 * concurrently on context-owned streams and workspaces (view 0 on hip_stream), and later work on
 * hip_stream waits for all of them. n_views in [1, PTGS_MAX_VIEWS]. Not a replacement of
 * ptgs_splat_gaussians in ptgs_splat_get_buffers: the buffers are view 0's. */
#define PTGS_MAX_VIEWS 8
int ptgs_splat_gaussians_views(ptgs_ctx* ctx, const ptgs_gaussians* g, uint32_t n_views, const ptgs_ubo* ubos,
                               uint32_t width, uint32_t height, const float bg[3], float* const* outs,
                               void* hip_stream);

/* Front end. Once a finished frame of the context's workspace has reported its largest tile, frames
 * run a single-launch front end: per-tile key rows of a fixed capacity (a power of two >= 1.25x that
 * tile, <= 2048 pairs) filled through per-tile atomic reservations, instead of the exact tile
 * segments of count + column scan + scatter (first frame, larger tiles, PTGS_GS_FRONTEND=three).
 * Both give the same keys, values, ranges and image. A tile above its row capacity is completed
 * through the spill pool (above), and the next frame sizes its rows from it.
 *
 * Spatial order: the fused front end reserves one run per (workgroup, touched tile); Gaussians whose
 * neighbours in memory are neighbours in space touch few tiles per workgroup. This writes a copy of
 * g in 3D Morton order of the means (10 bits per axis over the means' bounding box, ties by index)
 * to the caller's device buffers (sizes as g's) and ids[i] = the original index of copy i (g->ids
 * composed when set): render the copy with .ids = ids for output identical to g's. Scene preparation
 * (like ptgs_scene_upload's BVH build): synchronises; device temporaries are freed. */
int ptgs_gaussians_sort_spatial(ptgs_ctx* ctx, const ptgs_gaussians* g, float* means, float* scales, float* rotations,
                                float* opacities, float* colors, uint32_t* ids, void* hip_stream);

/* Bounds of every chunk of 256 consecutive Gaussians of g (device float[8 * ceil(count / 256)]): the
 * box of its means (min x, y, z, then max x, y, z at [4..6]) and its largest scale ([3]); [7] = 0. For
 * ptgs_gaussians.chunk_bounds; useful when chunks are spatially compact (ptgs_gaussians_sort_spatial's
 * order). Recompute after the Gaussians change. Stream-ordered. */
int ptgs_gaussians_chunk_bounds(ptgs_ctx* ctx, const ptgs_gaussians* g, float* bounds, void* hip_stream);

/* Trained 3DGS checkpoints (the point_cloud.ply of Kerbl et al. 2023; ptgs_read_gaussian_ply in
 * ptgs_host.h reads one): view-dependent colour from spherical harmonics, the activations, and the SH
 * rows of a reordered copy. All pointers are device pointers; the calls are stream-ordered, do not
 * synchronise the host and allocate nothing. PTGS_EINVAL: a null context, a degree above 3,
 * active_degree > sh_degree, a null pointer. count == 0 (checked before the array pointers: empty
 * arrays may be null): PTGS_OK, nothing is launched.
 *
 * ptgs_gaussians_sh_colors: colors[3 i..] = max(SH(dir_i) + 0.5, 0) for ptgs_gaussians.colors; call it
 * on the frame's stream before ptgs_splat_gaussians (with PTGS_FLAG_SPLAT_OVERLAP colors is then an
 * input written during a run: see that flag).
 * sh: float[count][(sh_degree+1)^2][3] (coefficient-major, rgb innermost: the trainers' `features`
 * tensor). sh_degree in 0..3 is the STORED degree (row stride); active_degree <= sh_degree is how many
 * bands are evaluated. camera_pos is read by the host during the call.
 * Numerical contract (f32, no FMA, no reassociation: checkable bit for bit like the splat):
 *   d = means[i] - camera_pos; len = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);
 *   (x, y, z) = len > 0 ? d / len : (0, 0, 0)      (a Gaussian at the eye gets its DC colour, not NaN)
 *   per channel, computeColorFromSH of the original rasterizer's forward.cu evaluated left to right
 *   as written there (a*b*s = (a*b)*s, a*b*(e)*s = ((a*b)*(e))*s, sums term by term in index order):
 *   res = C0*sh[0]
 *   degree >= 1: res = res - C1*y*sh[1] + C1*z*sh[2] - C1*x*sh[3]
 *   degree >= 2: res = res + C2[0]*xy*sh[4] + C2[1]*yz*sh[5] + C2[2]*(2*zz - xx - yy)*sh[6]
 *                          + C2[3]*xz*sh[7] + C2[4]*(xx - yy)*sh[8]
 *   degree >= 3: res = res + C3[0]*y*(3*xx - yy)*sh[9] + C3[1]*xy*z*sh[10] + C3[2]*y*(4*zz - xx - yy)*sh[11]
 *                          + C3[3]*z*(2*zz - 3*xx - 3*yy)*sh[12] + C3[4]*x*(4*zz - xx - yy)*sh[13]
 *                          + C3[5]*z*(xx - yy)*sh[14] + C3[6]*x*(3*xx - yy)*sh[15]
 *   color = res + 0.5 < 0 ? 0 : res + 0.5
 *   C0 = 0.28209479177387814, C1 = 0.4886025119029199,
 *   C2 = {1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792,
 *         0.5462742152960396},
 *   C3 = {-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154,
 *         -0.4570457994644658, 1.445305721320277, -0.5900435899266435}, each rounded to f32. */
int ptgs_gaussians_sh_colors(ptgs_ctx* ctx, const float* means, const float* sh, uint32_t count,
                             uint32_t sh_degree, uint32_t active_degree, const float camera_pos[3],
                             float* colors, void* hip_stream);
/* scales = exp(log_scales) (3N), opacities = 1 / (1 + exp(-logits)) (N); in place allowed (scales ==
 * log_scales, opacities == opacity_logits). exp is the renderer's deterministic polynomial (detmath.h
 * expx: exp2 of x * 1.44269504088896341 by a degree-6 polynomial), the opacity 1.0f / (1.0f + expx(-o)).
 * Rotations need no activation: ptgs_gaussians.rotations are un-normalised. */
int ptgs_gaussians_activate(ptgs_ctx* ctx, const float* log_scales, const float* opacity_logits,
                            uint32_t count, float* scales, float* opacities, void* hip_stream);
/* Backward of ptgs_gaussians_sh_colors (training on checkpoint-format parameters): given dL_dcolors (3N,
 * e.g. ptgs_gaussian_grads.colors), dL_dsh (N (sh_degree+1)^2 3, the layout of sh; every element is
 * overwritten; must not alias sh) and, when dL_dmeans != NULL, the colour's dependence on the mean through the
 * view direction ADDED to dL_dmeans (3N: pass the ptgs_gaussian_grads.means that the rasterizer's backward just
 * wrote). means, sh, the degrees and camera_pos are the forward call's. Errors and count == 0 as above (a
 * null means / sh / camera_pos / dL_dcolors / dL_dsh is PTGS_EINVAL; dL_dmeans may be null).
 * Numerical contract (f32, no FMA, the derivative of the contract above with the two selects held fixed):
 *   (x, y, z), len and res are recomputed exactly as in the forward (the same operations in the same order)
 *   dL_dres[c] = (res + 0.5 < 0) ? 0 : dL_dcolors[c]      (the forward's own test, not the stored colour: a
 *                                                           stored 0 does not say which side it came from)
 *   dL_dsh[i][k][c] = f_k * dL_dres[c]   (one multiply), f_k being the factor the forward forms in front of
 *     sh[k]: C0, -(C1*y), C1*z, -(C1*x), C2[0]*xy, C2[1]*yz, C2[2]*(2*zz - xx - yy), ..., C3[6]*x*(3*xx - yy),
 *     each evaluated as written there; k >= (active_degree+1)^2: 0. Checkable bit for bit.
 *   v = dL/d(x, y, z) = sum_c dL_dres[c] * sum_k grad f_k(x, y, z) * sh[k][c]   (the polynomial derivatives)
 *   dL_dmeans[i] += (v - dir * (dir . v)) / len; a Gaussian at the eye (len == 0) adds nothing.
 *   The order of the operations inside v is not part of the contract (f32 throughout: about 1e-7 relative).
 * Each Gaussian's three sums are read, added to and written once by its own work-item: no atomics, so the
 * result is reproducible from run to run. With dL_dmeans == NULL, active_degree == 0 or sh_degree == 0 the
 * colour does not depend on the direction: that part is skipped and dL_dmeans is neither read nor written. */
int ptgs_gaussians_sh_colors_backward(ptgs_ctx* ctx, const float* means, const float* sh, uint32_t count,
                                      uint32_t sh_degree, uint32_t active_degree, const float camera_pos[3],
                                      const float* dL_dcolors, float* dL_dsh, float* dL_dmeans, void* hip_stream);
/* ptgs_gaussians_sh_colors_backward plus the gradient with respect to the eye: with SH colours the frame depends on
 * the camera through camera_pos as well (the rasterizer itself does not read it), so a pose gradient of a
 * checkpoint of degree >= 1 needs this term. dL_dsh and the addition into dL_dmeans (which may be null) are those
 * of ptgs_gaussians_sh_colors_backward, bit for bit; in addition dL_dcamera_pos (device float[3]) is written:
 *   dL_dcamera_pos = -sum_i (v_i - dir_i (dir_i . v_i)) / len_i
 * the negative of the sum of what the call adds to dL_dmeans (formed with dL_dmeans == NULL too): the colour sees
 * mean - camera_pos alone. A Gaussian at the eye adds nothing; with active_degree == 0, sh_degree == 0 or
 * count == 0 three exact zeros are written. The sum has two stages: each workgroup of 256 Gaussians leaves one
 * partial (f32, a fixed order), and a second launch on the stream adds the partials in float64 in a fixed order.
 * No atomics: two runs give the same bits. Scratch for the partials (12 bytes per 256 Gaussians) belongs to the
 * context; growing it may synchronise. PTGS_EINVAL as above, and for a null or non-device dL_dcamera_pos
 * (nothing enqueued). */
int ptgs_gaussians_sh_colors_backward_eye(ptgs_ctx* ctx, const float* means, const float* sh, uint32_t count,
                                          uint32_t sh_degree, uint32_t active_degree, const float camera_pos[3],
                                          const float* dL_dcolors, float* dL_dsh, float* dL_dmeans,
                                          float* dL_dcamera_pos, void* hip_stream);
/* Backward of ptgs_gaussians_activate from the ACTIVATED values (what the forward left: scales 3N, opacities
 * N): dL_dlog_scales = dL_dscales * scales, dL_dlogits = (dL_dopacities * o) * (1.0f - o); plain f32, no
 * FMA (checkable bit for bit). In place allowed (dL_dlog_scales == dL_dscales, dL_dlogits == dL_dopacities).
 * These are the derivatives of exp and of the sigmoid; the forward's expx is an exp to about 1e-7 max(1, |x|)
 * relative, so they differentiate the function computed to that accuracy, not its polynomial term by term.
 * PTGS_EINVAL: a null context or pointer; count == 0: PTGS_OK. */
int ptgs_gaussians_activate_backward(ptgs_ctx* ctx, const float* scales, const float* opacities, uint32_t count,
                                     const float* dL_dscales, const float* dL_dopacities, float* dL_dlog_scales,
                                     float* dL_dlogits, void* hip_stream);
/* out[i] = sh[ids[i]] (rows of (sh_degree+1)^2 * 3 floats): SH rows for a copy made by
 * ptgs_gaussians_sort_spatial. out must not alias sh. A row whose id is >= count is written as zeros
 * (never read out of bounds). */
int ptgs_gaussians_permute_sh(ptgs_ctx* ctx, const float* sh, uint32_t sh_degree, const uint32_t* ids,
                              uint32_t count, float* out, void* hip_stream);

/* Backward pass of ptgs_splat_gaussians (training): the gradients of a loss with respect to the
 * Gaussians, given dL/d(out_rgba32f). It consumes the frame the forward left in the context's
 * workspace, so the context's most recent splat call must have been a complete, full-frame
 * ptgs_splat_gaussians (tile rows 0, ~0u; not _over, not _views) rendered with PTGS_FLAG_SPLAT_PUBLISH
 * and stats != NULL for the same count, width and height; the caller guarantees that g, ubo and bg are
 * that frame's. g->chunk_bounds is ignored; g->ids must be NULL (training does not use reordered copies:
 * differentiate the original order).
 *
 * The function being differentiated is the forward as it stands.
 * Per Gaussian (gs_preprocess_one):
 *   culled (every gradient 0) when d = -(view * mean).z <= 0.2, when det == 0, or when its tile rect is empty
 *   means2d = ndc2pix(ph.xy / (ph.w + 1e-7)), ph = mvp * mean, ndc2pix(v, S) = ((v + 1) S - 1) / 2
 *   Sigma = R(q/|q|) S^2 R(q/|q|)^T
 *   cov2d = T Sigma T^T + 0.3 I, T = J W (W: the view's rotation), J = [[fx/d, 0, fx tx/d^2], [0, fy/d, fy ty/d^2]]
 *           at the clamped point tx = clamp(x/d, +-1.3 tan_fovx) d (ty likewise), (x, y, -d) = view * mean
 *   conic (a, b, c) = cov2d^-1
 *   the 3-sigma radius and the rect decide only membership (which tiles hold the Gaussian), the depth
 *   only order: neither carries a gradient
 * Per pixel, over its tile's list in sorted order:
 *   alpha = min(0.99, o exp(power)), power = -(a dx^2 + c dy^2)/2 - b dx dy, (dx, dy) = pixel - means2d
 *   a pair with alpha < 1/255 is skipped; the pixel stops before the Gaussian that would take T below 1e-4
 *   out.rgb = sum c alpha T + T_final bg, out.a = 1 - T_final
 * The gradient is the derivative of exactly this function with every discrete decision (membership,
 * order, skip, stop, culling) held fixed, and min(0.99, .) and clamp as autograd treats them: a pair
 * clamped at 0.99 passes gradient to its colour and, through T, to the pairs behind it, but none to its
 * own opacity, conic or 2D mean; a clamped tx depends on the mean only through d. dL_dout_rgba32f
 * (device, W*H*4) carries all four channels.
 *
 * Stream-ordered on hip_stream. Every non-null array of grads (device pointers) is overwritten (zeroed,
 * then accumulated into). Scratch (9 floats per Gaussian) belongs to the context's splat workspace;
 * growing it may synchronise, like the other workspace buffers. The per-tile partial sums are added with
 * float atomics, so the results are NOT bit-reproducible from run to run (the order of the adds varies).
 * count == 0: PTGS_OK, nothing is launched. PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a
 * null ctx / g / ubo / bg / dL_dout / grads or a null required array, g->ids != NULL, or no matching
 * published frame (above).
 * ptgs_gaussians_sh_colors_backward and ptgs_gaussians_activate_backward continue the chain from
 * grads.colors / means / scales / opacities to a checkpoint's SH coefficients, log-scales and logits.
 * The gradient with respect to the camera pose is ptgs_splat_gaussians_backward_pose (below).
 * Not covered: the `over` composite, tile-row shards. */
typedef struct ptgs_gaussian_grads {
    float* means;      /* 3N */
    float* scales;     /* 3N, w.r.t. the linear scales */
    float* rotations;  /* 4N, w.r.t. the un-normalised quaternion */
    float* opacities;  /* N  */
    float* colors;     /* 3N */
    float* means2d;    /* NULL or 2N: dL/d(pixel position), the densification statistic */
    float* conics;     /* NULL or 3N: dL/d(conic a, b, c); test / debug access to the blend's own output */
} ptgs_gaussian_grads;
int ptgs_splat_gaussians_backward(ptgs_ctx* ctx, const ptgs_gaussians* g, const ptgs_ubo* ubo,
                                  uint32_t width, uint32_t height, const float bg[3],
                                  const float* dL_dout_rgba32f, const ptgs_gaussian_grads* grads,
                                  void* hip_stream);

/* Depth supervision (the trainer's L1 on rendered inverse depth). ptgs_splat_gaussians_invdepth renders the
 * expected inverse depth of the frame the context's latest ptgs_splat_gaussians published:
 *   D[pixel] = sum alpha T / d   over the pixel's list, with the alpha, the skip, the clamp and the stop of the
 *   function stated above and d = -(view * mean).z, the depth the rasterizer sorts by; no background term
 * out_invdepth: device W*H floats; every pixel is written (0 where the tile's list is empty). The frame must meet
 * the conditions of ptgs_splat_gaussians_backward (full-frame, published, with stats, the same width and height);
 * the call only reads it and is not a splat call: the frame stays valid, so it can sit between the forward and
 * the backward. The decisions are taken from z evaluated at (dx, dy) = pixel - means2d, as the backward takes
 * them. Stream-ordered, no host wait, allocates nothing, no atomics: two runs give the same bits.
 * PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a null ctx or out_invdepth, out_invdepth not a
 * device pointer, no matching published frame.
 *
 * ptgs_splat_gaussians_backward_depth is ptgs_splat_gaussians_backward for a loss that depends on both out and
 * D, in one pass: dL_dinvdepth (device, W*H) is dL/dD. The function being differentiated gains one sentence:
 *   D = sum alpha T / d with the same alpha and T, every discrete decision held fixed as before
 * so D passes gradient to the opacity, the conic and the 2D mean of a Gaussian through alpha and T exactly as a
 * fourth colour channel of value 1 / d with background 0 would, and to the mean through 1 / d,
 * d = -(view row 2) . (mean, 1). The depth still carries no gradient through order or membership; grads.colors
 * does not depend on dL_dinvdepth. Contract, outputs and error paths are those of ptgs_splat_gaussians_backward
 * (scratch: 10 floats per Gaussian), plus PTGS_EINVAL for a null or non-device dL_dinvdepth.
 * Not covered: depth for _over, _views and tile-row shards, expected (non-inverse) or median depth, normals. */
int ptgs_splat_gaussians_invdepth(ptgs_ctx* ctx, uint32_t width, uint32_t height, float* out_invdepth,
                                  void* hip_stream);
int ptgs_splat_gaussians_backward_depth(ptgs_ctx* ctx, const ptgs_gaussians* g, const ptgs_ubo* ubo,
                                        uint32_t width, uint32_t height, const float bg[3],
                                        const float* dL_dout_rgba32f, const float* dL_dinvdepth,
                                        const ptgs_gaussian_grads* grads, void* hip_stream);

/* The camera-pose gradient (pose refinement, tracking, joint pose and scene optimisation).
 * ptgs_splat_gaussians_backward_pose does everything ptgs_splat_gaussians_backward does, or
 * ptgs_splat_gaussians_backward_depth when dL_dinvdepth != NULL (NULL: the loss depends on the image alone): the
 * frame conditions, the grads outputs and the error paths are the same. In addition it writes dL_dview (device
 * float[16]), column-major like ptgs_ubo.view: entry c * 4 + r is dL/d view[r][c].
 * The function differentiated is the one stated above, read as a function of `view`:
 *   (x, y, -d) = view * (mean, 1)
 *   W is the upper-left 3x3 of view in T = J W
 *   ph = (proj * view) * (mean, 1) with proj a constant (mvp is formed on the host; the gradient treats it as
 *   that product)
 *   fx, fy and the clamp limits are constants; the rasterizer does not read camera_pos
 *   every discrete decision is held fixed, as before; a clamped tx depends on the view through d only
 *   with dL_dinvdepth, 1 / d passes gradient to row 2 of view
 *   row 3 of view is held at (0, 0, 0, 1): its four entries are written as exactly 0
 * Per visible Gaussian, with mh = (mean, 1), dpx, dpy, dd = dL/d(x, y, d) and dph = dL/d ph, the twelve
 * contributions are g_r * mh[c] (r < 3, c < 4) with
 *   g = (dpx, dpy, -dd) + the first three entries of proj^T (dphx, dphy, 0, dphw)
 * and the rotation block additionally gets J^T dT (dT = dL/dT): row 0 J00 dT[0][k], row 1 J11 dT[1][k], row 2
 * J02 dT[0][k] + J12 dT[1][k]. A culled Gaussian contributes exactly 0.
 * The sum over the Gaussians has two stages: each workgroup of 256 Gaussians leaves one partial of 12 floats
 * (f32, a fixed order), and a second launch on the stream adds the partials in float64 in a fixed order and
 * writes the 16 floats. It uses no atomics; dL_dview still inherits the run-to-run variation of the blend's
 * per-Gaussian sums (above). Scratch (48 bytes per 256 Gaussians) belongs to the context's splat workspace and is
 * grown like the other buffers; every partial read was written by the same call.
 * count == 0: dL_dview is set to sixteen zeros, PTGS_OK. PTGS_EINVAL (nothing enqueued), besides the cases above:
 * a null or non-device dL_dview.
 * With SH colours the eye adds its own term: ptgs_gaussians_sh_colors_backward_eye.
 * Not covered: gradients with respect to proj (the intrinsics). */
int ptgs_splat_gaussians_backward_pose(ptgs_ctx* ctx, const ptgs_gaussians* g, const ptgs_ubo* ubo,
                                       uint32_t width, uint32_t height, const float bg[3],
                                       const float* dL_dout_rgba32f, const float* dL_dinvdepth,
                                       const ptgs_gaussian_grads* grads, float* dL_dview, void* hip_stream);

/* Densification and pruning of a training run (densify_and_prune of Kerbl et al.'s trainer, new Gaussians
 * inheriting the parent's screen radius), in three steps: a statistic accumulated after every backward, a
 * plan (decision per Gaussian + scan) and one gather that writes the new arrays. Every float operation is an
 * IEEE f32 add / sub / mul / div / sqrt in the order written (no FMA, no transcendental: the caller passes the
 * activated scales and opacities of ptgs_gaussians_activate), so a float32 restatement is reproduced bit for
 * bit, and no float atomics are used: results are the same from run to run. All arrays are device pointers.
 *
 * Common argument handling: PTGS_EINVAL (message in ptgs_last_error, nothing enqueued) for a null ctx or a null
 * required pointer, or an output that is not a device pointer. n == 0: PTGS_OK before any array pointer is
 * looked at, nothing is launched (the plan's counts are all zero, and it is a valid plan of 0 -> 0).
 *
 * ptgs_densify_accumulate: once per training view, after the backward. g2d (2n) is dL/d(pixel position)
 * (ptgs_gaussian_grads.means2d), radii (n, int32) the frame's ptgs_splat_buffers.radii, W x H the frame's
 * size. A Gaussian is visible when radii[i] > 0; for a visible one
 *   gx = g2d[2i] * (0.5f * W); gy = g2d[2i+1] * (0.5f * H)     (the NDC convention the 0.0002 threshold is stated in)
 *   accum[i] += sqrt(gx*gx + gy*gy); denom[i] += 1.0f; max_radii[i] = max(max_radii[i], (float)radii[i])
 * and an invisible one is left untouched. accum / denom / max_radii: n floats each, zero before the first
 * view. One work-item owns one i. Stream-ordered; allocates nothing.
 *
 * ptgs_gaussians_densify_plan: scales (3n) and opacities (n) are the activated values.
 *   avg  = denom > 0 ? accum / denom : 0;  smax = max(max(s.x, s.y), s.z);  hot = avg >= grad_threshold
 *   clone = hot && smax <= scale_split;  split = hot && smax > scale_split
 *   P(o, m, r) = o < min_opacity || (max_screen_radius > 0 && r > max_screen_radius) || (max_scale > 0 && m > max_scale)
 *   the original survives iff !split && !P(o, smax, r); its clone exists iff clone && !P(o, smax, r);
 *   its two children exist iff split && !P(o, smax / 1.6f, r)                     (r = max_radii[i])
 * Output order (the trainer's concatenation order after its masks): surviving originals by source index, clones
 * by source index, all first children by source index, all second children by source index; total = survivors +
 * clones + 2 split_sources. The call launches the decision and a two-level exclusive scan, waits for the stream,
 * returns the counts and leaves in the context's workspace (grown when needed; that may synchronise the
 * device) a map source[total]: the source index in bits 0..29, the kind in bits 30..31 (0 original, 1 clone,
 * 2 first child, 3 second child), written stream-ordered for ptgs_gaussians_densify_apply. pruned_originals
 * counts the originals the prune test removed (a split parent is replaced, not pruned), pruned_children the
 * children it removed (two per source). n above 2^30 (the index would not fit beside the kind): PTGS_EINVAL.
 *
 * ptgs_gaussians_densify_apply consumes the plan the context's latest plan call left: PTGS_EINVAL when there is
 * none, or when n / n_out differ from its n / total. An original or a clone copies every array's row of its
 * source. Child k (0, 1) of source i copies its rows too, except
 *   log_scales' = log_scales - 0.4700036f                                 (ln 1.6: the trainer's / (0.8 * 2))
 *   mean' = mean + R v, v = scales * noise[k][i]   (noise: float [2][n][3], standard-normal draws of the caller)
 *   R = the rotation of (w, x, y, z) / len, len = sqrt(((w*w + x*x) + y*y) + z*z); len == 0: the identity
 *   R = [[1 - 2 (y*y + z*z), 2 (x*y - w*z), 2 (x*z + w*y)], [2 (x*y + w*z), 1 - 2 (x*x + z*z), 2 (y*z - w*x)],
 *        [2 (x*z - w*y), 2 (y*z + w*x), 1 - 2 (x*x + y*y)]] evaluated as written (the forward projection's order)
 *   (R v)_r = (R_r0*v0 + R_r1*v1) + R_r2*v2
 * means / log_scales / rotations (un-normalised) / scales (activated) are the source arrays (3n, 3n, 4n, 3n),
 * means_out / log_scales_out have 3 n_out floats. rows[0 .. n_rows) (n_rows <= 16, read by the host during the
 * call) are the other per-Gaussian arrays: rotations, logits, SH coefficients, Adam moments, ...: dst row j
 * (width floats) = src row of j's source, or zeros when zero_new is set and j is a clone or a child. Any width
 * >= 1 and any 4-byte-aligned base are accepted (16-byte accesses are used only where base and width allow).
 * PTGS_EINVAL: n_rows > 16, a width of 0, a null src / dst, or an output (means_out, log_scales_out, a dst,
 * source_out) that overlaps an input or another output. source_out: NULL, or n_out u32 that receive the map.
 * n_out == 0 (everything pruned): PTGS_OK, nothing is launched. Stream-ordered; allocates nothing. */
typedef struct ptgs_densify_params {
    float grad_threshold;     /* on the averaged statistic (the trainer's 0.0002) */
    float scale_split;        /* percent_dense x scene extent: clone at or below it, split above */
    float min_opacity;        /* prune below it (0.005) */
    float max_scale;          /* prune above it (0.1 x scene extent); 0: test disabled */
    float max_screen_radius;  /* prune above it, in pixels; 0: test disabled */
} ptgs_densify_params;
typedef struct ptgs_densify_counts {
    uint32_t survivors;
    uint32_t clones;
    uint32_t split_sources;
    uint32_t pruned_originals;
    uint32_t pruned_children;
    uint32_t total;
} ptgs_densify_counts;
typedef struct ptgs_densify_rows {
    const float* src;   /* n rows */
    float* dst;         /* n_out rows */
    uint32_t width;     /* floats per Gaussian */
    uint32_t zero_new;  /* != 0: clones and children get zeros (optimizer moments) */
} ptgs_densify_rows;
#define PTGS_DENSIFY_MAX_ROWS 16
int ptgs_densify_accumulate(ptgs_ctx* ctx, const float* g2d, const int32_t* radii, uint32_t n, uint32_t width,
                            uint32_t height, float* accum, float* denom, float* max_radii, void* hip_stream);
int ptgs_gaussians_densify_plan(ptgs_ctx* ctx, const float* scales, const float* opacities, const float* accum,
                                const float* denom, const float* max_radii, uint32_t n,
                                const ptgs_densify_params* params, ptgs_densify_counts* out, void* hip_stream);
int ptgs_gaussians_densify_apply(ptgs_ctx* ctx, uint32_t n, uint32_t n_out, const float* means,
                                 const float* log_scales, const float* rotations, const float* scales,
                                 const float* noise, float* means_out, float* log_scales_out,
                                 const ptgs_densify_rows* rows, uint32_t n_rows, uint32_t* source_out,
                                 void* hip_stream);

/* The 3DGS training loss (Kerbl et al.) of a rendered frame against a target, and its gradient:
 *   loss = (1 - lambda) * l1 + lambda * (1 - ssim),   l1 = mean |a - b|,   ssim = mean m     (lambda = 0.2 in the paper)
 * a = image_rgba32f [H, W, 4] as the rasterizer writes it, b = target [H, W, target_channels], target_channels
 * 3 or 4; both contiguous device float32, values expected in roughly [0, 1] (NaN / Inf and HDR magnitudes are
 * not handled). Only channels 0..2 take part; the means are over n = 3 W H values.
 *   g[k] = exp(-(k - 5)^2 / (2 * 1.5^2)), k = 0..10, normalised to sum 1;  w = g (x) g
 *   conv(x) = per-channel correlation with w, zero padding of 5 (missing pixels count as 0; no renormalisation)
 *   mu1 = conv(a); mu2 = conv(b); s1 = conv(a a) - mu1^2; s2 = conv(b b) - mu2^2; s12 = conv(a b) - mu1 mu2
 *   C1 = 0.01^2; C2 = 0.03^2; A = 2 mu1 mu2 + C1; B = 2 s12 + C2; Cc = mu1^2 + mu2^2 + C1; D = s1 + s2 + C2
 *   m = A B / (Cc D)
 *   dm/ds1 = -m / D;  dm/ds12 = 2 A / (Cc D)
 *   dm/dmu1 = 2 mu2 B / (Cc D) - 2 mu1 m / Cc - 2 mu1 dm/ds1 - mu2 dm/ds12
 *   G = conv(dm/dmu1) + 2 a conv(dm/ds1) + b conv(dm/ds12)
 *   dL/da = grad_scale * [ (1 - lambda) / n * sign(a - b) - lambda / n * G ],   sign(0) = 0
 * loss_out: device float[4] = (loss, l1, ssim, 0). dL_dimage_rgba32f: device [H, W, 4], every element
 * overwritten (alpha with 0), or NULL: only the terms are computed (bit for bit the terms of a call with the
 * gradient). The arithmetic is f32 with explicit FMA, separable (11 + 11 taps), the sums of the two means in
 * f64; the contract is a tolerance against a float64 evaluation of the formulas above, not bit-exactness
 * against a restatement. There are no float atomics and every sum has a fixed order: two calls on the same
 * inputs give the same bits. Stream-ordered with no host wait; the partial maps (36 bytes per pixel) live in a
 * workspace of the context that grows on demand (a growing call frees the old one, which may synchronise the
 * device), so the calls of one context must be ordered on their streams. Any 4-byte-aligned base is accepted
 * (16-byte accesses where the bases allow).
 * PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a null ctx, image, target or loss_out; width or
 * height 0 or above 16384; target_channels not 3 or 4; lambda NaN or outside [0, 1]; grad_scale not finite;
 * dL_dimage overlapping image or target; loss_out or dL_dimage not a device pointer. */
int ptgs_image_loss_l1_dssim(ptgs_ctx* ctx, const float* image_rgba32f, const float* target,
                             uint32_t target_channels, uint32_t width, uint32_t height, float lambda,
                             float grad_scale, float* loss_out, float* dL_dimage_rgba32f, void* hip_stream);

/* The trainer's depth regulariser: an L1 between a rendered inverse depth (ptgs_splat_gaussians_invdepth) and a
 * target given as a VIEW DEPTH map t, as ptgs_trace_depth writes it (both device, W*H floats). A pixel is
 * supervised when t > 0; that includes +inf (a miss), whose target inverse depth is 0. A pixel with t <= 0 or a
 * NaN t is not supervised: it adds 0 to the loss and gets gradient 0.
 *   term = |D - 1.0f / t|                      f32, IEEE divide, no contraction
 *   sum  = the f64 sum of the terms in a fixed order (per workgroup, then one final workgroup)
 *   terms = (weight * sum / (W H), sum / (W H), number of supervised pixels, 0)      device float[4], rounded to f32
 *   dL/dD = k * sign(D - 1.0f / t), sign(0) = 0, k = (float)((double)weight * grad_scale / (W H))
 * The mean is over all W H pixels (the trainer's .mean() of the masked difference). dL_dinvdepth: device W*H,
 * every element overwritten, or NULL: only the terms (bit for bit those of a call with the gradient). No atomics:
 * two calls give the same bits. Stream-ordered, no host wait; the per-workgroup sums live in the context's loss
 * workspace, which grows on demand as for ptgs_image_loss_l1_dssim.
 * PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a null ctx, invdepth, target_depth or terms; width
 * or height 0 or above 16384; weight or grad_scale not finite; dL_dinvdepth overlapping invdepth or target_depth;
 * invdepth, target_depth, terms or dL_dinvdepth not a device pointer. */
int ptgs_image_loss_invdepth_l1(ptgs_ctx* ctx, const float* invdepth, const float* target_depth, uint32_t width,
                                uint32_t height, float weight, float grad_scale, float* terms,
                                float* dL_dinvdepth, void* hip_stream);

/* The optimizer step of a training run: Adam (Kingma & Ba; no weight decay, no amsgrad) over every per-Gaussian
 * parameter array in one launch, optionally skipping the Gaussians the view did not see (the `sparse_adam` of
 * Kerbl et al.'s trainer, after Taming-3DGS), and the trainer's opacity reset. All arrays are device pointers.
 *
 * ptgs_gaussians_adam_step: rows[0 .. n_rows) (1 <= n_rows <= 16, read by the host during the call) are the
 * parameter arrays, each with its gradient and its two moments, n rows of `width` floats. Every operation is
 * an IEEE f32 add / sub / mul / div / sqrt in the order written (no FMA, no transcendental on the device, no
 * atomics), so a float32 restatement is reproduced bit for bit. The host computes once per call
 *   ob1 = 1.0f - beta1;  ob2 = 1.0f - beta2                                   (f32)
 *   bc1 = (float)(1.0 - pow((double)beta1, (double)step))
 *   bc2s = (float)sqrt(1.0 - pow((double)beta2, (double)step))
 *   per row: ss = lr / bc1;  ss_head = lr_head / bc1                         (f32 divisions)
 * and every element, with g its gradient and c its column (its index within the row), becomes
 *   m' = (beta1 * m) + (ob1 * g)
 *   v' = (beta2 * v) + ((ob2 * g) * g)
 *   d  = (sqrt(v') / bc2s) + eps
 *   p' = p - ((c < head ? ss_head : ss) * (m' / d))
 * head splits a row's rate: the first `head` floats step with lr_head (the SH DC term of a [16, 3] row: head 3),
 * the others with lr. step counts the calls of the run, 1 for the first; it is global: a Gaussian that was
 * skipped is corrected like one that was not, as in the trainer's sparse Adam.
 * radii: NULL, or n int32 (the frame's ptgs_splat_buffers.radii). With radii, a Gaussian with radii[i] <= 0 is
 * left untouched in param, exp_avg and exp_avg_sq of every row, bit for bit (and none of them is read); with
 * NULL every Gaussian steps (a dense Adam). With PTGS_FLAG_SPLAT_OVERLAP the published radii may be rewritten
 * by the next frame's front end: pass the frame's own radii only for frames that are not overlapped, or a copy.
 * Bit-exactness holds for finite inputs whose intermediates are normal numbers or zero; with g == 0 and v == 0
 * the update is exactly 0 (0 / eps). Subnormal intermediates give finite results, but are outside the bit-exact
 * claim. NaN and Inf gradients propagate and are not handled. Any width >= 1 and any 4-byte-aligned base are
 * accepted (16-byte accesses are used only where the width and all four bases of a row allow).
 * Stream-ordered, allocates nothing, no host wait; two calls on the same inputs give the same bits.
 * PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a null ctx, rows or params; n_rows == 0 or > 16;
 * a null param / grad / exp_avg / exp_avg_sq; a width of 0; head > width; step == 0; beta1 or beta2 NaN or
 * outside [0, 1); eps NaN, negative or infinite; an lr or lr_head that is not finite; a written array (param,
 * exp_avg, exp_avg_sq) that overlaps another array of the table or radii; a written array that is not a device
 * pointer. PTGS_ERANGE: more elements than one launch holds. n == 0: PTGS_OK before the rows' pointers are
 * looked at, nothing is launched.
 *
 * ptgs_gaussians_opacity_reset (the trainer's reset_opacity, every 3000 iterations), in exact arithmetic:
 *   cap = (float)log((double)max_opacity / (1.0 - (double)max_opacity))     (host)
 *   logit' = logit > cap ? cap : logit                                       (a NaN stays)
 * and zeros to every element of exp_avg and exp_avg_sq (n floats each) where they are given: the trainer
 * replaces the opacity's moments by zeros for all Gaussians. The trainer computes inverse_sigmoid(min(sigmoid(x),
 * 0.01)), which rounds a logit below the cap through a sigmoid and back; this form leaves such a logit as it is.
 * Stream-ordered, allocates nothing. PTGS_EINVAL: a null ctx or opacity_logits; max_opacity NaN or not in
 * (0, 1); the three arrays overlapping; one of them not a device pointer. n == 0: PTGS_OK, nothing launched. */
typedef struct ptgs_adam_rows {      /* one per-Gaussian parameter array; 48 bytes */
    float* param;                    /* n rows of `width` floats, updated in place */
    const float* grad;               /* n rows, read only */
    float* exp_avg;                  /* n rows, updated in place */
    float* exp_avg_sq;               /* n rows, updated in place */
    uint32_t width;                  /* floats per Gaussian, >= 1 */
    uint32_t head;                   /* the first `head` floats of every row step with lr_head; 0: none; <= width */
    float lr;
    float lr_head;
} ptgs_adam_rows;
typedef struct ptgs_adam_params { float beta1, beta2, eps; uint32_t step; } ptgs_adam_params;  /* step: 1 for the first */
#define PTGS_ADAM_MAX_ROWS 16
int ptgs_gaussians_adam_step(ptgs_ctx* ctx, uint32_t n, const ptgs_adam_rows* rows, uint32_t n_rows,
                             const ptgs_adam_params* params, const int32_t* radii /* NULL: every row */,
                             void* hip_stream);
int ptgs_gaussians_opacity_reset(ptgs_ctx* ctx, float* opacity_logits, uint32_t n, float max_opacity,
                                 float* exp_avg /* NULL or n */, float* exp_avg_sq /* NULL or n */, void* hip_stream);

/* The two ends of a training run (pathtracer_gaussiansplatting_amd/train.py): the leaves of a checkpoint from
 * initialised Gaussians, and the squared error its evaluation reports as PSNR. Both are stream-ordered, wait for
 * nothing on the host, allocate nothing, use no atomics (two runs give the same bits) and take device pointers.
 *
 * ptgs_gaussians_checkpoint_init: the inverse of ptgs_gaussians_activate plus the trainer's RGB2SH, in one launch:
 * what ptgs_gaussians_from_points wrote (scales 3n, opacities n, colors 3n, post-activation) becomes what a
 * trainer optimises and ptgs_read_gaussian_ply returns. Numerical contract (f32, no FMA, checkable bit for bit):
 *   log_scales[e]     = log2x(scales[e]) * 0.69314718055994531f                       (detmath.h log2x)
 *   opacity_logits[i] = (log2x(o) - log2x(1.0f - o)) * 0.69314718055994531f,   o = opacities[i]
 *   sh[i][0][c]       = (colors[3 i + c] - 0.5f) / C0f      (IEEE division; C0 of ptgs_gaussians_sh_colors)
 *   sh[i][k][c]       = +0.0f for every k >= 1
 * sh: float[n][(sh_degree+1)^2][3], the layout of ptgs_gaussians_sh_colors; sh_degree in 0..3. log2x is an atanh
 * series, accurate to about 1e-7 relative in the logarithm's value away from 1 and to about 1e-7 absolute near it.
 * In place is allowed as for activate (log_scales == scales, opacity_logits == opacities); any other overlap of
 * an output with another array of the call is refused. log2x returns -1e30 for an argument that is not positive,
 * so o == 0 gives a logit of about -6.9e29 and o == 1 about +6.9e29 (finite, never NaN or Inf; activate maps
 * them back to less than 1e-38 and to exactly 1), a scale of 0 a log-scale of about -6.9e29: a caller that wants bounded leaves clips its opacities
 * and scales first. PTGS_EINVAL (message in ptgs_last_error, nothing enqueued): a null ctx; sh_degree above 3; a
 * null pointer; such an overlap; an output that is not a device pointer. n == 0: PTGS_OK before any pointer is
 * looked at, nothing is launched.
 *
 * ptgs_image_mse: out_sum (device double[1]) = sum over every pixel p and c = 0..2 of (double)(d * d),
 * d = image_rgba32f[4 p + c] - target[target_channels p + c] in f32 (the product rounded to f32, then widened).
 * target_channels is 3 or 4, as for ptgs_image_loss_l1_dssim. The sum has a fixed order: at most 1024 workgroups,
 * each over a contiguous span of pixels (a work-item adds its pixels in index order, the workgroup's 256 sums meet
 * in a halving tree), then one workgroup adds the workgroups' sums likewise, all in f64. Identical images give
 * exactly 0. The host computes mse = sum / (3 W H) and PSNR = -10 log10(mse) after reading the double back. The
 * workgroups' sums (8 KiB) belong to the context since ptgs_create, so the calls of one context must be ordered on
 * their streams. PTGS_EINVAL: a null ctx; target_channels not 3 or 4; a null image, target or out_sum; out_sum not
 * a device pointer. width * height == 0: PTGS_OK before any pointer is looked at; out_sum is not written. */
int ptgs_gaussians_checkpoint_init(ptgs_ctx* ctx, const float* scales, const float* opacities, const float* colors,
                                   uint32_t n, uint32_t sh_degree, float* log_scales, float* opacity_logits,
                                   float* sh, void* hip_stream);
int ptgs_image_mse(ptgs_ctx* ctx, const float* image_rgba32f, const float* target, uint32_t target_channels,
                   uint32_t width, uint32_t height, double* out_sum, void* hip_stream);

/* Report of the stream-ordered splat (no stats): waits for hip_stream and the context's view streams,
 * then returns (and clears) the counts since the last query. frames / views[v]: frames left
 * incomplete (spill pool exhausted, see PTGS_EINCOMPLETE; each was also reported by a later call)
 * per view slot v (slot 0 counts ptgs_splat_gaussians / _over and view 0 of
 * ptgs_splat_gaussians_views); frames = their sum. spilled_tiles: tiles completed through the spill
 * pool (rendered; a measure of how far the camera outran the buffers sized from earlier frames);
 * incomplete_tiles: tiles left at the background. pair_capacity: the smallest pair capacity over the
 * slots in use; last_pairs: the largest pair count any slot's latest frame produced; spill_capacity /
 * spill_demand: slot 0's pool and the largest demand of one of its frames so far. */
typedef struct ptgs_splat_status {
    uint64_t frames;
    uint32_t views[PTGS_MAX_VIEWS];
    uint32_t pair_capacity;
    uint32_t last_pairs;
    uint32_t touched_runs;  /* slot 0's latest frame: (front-end workgroup, tile) runs, i.e. per-tile
                             * reservations of the fused front end / nonzero histogram entries of the
                             * count: the spatial coherence of the Gaussians' order */
    uint32_t fused;         /* slot 0's latest frame ran the fused front end */
    uint64_t spilled_tiles;
    uint64_t incomplete_tiles;
    uint32_t spill_capacity;
    uint32_t spill_demand;
} ptgs_splat_status;
int ptgs_splat_status_read(ptgs_ctx* ctx, ptgs_splat_status* out, void* hip_stream);

/* Grow the pair buffers and spill pools of every view slot to at least `pairs` (Gaussian, tile) pairs:
 * stream-ordered frames of up to that many pairs then store every pair (three-launch front end) or
 * complete every spilled tile (fused rows: a frame's spilled tiles hold at most its pair count), so
 * they are never incomplete — including hipGraph replays, whose row capacity is fixed at capture
 * (e.g. before capturing, or from a previous frame's stats.num_rendered plus headroom).
 * Synchronises the device when it grows. */
int ptgs_splat_reserve(ptgs_ctx* ctx, uint32_t pairs);

/* Hybrid composite (C4): the same splat, front to back over an image: a pixel stops at the first
 * Gaussian whose view depth is >= depth[pixel] (the mesh occludes it and everything behind), and
 * out = C + T * under (all four channels, C.a = 1 - T). depth: device float[W*H] (e.g. from
 * ptgs_trace_depth); under: device RGBA32F[W*H] (e.g. the ptgs_trace_camera accumulator); out may
 * alias under, for calls with stats too, whether the call re-runs its frame or not: such a call
 * composites over under as the caller passed it, through a copy the context keeps (W*H*16 bytes,
 * taken in stream order when the two ranges overlap at all; calls without stats, and calls whose out is
 * apart from under, copy nothing). A call without stats blends once, each pixel reading under before
 * it writes out: there out is under itself or does not overlap it.
 * Integer outputs (keys, values, ranges) are those of ptgs_splat_gaussians. */
int ptgs_splat_gaussians_over(ptgs_ctx* ctx, const ptgs_gaussians* g, const ptgs_ubo* ubo, uint32_t width,
                              uint32_t height, const float* depth, const float* under_rgba32f,
                              uint32_t tile_row_begin, uint32_t tile_row_end, float* out_rgba32f,
                              ptgs_splat_stats* stats, void* hip_stream);

/* 3DGS initialisation from a point cloud (Kerbl et al. 2023 create_from_pcd; the point cloud is the
 * reference's points3d.ply, Engine::savePly engine.cpp:2849-2895, read with ptgs_read_ply).
 * ptgs_knn3_mean_dist2: dist2[i] = mean of the 3 smallest squared distances from point i to the
 * other points, exact in f32 ((dx*dx + dy*dy) + dz*dz, no FMA; ((b0 + b1) + b2) / 3); fewer than 3
 * other points: mean of those, none: 0. ptgs_gaussians_from_points writes post-activation
 * parameters (ptgs_gaussians layout): means = xyz, scales = sqrt(max(dist2, 1e-7)) x3, rotations =
 * (1, 0, 0, 0), opacities = 0.1, colors = rgb / 255 (rgb: device uchar[3N] or NULL = black).
 * All buffers are device pointers; both calls synchronise the stream (temporaries are freed). */
int ptgs_knn3_mean_dist2(ptgs_ctx* ctx, const float* xyz, uint32_t n, float* dist2, void* hip_stream);
int ptgs_gaussians_from_points(ptgs_ctx* ctx, const float* xyz, const uint8_t* rgb, uint32_t n, float* means,
                               float* scales, float* rotations, float* opacities, float* colors, void* hip_stream);

/* Debug/parity access to the integer intermediates of the most recent ptgs_splat_gaussians call
 * (device buffers owned by the context, valid until the next splat call):
 * radii[N] (int32), tiles_touched[N] (u32), sorted keys[K] (u64: tile<<32 | depth bits),
 * sorted values[K] (u32 gaussian index), tile ranges[tiles] (uint2 start,end). sorted_keys /
 * sorted_values are NULL unless that call ran with PTGS_FLAG_SPLAT_PUBLISH and stats. */
/* radii / tiles_touched / means2d / depths / conic_opacity are written only by frames rendered with
 * PTGS_FLAG_SPLAT_PUBLISH (indexed by the caller's Gaussian index, see ptgs_gaussians.ids); tile_ranges
 * by every frame (unpublished fused frames: end - begin = the tile's pair count, begin = t * capacity). */
typedef struct ptgs_splat_buffers {
    const int32_t* radii;
    const uint32_t* tiles_touched;
    const uint64_t* sorted_keys;
    const uint32_t* sorted_values;
    const uint32_t* tile_ranges;
    const float* means2d;   /* 2N */
    const float* depths;    /* N */
    const float* conic_opacity; /* 4N */
    uint32_t num_gaussians;
    uint32_t num_rendered;
    uint32_t num_tiles;
} ptgs_splat_buffers;
int ptgs_splat_get_buffers(const ptgs_ctx* ctx, ptgs_splat_buffers* out);
/* Debug/parity access to the most recent splat call's own pair rows when its front end was the fused
 * one (every frame, published or not, timed or overlapped: the bench's frames): tile t's pairs are
 * rows[t * row_capacity .. t * row_capacity + n_t), n_t = end - begin of tile_ranges[t] (the blend
 * writes those ranges), each pair (depth bits << 32) | gaussian index, in no particular order (the blend
 * sorts them in LDS; a tile's row may be left permuted). A tile with n_t > row_capacity kept its first
 * row_capacity pairs only (completed through the spill pool). *rows = NULL, *row_capacity = 0 when that
 * frame ran the three-launch front end. Device memory owned by the context, valid until the next splat
 * call; synchronise the call's stream before reading. No reference counterpart (test access). */
int ptgs_splat_get_tile_rows(const ptgs_ctx* ctx, const uint64_t** rows, uint32_t* row_capacity);

/* With PTGS_FLAG_TIME_STAGES: milliseconds of the stages of the most recent ptgs_splat_gaussians
 * call, measured with hipEvents on its stream: [0] preprocess + count (tile histograms) [1] column
 * scan (tile totals) [2] scatter (pairs into tile segments, K) [3] radix sort of the tiles above 512 pairs
 * [4] 0 [5] sort (tiles up to 512 pairs) + blend. Synchronises. */
int ptgs_splat_stage_ms(ptgs_ctx* ctx, float out_ms[6]);

/* ---------------- dataset capture (Engine::captureSceneData, engine.cpp:2658-2814) -------- */
typedef struct ptgs_capture_desc {
    const char* out_dir;            /* writes out_dir/train/r_<i>.jpg, transforms_{train,test}.json, points3d.ply */
    uint32_t width, height;         /* render size (the reference's swapchain extent) */
    uint32_t total_positions;       /* camera views (settings "total_positions", default 336) */
    uint32_t accumulation_steps;    /* samples per view and torus frames (settings default 512) */
    float min_beta, max_beta;       /* torus elevation range, degrees (defaults -45, 45) */
    float fov_deg;                  /* camera fov (60) */
    float major_radius, torus_height; /* Camera::updateToroidalAngles radius / height */
    float image_divisor;            /* > 1: every 2nd pixel is kept (engine.cpp:2737-2754) */
    uint32_t seed;                  /* mt19937 seed (13) */
    uint32_t capture_images, capture_pointcloud;
    const ptgs_ubo* ubo;            /* template: ambient light, fluxes, lod settings (view/proj/frame set per view) */
    ptgs_ray_push torus;            /* torus push constants for the point cloud */
    const ptgs_ray_sample* samples; /* device array (Morton-sorted RaySamples), num_samples entries */
    uint32_t num_samples;
    void* hip_stream;
} ptgs_capture_desc;

/* Synchronous: traces every view (one batched ptgs_trace_camera call of accumulation_steps samples per
 * view), encodes/reads back/downsamples/writes JPEG quality 90, accumulates the torus point cloud,
 * writes the PLY and the two transforms files. Requires an uploaded scene. */
int ptgs_capture_dataset(ptgs_ctx* ctx, const ptgs_capture_desc* desc);

/* ---------------- multi-GPU frame reduce over RCCL / xGMI ---------------- */
/* The path tracer shards samples across GPUs (ptgs_trace_camera with PTGS_ACCUM_SUM and
 * frame_stride = number of GPUs) and sums the RGBA32F buffers; tile-row shards of the splat are
 * disjoint and combine with the same sum. One RCCL communicator per context: one rank calls
 * ptgs_comm_unique_id, the caller ships the 128 bytes to every rank (any channel), each rank calls
 * ptgs_comm_create with its rank. RCCL is loaded at run time; without it these return PTGS_EHIP. */
#define PTGS_COMM_ID_BYTES 128
int ptgs_comm_unique_id(uint8_t id[PTGS_COMM_ID_BYTES]);
int ptgs_comm_create(ptgs_ctx* ctx, const uint8_t id[PTGS_COMM_ID_BYTES], int nranks, int rank);
int ptgs_comm_destroy(ptgs_ctx* ctx);
/* In-place SUM of n_floats device floats: to `root` (ncclReduce) or to every rank (ncclAllReduce).
 * Stream-ordered on hip_stream. */
int ptgs_reduce_radiance(ptgs_ctx* ctx, float* accum, size_t n_floats, int root, void* hip_stream);
int ptgs_allreduce_radiance(ptgs_ctx* ctx, float* accum, size_t n_floats, void* hip_stream);
/* Tile-row shards of the splat: rank g's pixel rows [row_ranges[2 g], row_ranges[2 g + 1]) of its
 * RGBA32F width x height image are copied into the same rows of root's image (ncclSend / ncclRecv in
 * one group: each rank moves only its own rows, W*H*16/G bytes, instead of a full-frame reduce).
 * row_ranges holds every rank's range (2 x nranks, identical on all ranks). Stream-ordered. */
int ptgs_gather_rows(ptgs_ctx* ctx, float* image, uint32_t width, uint32_t height, const uint32_t* row_ranges,
                     int root, void* hip_stream);
/* Reduce-scatter by rows (the C5 hybrid's radiance): afterwards rank g's rows [row_ranges[2 g],
 * row_ranges[2 g + 1]) of its RGBA32F image hold the SUM over all ranks of those rows (other rows
 * unspecified); one ncclReduce per rank's rows (root = that rank) in one group: about one frame sent
 * per rank instead of an all-reduce's two. row_ranges as ptgs_gather_rows. Stream-ordered. */
int ptgs_reduce_scatter_rows(ptgs_ctx* ctx, float* image, uint32_t width, uint32_t height, const uint32_t* row_ranges,
                             void* hip_stream);

/* ---------------- output encode (blit rgba32f -> B8G8R8A8_SRGB, engine.cpp:2004-2020) --------- */
/* rgba8 (device W*H u32, R in the low byte): linear -> sRGB8 of clamp(rgb,0,1), alpha 255. */
int ptgs_encode_srgb8(ptgs_ctx* ctx, const float* rgba32f, uint32_t width, uint32_t height,
                      uint32_t* rgba8, void* hip_stream);

/* ---------------- device memory helpers (usable without any other GPU framework) ------------ */
int ptgs_device_alloc(ptgs_ctx* ctx, size_t bytes, void** out);
int ptgs_device_free(ptgs_ctx* ctx, void* ptr);
int ptgs_memcpy_h2d(ptgs_ctx* ctx, void* dst, const void* src, size_t bytes);
int ptgs_memcpy_d2h(ptgs_ctx* ctx, void* dst, const void* src, size_t bytes);
int ptgs_memset_d32(ptgs_ctx* ctx, void* dst, uint32_t value, size_t count, void* hip_stream);
int ptgs_synchronize(ptgs_ctx* ctx);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* PTGS_H_ */
