// splat_backward.hip — backward pass of the 3DGS rasterizer for gfx950 (ptgs_splat_gaussians_backward).
//
// It differentiates the forward of splat.hip as it stands (the contract is stated in ptgs.h) and consumes
// the frame that forward published: every tile's depth-sorted Gaussians and the per-Gaussian blend records.
// Two launches:
//   1. blend backward   one workgroup per 16x16 tile, one pixel per lane (the forward's quadrant-per-wave
//                       mapping). The records are staged through LDS in batches of 256; z = A dx^2 + B dx dy +
//                       C dy^2 + log2 o is evaluated from (dx, dy) = pixel - 2D mean, and the alpha >= 1/255
//                       skip and the T < 1e-4 stop are the forward's tests on it (the forward takes z from
//                       pixel - mean as well, splat_blend.h; the two differ by the grouping of their FMAs
//                       alone). Two front-to-back walks: the first recomputes what the forward
//                       does not keep (the pixel's T_final and, folded into one number, the whole sum
//                       dL/dC . C + dL/dT_final T_final); the second walks again with the prefix of that
//                       sum, which gives each pair's suffix without a division by 1 - alpha per step, and
//                       reduces the pair's nine partial sums over the wave in DPP, over the four waves
//                       through LDS (per chunk of 64 staged pairs), and adds them to a per-Gaussian
//                       accumulator with one f32 atomic per value per (tile, Gaussian). A wave walks only
//                       the pairs whose alpha box reaches its quadrant, and skips by ballot a pair none of
//                       its lanes evaluates.
//   2. project backward one work-item per Gaussian: the accumulator -> colours, opacity, (2D mean, conic)
//                       and, through conic = cov^-1, cov = A A^T + 0.3 I, A = T R S, T = J W, q / |q|, the
//                       3D mean, the scales and the rotation. Plain f32, one column of A at a time
//                       (splat_backward_math.h says why).
// Float atomics: the sums depend on the arrival order, so the gradients are not bit-reproducible.
//
// Depth supervision rides in the same walks. The expected inverse depth D = sum alpha T / d of a pixel is
// formally a fourth colour channel (1 / d per Gaussian, d the record's view depth, background 0):
//   gs_invdepth_kernel (ptgs_splat_gaussians_invdepth) renders it with the blend backward's first walk;
//   both backward kernels are templated on DEPTH (ptgs_splat_gaussians_backward_depth): the blend adds
//   (1 / d) dL/dD to c . dL/dC and a tenth sum, dL/d(1/d); the projection carries that to the mean through d.
// The DEPTH = false instantiations are the kernels as they were.
//
// The camera pose (ptgs_splat_gaussians_backward_pose): the projection backward already forms what dL/d view is
// made of, per Gaussian; the POSE instantiations sum the twelve shares over the workgroup (DPP, LDS) into one row
// of partials per workgroup, and gs_pose_finish_kernel, the next launch on the stream, adds the rows in float64
// in a fixed order. No atomics: given the accumulator, dL/d view is reproducible. DESIGN.md 5h.
#include <hip/hip_runtime.h>

#include "../../include/ptgs/ptgs.h"
#include "detmath.h"
#include "splat_backward.h"
#include "splat_backward_math.h"
#include "splat_partial_sum.h"

namespace ptgs {

#define GB_BLOCK 256
#define GB_TILE 16
#define GB_CHUNK 64  // staged pairs per reduction round: a wave's ballot; 23 KiB of LDS, 7 waves per SIMD (256:
                     // 50 KiB, 3 waves per SIMD, 0.50 vs 0.37 ms at C2)
#ifndef GB_CHUNK_DEPTH
#define GB_CHUNK_DEPTH GB_CHUNK  // the same for the kernel with the inverse-depth sum (10 sums per pair)
#endif
#define GB_L2E 1.4426950408889634f
#define GB_LN2 0.69314718055994531f
static_assert(GS_BWD_ACC == 9, "2D mean x2, staged quadratic A B C, log2 opacity, colour x3");
static_assert(GS_BWD_ACC_DEPTH == GS_BWD_ACC + 1, "and 1 / d");

// One batch of a tile's list into LDS: work-item tid stages pair base + tid (records, Gaussian ids, quadrant
// masks). INVD: the free fourth word of the third stage entry holds 1 / d (d: the record's view depth, the
// forward's sort key), computed once per staged record; otherwise it is 0. GID: the ids are staged (s_gid).
template <bool INVD, bool GID>
__device__ __forceinline__ void gb_stage_batch(uint32_t tid, uint32_t idx, uint32_t n, uint32_t first,
                                               const uint32_t* vals, const float4* rec, float tx0, float ty0,
                                               float4* s_stage, uint32_t* s_gid, uint8_t* s_mask) {
  if (idx < n) {
    const uint32_t g = vals[first + idx];
    const float4 ga = rec[3 * g], gb = rec[3 * g + 1], gc = rec[3 * g + 2];
    // the record's quadratic and the 2D mean in tile-local pixel coordinates. z is evaluated from
    // (dx, dy) = pixel - mean, as ptgs.h states the function and as the forward's blend evaluates it, not
    // from the quadratic expanded into A ux^2 + ... + F: there terms of several hundred cancel to a z of
    // a few units, an error of 3e-5 in alpha that reached 1.5e-4 relative L2 in the gradients of the
    // quarter of a case's Gaussians with the smallest ones (5e-6, float32 autograd's own error there, in
    // this form). The forward keeps the expansion for its exact quadrant test alone.
    const float gx = ga.x - tx0, gy = ga.y - ty0;
    s_stage[3 * tid] = make_float4(ga.z, ga.w, gb.x, gb.y);
    s_stage[3 * tid + 1] = make_float4(0.0f, 0.0f, gb.z, gb.w);
    s_stage[3 * tid + 2] = make_float4(gc.x, gx, gy, INVD ? 1.0f / gc.w : 0.0f);
    if (GID) s_gid[tid] = g;
    // the forward's quadrant mask of the record's alpha box (gc.y, gc.z: the half-extents outside
    // which alpha < 1/255): bit q = (x half q & 1, y half q >> 1), wave q's pixels
    const float x0 = gx - gc.y, x1 = gx + gc.y, y0 = gy - gc.z, y1 = gy + gc.z;
    const bool xl = x0 <= 7.0f && x1 >= 0.0f, xr = x0 <= 15.0f && x1 >= 8.0f;
    const bool yt = y0 <= 7.0f && y1 >= 0.0f, yb = y0 <= 15.0f && y1 >= 8.0f;
    s_mask[tid] = (uint8_t)((uint32_t)(xl && yt) | ((uint32_t)(xr && yt) << 1) | ((uint32_t)(xl && yb) << 2) |
                            ((uint32_t)(xr && yb) << 3));
  }
}

// The front-to-back walk of a chunk [c0, c1) of the staged batch by one wave, the part that the backward's two
// walks and the inverse-depth render share. gb_walk_begin: the chunk's pairs whose alpha box reaches the
// wave's quadrant (a ballot of the masks; the walk takes them in sorted order, lowest bit first).
// gb_walk_z: z of a staged record at (dx, dy) = pixel - mean; a lane evaluates the pair when
// z >= GB_Z_SKIP (alpha >= 1/255) and it has not stopped. gb_walk_pair: alpha with the 0.99 clamp (0 for a
// lane that does not evaluate the pair), wgt = alpha T, and next_T = T - wgt; the pixel stops before a pair
// whose next_T < GB_T_STOP. (That test and its four assignments stay in the kernels: inside this function they
// cost the backward kernel two VGPRs.)
#define GB_Z_SKIP (-7.9943534f)
#define GB_T_STOP 0.0001f
__device__ __forceinline__ unsigned long long gb_walk_begin(const uint8_t* s_mask, uint32_t c0, uint32_t c1,
                                                            uint32_t wave, uint32_t lane) {
  return __builtin_amdgcn_ballot_w64(c0 + lane < c1 && ((s_mask[c0 + lane] >> wave) & 1u));
}

__device__ __forceinline__ float gb_walk_z(const float4& a, float dx, float dy) {
  return __builtin_fmaf(a.x * dx, dx, __builtin_fmaf(a.y * dx, dy, __builtin_fmaf(a.z * dy, dy, a.w)));
}

struct GbPair {
  float alpha, wgt, next_T;
};

__device__ __forceinline__ GbPair gb_walk_pair(float e, bool valid, float T) {
  GbPair p;
  p.alpha = valid ? fminf(0.99f, e) : 0.0f;
  p.wgt = p.alpha * T;
  p.next_T = T - p.wgt;
  return p;
}

// acc: per Gaussian (d gx, d gy, dA, dB, dC, dL, d r, d g, d b[, d (1/d)]) for the staged z = A dx^2 + B dx dy +
// C dy^2 + L (dx, dy: pixel - 2D mean; A = -a/2 log2e, B = -b log2e, C = -c/2 log2e, L = log2 o).
// DEPTH: the loss also depends on the inverse depth D = sum wgt / d (gs_invdepth_kernel), formally a fourth
// colour channel 1 / d with background 0 and upstream gradient dinv: it joins c . dL/dC, and a tenth sum
// (wgt dinv = dL/d(1/d)) joins the accumulator.
template <bool DEPTH>
__global__ __launch_bounds__(GB_BLOCK) void gs_blend_backward_kernel(uint32_t W, uint32_t H, uint32_t grid_x,
                                                                      const uint2* __restrict__ ranges,
                                                                      const uint32_t* __restrict__ vals,
                                                                      const float4* __restrict__ rec, float bg_r,
                                                                      float bg_g, float bg_b,
                                                                      const float4* __restrict__ dout,
                                                                      const float* __restrict__ dinv,
                                                                      float* __restrict__ acc) {
  constexpr uint32_t ACC = DEPTH ? GS_BWD_ACC_DEPTH : GS_BWD_ACC, CHUNK = DEPTH ? GB_CHUNK_DEPTH : GB_CHUNK;
  static_assert(CHUNK <= 64 && (CHUNK * ACC) % 4 == 0, "a chunk is one ballot; its sums are cleared as float4");
  __shared__ float4 s_stage[3 * GB_BLOCK];  // (A, B, C, L) (-, -, r, g) (b, gx, gy, 1/d): the record, mean tile-local
  __shared__ __attribute__((aligned(16))) float s_red[4][CHUNK * ACC];  // per wave, per pair of a chunk
  __shared__ uint32_t s_gid[GB_BLOCK];
  __shared__ uint8_t s_mask[GB_BLOCK];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t tile = blockIdx.x, tile_y = tile / grid_x, tile_x = tile - tile_y * grid_x;
  const uint2 range = ranges[tile];
  const uint32_t n = range.y - range.x;
  if (n == 0) return;  // (uniform)
  const float tx0 = (float)(tile_x * GB_TILE), ty0 = (float)(tile_y * GB_TILE);
  const uint32_t px = tile_x * GB_TILE + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t py = tile_y * GB_TILE + (wave >> 1) * 8u + (lane >> 3);
  const bool inside = px < W && py < H;
  const float4 go = inside ? dout[(size_t)py * W + px] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  const float gd = (DEPTH && inside) ? dinv[(size_t)py * W + px] : 0.0f;
  const float ux = (float)px - tx0, uy = (float)py - ty0;
  // out.rgb = C + T_final bg, out.a = 1 - T_final: dL/dT_final (D has no background term)
  const float g_tf = ((go.x * bg_r + go.y * bg_g) + go.z * bg_b) - go.w;
  // sum over the pixel's pairs of wgt (c . dL/dC), + T_final dL/dT_final. It and its running prefix are f64
  // sums of the f32 terms: what lies behind a pair is their difference, and deep in a list (T small) that is
  // far smaller than either, so the rounding of f32 sums (eps |total|) swamped the gradients of occluded
  // Gaussians (1.3e-4 relative L2 on the quarter of a case's Gaussians with the smallest opacity gradients)
  double total = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    float T = 1.0f;
    double prefix = 0.0;
    bool done = !inside;
    for (uint32_t base = 0; base < n; base += GB_BLOCK) {
      // (every wave is done with the previous batch's records and sums)
      if (__syncthreads_count(done) == GB_BLOCK) break;
      gb_stage_batch<DEPTH, true>(tid, base + tid, n, range.x, vals, rec, tx0, ty0, s_stage, s_gid, s_mask);
      __syncthreads();
      const uint32_t nb = min((uint32_t)GB_BLOCK, n - base);
      // chunks of CHUNK staged pairs: the wave walks the chunk's pairs whose box reaches its quadrant, and
      // the second walk reduces and sends its sums per chunk (the sums' LDS is what bounds the workgroups per CU)
      for (uint32_t c0 = 0; c0 < nb; c0 += CHUNK) {
        const uint32_t c1 = min(nb, c0 + CHUNK);
        if (pass) {  // the wave's sums of this chunk start at zero: a pair it skips costs nothing more
          if (c0) __syncthreads();  // (the previous chunk's sums have been read)
          float4* z4 = reinterpret_cast<float4*>(s_red[wave]);
          for (uint32_t k = lane; k < CHUNK * ACC / 4; k += 64) z4[k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        unsigned long long todo = gb_walk_begin(s_mask, c0, c1, wave, lane);
        while (todo) {
          if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;  // every pixel of the wave has stopped
          const uint32_t k = (uint32_t)__builtin_ctzll(todo), j = c0 + k;
          todo &= todo - 1ull;
          const float4 a = s_stage[3 * j], b = s_stage[3 * j + 1], c = s_stage[3 * j + 2];
          const float dx = ux - c.y, dy = uy - c.z;
          const float z = gb_walk_z(a, dx, dy);
          bool valid = z >= GB_Z_SKIP && !done;  // alpha >= 1/255
          if (__builtin_amdgcn_ballot_w64(valid) == 0ull) continue;  // no lane of the wave evaluates the pair
          const float e = __builtin_amdgcn_exp2f(z);
          const GbPair p = gb_walk_pair(e, valid, T);
          const float alpha = p.alpha;
          float wgt = p.wgt;
          float test_T = p.next_T;
          if (test_T < GB_T_STOP) {  // this Gaussian would saturate the pixel: stop before it
            done = true;
            valid = false;
            wgt = 0.0f;
            test_T = T;
          }
          float cdot = (b.z * go.x + b.w * go.y) + c.x * go.z;
          if (DEPTH) cdot += c.w * gd;
          if (!pass) {
            total += (double)(wgt * cdot);
          } else {
            prefix += (double)(wgt * cdot);
            if (__builtin_amdgcn_ballot_w64(valid) != 0ull) {  // (uniform: every lane takes part in the sums)
              // dL/dalpha = T (c . dL/dC) - (what lies behind the pair) / (1 - alpha); the 0.99 clamp
              // passes nothing to z
              const float behind = (float)(total - prefix);
              const float dalpha = T * cdot - behind / (1.0f - alpha);
              const float dz = (valid && e <= 0.99f) ? dalpha * alpha * GB_LN2 : 0.0f;
              const float v0 = dz * (-2.0f * a.x * dx - a.y * dy), v1 = dz * (-a.y * dx - 2.0f * a.z * dy);
              const float s0 = gb_wave_sum(v0), s1 = gb_wave_sum(v1);
              const float s2 = gb_wave_sum(dz * dx * dx), s3 = gb_wave_sum(dz * dx * dy), s4 = gb_wave_sum(dz * dy * dy);
              const float s5 = gb_wave_sum(dz);
              const float s6 = gb_wave_sum(wgt * go.x), s7 = gb_wave_sum(wgt * go.y), s8 = gb_wave_sum(wgt * go.z);
              const float s9 = DEPTH ? gb_wave_sum(wgt * gd) : 0.0f;
              if (lane == 63) {
                float* r = &s_red[wave][k * ACC];
                r[0] = s0; r[1] = s1; r[2] = s2; r[3] = s3; r[4] = s4; r[5] = s5; r[6] = s6; r[7] = s7; r[8] = s8;
                if (DEPTH) r[9] = s9;
              }
            }
          }
          T = test_T;
        }
        if (pass) {
          __syncthreads();
          // the four waves' sums, one atomic per value per (tile, Gaussian): consecutive lanes add the
          // consecutive values of a Gaussian; a value no pixel of the tile contributed to is not sent
          for (uint32_t i = tid; i < (c1 - c0) * ACC; i += GB_BLOCK) {
            const float s = (s_red[0][i] + s_red[1][i]) + (s_red[2][i] + s_red[3][i]);
            const uint32_t slot = i / ACC;
            if (s != 0.0f) (void)unsafeAtomicAdd(acc + (size_t)s_gid[c0 + slot] * ACC + (i - slot * ACC), s);
          }
        }
      }
    }
    if (!pass) total += (double)(T * g_tf);
  }
}

// D[pixel] = sum over the pixel's pairs of wgt / d (ptgs_splat_gaussians_invdepth): the backward's first walk
// with the staged 1 / d as the only colour and no background. One workgroup per tile, one pixel per lane; no
// atomics, a fixed order: two runs are bit-equal. Every pixel inside the image is written (0 in an empty tile).
__global__ __launch_bounds__(GB_BLOCK) void gs_invdepth_kernel(uint32_t W, uint32_t H, uint32_t grid_x,
                                                                const uint2* __restrict__ ranges,
                                                                const uint32_t* __restrict__ vals,
                                                                const float4* __restrict__ rec,
                                                                float* __restrict__ out) {
  __shared__ float4 s_stage[3 * GB_BLOCK];
  __shared__ uint8_t s_mask[GB_BLOCK];
  const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
  const uint32_t tile = blockIdx.x, tile_y = tile / grid_x, tile_x = tile - tile_y * grid_x;
  const uint2 range = ranges[tile];
  const uint32_t n = range.y - range.x;
  const float tx0 = (float)(tile_x * GB_TILE), ty0 = (float)(tile_y * GB_TILE);
  const uint32_t px = tile_x * GB_TILE + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t py = tile_y * GB_TILE + (wave >> 1) * 8u + (lane >> 3);
  const bool inside = px < W && py < H;
  const float ux = (float)px - tx0, uy = (float)py - ty0;
  float T = 1.0f, D = 0.0f;
  bool done = !inside;
  for (uint32_t base = 0; base < n; base += GB_BLOCK) {
    if (__syncthreads_count(done) == GB_BLOCK) break;  // (and: every wave is done with the previous batch)
    gb_stage_batch<true, false>(tid, base + tid, n, range.x, vals, rec, tx0, ty0, s_stage, nullptr, s_mask);
    __syncthreads();
    const uint32_t nb = min((uint32_t)GB_BLOCK, n - base);
    for (uint32_t c0 = 0; c0 < nb; c0 += GB_CHUNK) {
      unsigned long long todo = gb_walk_begin(s_mask, c0, min(nb, c0 + GB_CHUNK), wave, lane);
      while (todo) {
        if (__builtin_amdgcn_ballot_w64(!done) == 0ull) break;  // every pixel of the wave has stopped
        const uint32_t j = c0 + (uint32_t)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const float4 a = s_stage[3 * j], c = s_stage[3 * j + 2];
        const float z = gb_walk_z(a, ux - c.y, uy - c.z);
        const bool valid = z >= GB_Z_SKIP && !done;  // alpha >= 1/255
        if (__builtin_amdgcn_ballot_w64(valid) == 0ull) continue;  // no lane of the wave evaluates the pair
        const GbPair p = gb_walk_pair(__builtin_amdgcn_exp2f(z), valid, T);
        float wgt = p.wgt, test_T = p.next_T;
        if (test_T < GB_T_STOP) {  // this Gaussian would saturate the pixel: stop before it
          done = true;
          wgt = 0.0f;
          test_T = T;
        }
        D += wgt * c.w;
        T = test_T;
      }
    }
  }
  if (inside) out[(size_t)py * W + px] = D;
}

struct GbOut {
  float *means, *scales, *rots, *opac, *colors, *means2d, *conics;
};

struct GbProj {
  float m[16];  // the ubo's proj, column-major (POSE: d ph / d view)
};

// DEPTH: the accumulator has the tenth sum, dL/d(1/d), which reaches the mean through d (splat_backward_math.h).
// POSE: the workgroup also leaves the sum of its Gaussians' twelve shares of dL/d view (gs_project_backward_one)
// in partials[blockIdx.x * GS_POSE_K ..]: over the wave with gb_wave_sum, which needs every lane, so this form
// keeps the lanes past n (they and the culled Gaussians add zeros), over the four waves through LDS, and one
// plain store per value. gs_pose_finish_kernel adds the rows. The POSE = false instantiations are the kernels as
// they were (proj and partials are not read).
template <bool DEPTH, bool POSE>
__global__ __launch_bounds__(256) void gs_project_backward_kernel(GbCam cam, const float* __restrict__ means,
                                                                   const float* __restrict__ scales,
                                                                   const float* __restrict__ rots,
                                                                   const float* __restrict__ opac, uint32_t n,
                                                                   const int* __restrict__ radii,
                                                                   const float* __restrict__ acc, GbOut out,
                                                                   GbProj proj, float* __restrict__ partials) {
  constexpr uint32_t ACC = DEPTH ? GS_BWD_ACC_DEPTH : GS_BWD_ACC;
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (!POSE && i >= n) return;
  float dv[GS_POSE_K];
  if (POSE) {
#pragma unroll
    for (int k = 0; k < GS_POSE_K; ++k) dv[k] = 0.0f;
  }
  if (!POSE || i < n) {
    const bool visible = radii[i] > 0;  // (a culled Gaussian is in no tile's list: its sums are zero)
    const float* s9 = acc + (size_t)i * ACC;
    const float dgx = s9[0], dgy = s9[1];
    const float da = -0.5f * GB_L2E * s9[2], db = -GB_L2E * s9[3], dc = -0.5f * GB_L2E * s9[4];
    const float o = opac[i];
    out.opac[i] = (visible && o > 0.0f) ? s9[5] / (o * GB_LN2) : 0.0f;
    out.colors[3 * i] = s9[6];
    out.colors[3 * i + 1] = s9[7];
    out.colors[3 * i + 2] = s9[8];
    if (out.means2d) {
      out.means2d[2 * i] = dgx;
      out.means2d[2 * i + 1] = dgy;
    }
    if (out.conics) {
      out.conics[3 * i] = da;
      out.conics[3 * i + 1] = db;
      out.conics[3 * i + 2] = dc;
    }
    float dm[3] = {0.0f, 0.0f, 0.0f}, dsc[3] = {0.0f, 0.0f, 0.0f}, dq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (visible)
      gs_project_backward_one<DEPTH, POSE>(cam, means + 3 * i, scales + 3 * i, rots + 4 * i, dgx, dgy, da, db, dc, dm,
                                           dsc, dq, DEPTH ? s9[GS_BWD_ACC] : 0.0f, proj.m, dv);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      out.means[3 * i + k] = dm[k];
      out.scales[3 * i + k] = dsc[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) out.rots[4 * i + k] = dq[k];
  }
  if (POSE) {
    __shared__ float s_pose[4][GS_POSE_K];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
#pragma unroll
    for (int k = 0; k < GS_POSE_K; ++k) {  // (every lane of the workgroup is here)
      const float s = gb_wave_sum(dv[k]);
      if (lane == 63) s_pose[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < GS_POSE_K)
      partials[(size_t)blockIdx.x * GS_POSE_K + threadIdx.x] =
          (s_pose[0][threadIdx.x] + s_pose[1][threadIdx.x]) + (s_pose[2][threadIdx.x] + s_pose[3][threadIdx.x]);
  }
}

// The second stage of dL/d view: one workgroup adds the `rows` partial rows of this call in float64, in a fixed
// order (splat_partial_sum.h), and writes the 16 floats column-major like ptgs_ubo.view: entry c * 4 + r =
// dL/d view[r][c]; row 3 (held at (0, 0, 0, 1)) is exactly 0. rows == 0: sixteen zeros.
__global__ __launch_bounds__(GS_PSUM_BLOCK) void gs_pose_finish_kernel(const float* __restrict__ partials, uint32_t rows,
                                                                        float* __restrict__ dview) {
  __shared__ double s_seg[GS_POSE_K * GS_PSUM_BLOCK];
  const double sum = gs_sum_partial_rows<GS_POSE_K, GS_PSUM_BLOCK>(partials, rows, s_seg);
  const uint32_t t = threadIdx.x;
  if (t < GS_POSE_K) dview[(t & 3u) * 4u + (t >> 2)] = (float)sum;  // partial k = r * 4 + c
  if (t < 4) dview[t * 4u + 3u] = 0.0f;
}

template <bool DEPTH, bool POSE>
static hipError_t gb_launch_project(const SplatFrame& f, const GbCam& cam, const ptgs_gaussians* g, const float* acc,
                                    const GbOut& out, const GbProj& proj, float* partials, hipStream_t s) {
  hipLaunchKernelGGL((gs_project_backward_kernel<DEPTH, POSE>), dim3((f.n + 255u) / 256u), dim3(256), 0, s, cam,
                     g->means, g->scales, g->rotations, g->opacities, f.n, f.radii, acc, out, proj, partials);
  return hipGetLastError();
}

hipError_t splat_gaussians_backward(const SplatFrame& f, float* acc, const ptgs_gaussians* g, const float* view,
                                    const float* mvp, float p00, float p11, const float bg[3], const float* dL_dout,
                                    const float* dL_dinvdepth, const ptgs_gaussian_grads* grads, hipStream_t s,
                                    const float* proj, float* pose_partials, float* dL_dview) {
  const uint32_t n = f.n;
  const bool depth = dL_dinvdepth != nullptr, pose = dL_dview != nullptr;
  hipError_t e;
  if ((e = hipMemsetAsync(acc, 0, (size_t)n * (depth ? GS_BWD_ACC_DEPTH : GS_BWD_ACC) * 4, s))) return e;
  GbCam cam;
  GbProj pr = {};
  for (int k = 0; k < 16; ++k) {
    cam.view[k] = view[k];
    cam.mvp[k] = mvp[k];
    if (pose) pr.m[k] = proj[k];
  }
  cam.fx = p00 * (float)f.W * 0.5f;
  cam.fy = p11 * (float)f.H * 0.5f;
  cam.limx = 1.3f * (1.0f / p00);
  cam.limy = 1.3f * (1.0f / (p11 < 0.0f ? -p11 : p11));
  cam.W = f.W;
  cam.H = f.H;
  cam.grid_x = (f.W + GB_TILE - 1) / GB_TILE;
  if (depth)
    hipLaunchKernelGGL(gs_blend_backward_kernel<true>, dim3(f.tiles), dim3(GB_BLOCK), 0, s, f.W, f.H, cam.grid_x,
                       f.ranges, f.sorted_values, f.rec, bg[0], bg[1], bg[2], (const float4*)dL_dout, dL_dinvdepth, acc);
  else
    hipLaunchKernelGGL(gs_blend_backward_kernel<false>, dim3(f.tiles), dim3(GB_BLOCK), 0, s, f.W, f.H, cam.grid_x,
                       f.ranges, f.sorted_values, f.rec, bg[0], bg[1], bg[2], (const float4*)dL_dout,
                       (const float*)nullptr, acc);
  if ((e = hipGetLastError())) return e;
  const GbOut out = {grads->means, grads->scales, grads->rotations, grads->opacities, grads->colors, grads->means2d,
                     grads->conics};
  if (!pose)
    return depth ? gb_launch_project<true, false>(f, cam, g, acc, out, pr, nullptr, s)
                 : gb_launch_project<false, false>(f, cam, g, acc, out, pr, nullptr, s);
  // every row the finish reads is written by this call's projection launch: (n + 255) / 256 of them
  if ((e = depth ? gb_launch_project<true, true>(f, cam, g, acc, out, pr, pose_partials, s)
                 : gb_launch_project<false, true>(f, cam, g, acc, out, pr, pose_partials, s)))
    return e;
  return splat_pose_finish(pose_partials, (n + 255u) / 256u, dL_dview, s);
}

hipError_t splat_pose_finish(const float* partials, uint32_t rows, float* dL_dview, hipStream_t s) {
  hipLaunchKernelGGL(gs_pose_finish_kernel, dim3(1), dim3(GS_PSUM_BLOCK), 0, s, partials, rows, dL_dview);
  return hipGetLastError();
}

hipError_t splat_gaussians_invdepth(const SplatFrame& f, float* out, hipStream_t s) {
  hipLaunchKernelGGL(gs_invdepth_kernel, dim3(f.tiles), dim3(GB_BLOCK), 0, s, f.W, f.H, (f.W + GB_TILE - 1) / GB_TILE,
                     f.ranges, f.sorted_values, f.rec, out);
  return hipGetLastError();
}

}  // namespace ptgs
