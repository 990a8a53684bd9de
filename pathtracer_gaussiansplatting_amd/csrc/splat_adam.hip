// splat_adam.hip — the step that changes the parameters of a 3DGS training run: Adam over every per-Gaussian
// array in one launch, skipping the Gaussians the view did not see (the sparse Adam of Kerbl et al.'s trainer,
// after Taming-3DGS), and the opacity reset. The contract is in include/ptgs/ptgs.h, the per-element arithmetic
// in splat_adam_math.h (host / device).
//
// Step. The shape of gs_densify_apply_kernel (splat_densify.hip): the rows are a table of segments in the kernel
// arguments, each owning a range of blocks that a block finds by a scalar search. A work-item owns four
// elements, 256 apart: floats, or float4s where the row width is a multiple of 4 floats and the row's four bases
// are 16-byte aligned (48-float SH rows: 12 dwordx4 per array and row). A float4 lies inside one Gaussian's row,
// so an element needs one radius; a masked-out element loads nothing else and stores nothing. The radii of the
// whole batch are loaded first, then g, p, m, v of the elements that step, then the arithmetic, then the
// stores, so the dependent loads overlap. Consecutive work-items touch consecutive addresses. No LDS, no
// atomics. Bytes per float that steps: 28 (g, p, m, v read; p, m, v written); per element: 4 (the radius).
#include "splat_adam.h"

#include <type_traits>

#include "splat_adam_math.h"

namespace ptgs {
namespace {

struct AdSeg {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  uint32_t units;        // elements per row: floats, or float4s with vec4
  uint32_t head;         // in floats
  uint32_t first_block;  // the segment's blocks are [first_block, the next segment's)
  uint32_t vec4;
  float ss, ss_head;
};
struct AdStep {
  AdSeg seg[PTGS_ADAM_MAX_ROWS];
  uint32_t nseg, n;
  const int32_t* radii;
  AdamScalars s;
};

constexpr uint32_t AD_WG = 256, AD_BATCH = 4;      // elements in flight per work-item
constexpr uint32_t AD_BLOCK = AD_WG * AD_BATCH;    // elements per workgroup

// MASKED: a Gaussian steps only where radii[i] > 0. WIDE: a segment has 2^32 elements or more (64-bit element
// index and division).
template <bool MASKED, bool WIDE>
__global__ __launch_bounds__(AD_WG) void gs_adam_step_kernel(const AdStep a) {
  const uint32_t b = blockIdx.x;
  uint32_t k = 0;
  for (uint32_t j = 1; j < a.nseg; ++j)
    if (b >= a.seg[j].first_block) k = j;  // (uniform in the block)
  float* __restrict__ P = a.seg[k].param;
  const float* __restrict__ G = a.seg[k].grad;
  float* __restrict__ M = a.seg[k].exp_avg;
  float* __restrict__ V = a.seg[k].exp_avg_sq;
  const uint32_t units = a.seg[k].units, head = a.seg[k].head;
  const float ss = a.seg[k].ss, ss_head = a.seg[k].ss_head;
  const AdamScalars s = a.s;
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type idx_t;
  const idx_t count = (idx_t)a.n * units;
  const idx_t first = (idx_t)(b - a.seg[k].first_block) * AD_BLOCK + threadIdx.x;
  bool on[AD_BATCH];
  uint32_t col[AD_BATCH];
#pragma unroll
  for (uint32_t j = 0; j < AD_BATCH; ++j) {
    const idx_t e = first + j * AD_WG;
    on[j] = e < count;
    col[j] = 0;
    if (on[j]) {
      const uint32_t o = (uint32_t)(e / units);
      col[j] = (uint32_t)(e - (idx_t)o * units);
      if (MASKED) on[j] = a.radii[o] > 0;
    }
  }
  if (a.seg[k].vec4) {
    float4 g[AD_BATCH], p[AD_BATCH], m[AD_BATCH], v[AD_BATCH];
#pragma unroll
    for (uint32_t j = 0; j < AD_BATCH; ++j) {
      const idx_t e = first + j * AD_WG;
      g[j] = p[j] = m[j] = v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (on[j]) {
        g[j] = reinterpret_cast<const float4*>(G)[e];
        p[j] = reinterpret_cast<const float4*>(P)[e];
        m[j] = reinterpret_cast<const float4*>(M)[e];
        v[j] = reinterpret_cast<const float4*>(V)[e];
      }
    }
#pragma unroll
    for (uint32_t j = 0; j < AD_BATCH; ++j) {
      if (!on[j]) continue;
      const uint32_t c = col[j] * 4u;  // the column of .x: only a row's first float4s can mix the two rates
      adam_update(s, c < head ? ss_head : ss, g[j].x, &p[j].x, &m[j].x, &v[j].x);
      adam_update(s, c + 1u < head ? ss_head : ss, g[j].y, &p[j].y, &m[j].y, &v[j].y);
      adam_update(s, c + 2u < head ? ss_head : ss, g[j].z, &p[j].z, &m[j].z, &v[j].z);
      adam_update(s, c + 3u < head ? ss_head : ss, g[j].w, &p[j].w, &m[j].w, &v[j].w);
    }
#pragma unroll
    for (uint32_t j = 0; j < AD_BATCH; ++j) {
      const idx_t e = first + j * AD_WG;
      if (on[j]) {
        reinterpret_cast<float4*>(P)[e] = p[j];
        reinterpret_cast<float4*>(M)[e] = m[j];
        reinterpret_cast<float4*>(V)[e] = v[j];
      }
    }
    return;
  }
  float g[AD_BATCH], p[AD_BATCH], m[AD_BATCH], v[AD_BATCH];
#pragma unroll
  for (uint32_t j = 0; j < AD_BATCH; ++j) {
    const idx_t e = first + j * AD_WG;
    g[j] = p[j] = m[j] = v[j] = 0.0f;
    if (on[j]) {
      g[j] = G[e];
      p[j] = P[e];
      m[j] = M[e];
      v[j] = V[e];
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < AD_BATCH; ++j)
    if (on[j]) adam_update(s, col[j] < head ? ss_head : ss, g[j], &p[j], &m[j], &v[j]);
#pragma unroll
  for (uint32_t j = 0; j < AD_BATCH; ++j) {
    const idx_t e = first + j * AD_WG;
    if (on[j]) {
      P[e] = p[j];
      M[e] = m[j];
      V[e] = v[j];
    }
  }
}

constexpr uint32_t AD_RESET_MAX_BLOCKS = 1u << 16;

__global__ __launch_bounds__(256) void gs_opacity_reset_kernel(float* __restrict__ logits, uint32_t n, float cap,
                                                               float* __restrict__ exp_avg,
                                                               float* __restrict__ exp_avg_sq) {
  const size_t stride = (size_t)gridDim.x * 256u;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    logits[i] = adam_reset_logit(logits[i], cap);
    if (exp_avg) exp_avg[i] = 0.0f;
    if (exp_avg_sq) exp_avg_sq[i] = 0.0f;
  }
}

}  // namespace

hipError_t adam_step(uint32_t n, const ptgs_adam_rows* rows, uint32_t n_rows, const ptgs_adam_params& params,
                     const int32_t* radii, hipStream_t s) {
  if (n == 0 || n_rows == 0 || n_rows > PTGS_ADAM_MAX_ROWS) return hipErrorInvalidValue;
  AdStep a{};
  float bc1 = 1.0f;
  a.s = adam_scalars(params, &bc1);
  a.n = n;
  a.nseg = n_rows;
  a.radii = radii;
  uint64_t blocks = 0;
  bool wide = false;
  for (uint32_t k = 0; k < n_rows; ++k) {
    const ptgs_adam_rows& r = rows[k];
    AdSeg& g = a.seg[k];
    g.param = r.param;
    g.grad = r.grad;
    g.exp_avg = r.exp_avg;
    g.exp_avg_sq = r.exp_avg_sq;
    g.head = r.head;
    g.ss = adam_step_size(r.lr, bc1);
    g.ss_head = adam_step_size(r.lr_head, bc1);
    const uintptr_t bases = (uintptr_t)r.param | (uintptr_t)r.grad | (uintptr_t)r.exp_avg | (uintptr_t)r.exp_avg_sq;
    g.vec4 = r.width % 4 == 0 && (bases & 15u) == 0;
    g.units = g.vec4 ? r.width / 4 : r.width;
    const uint64_t elems = (uint64_t)n * g.units;
    wide = wide || elems + AD_BLOCK > 0xFFFFFFFFull;  // (a block's last index must not wrap)
    g.first_block = (uint32_t)(blocks < 0xFFFFFFFFull ? blocks : 0xFFFFFFFFull);
    blocks += (elems + AD_BLOCK - 1) / AD_BLOCK;
  }
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid((uint32_t)blocks), wg(AD_WG);
  if (radii) {
    if (wide)
      gs_adam_step_kernel<true, true><<<grid, wg, 0, s>>>(a);
    else
      gs_adam_step_kernel<true, false><<<grid, wg, 0, s>>>(a);
  } else {
    if (wide)
      gs_adam_step_kernel<false, true><<<grid, wg, 0, s>>>(a);
    else
      gs_adam_step_kernel<false, false><<<grid, wg, 0, s>>>(a);
  }
  return hipGetLastError();
}

hipError_t opacity_reset(float* logits, uint32_t n, float cap, float* exp_avg, float* exp_avg_sq, hipStream_t s) {
  const uint64_t need = ((uint64_t)n + 255) / 256;
  const uint32_t blocks = (uint32_t)(need < AD_RESET_MAX_BLOCKS ? need : AD_RESET_MAX_BLOCKS);
  gs_opacity_reset_kernel<<<blocks, 256, 0, s>>>(logits, n, cap, exp_avg, exp_avg_sq);
  return hipGetLastError();
}

}  // namespace ptgs
