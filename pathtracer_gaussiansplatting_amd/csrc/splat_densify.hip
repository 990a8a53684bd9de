// splat_densify.hip — densify_and_prune of a 3DGS training run (Kerbl et al.'s trainer) on the device: the
// statistic of each view, the plan (what becomes of every Gaussian and where its rows go) and the gather that
// writes the new parameter arrays and optimizer moments. The contract is in include/ptgs/ptgs.h, the
// per-Gaussian arithmetic in splat_densify_math.h (host / device).
//
// Plan. gs_densify_decide_kernel evaluates the rule once per source Gaussian into one byte (DN_* bits) and
// counts each bit per block; gs_densify_scan_kernel turns the block counts into exclusive offsets (one
// workgroup walking them 256 at a time with a carry) and the five totals; after the host has read the totals
// and grown the map, gs_densify_scatter_kernel repeats the in-block ranks from the bytes and writes
// source[]: survivors at [0, A), clones at [A, A + B), first children at [A + B, A + B + C), second children
// at [A + B + C, A + B + 2 C), each by source index. A block covers DN_BLOCK = 2048 Gaussians: 8 rounds of 256,
// Gaussian base + 256 j + t in round j, so loads are lane-contiguous; a bit's rank inside the block is the
// count of the earlier (round, wave) cells (32 of them, in LDS) plus the wave64 ballot's bits below the lane.
//
// Apply. One launch for every array. A work-item owns four output elements, 256 apart: floats, or float4s where
// the row width is a multiple of 4 floats and both bases are 16-byte aligned (48-float SH rows and their moments:
// 12 dwordx4 per row). Consecutive work-items write consecutive addresses, and the elements of one row read one
// contiguous source row through source[row]; each array owns a range of blocks (a table in the kernel
// arguments, found per block by a scalar search). Bytes per output Gaussian: 4 (source map) + 8 per float of
// row width (read + write; a zeroed row of a new Gaussian is not read), + 52 for a child's mean.
#include "splat_densify.h"

#include <type_traits>

#include "dev_buf.h"
#include "splat_densify_math.h"

namespace ptgs {
namespace {

constexpr uint32_t DN_WG = 256, DN_ROUNDS = 8, DN_WAVES = DN_WG / 64;
constexpr uint32_t DN_BLOCK = DN_WG * DN_ROUNDS;  // Gaussians per workgroup of the plan
constexpr uint32_t DN_CELLS = DN_ROUNDS * DN_WAVES;

__global__ __launch_bounds__(256) void gs_densify_accumulate_kernel(const float* __restrict__ g2d,
                                                                   const int32_t* __restrict__ radii, uint32_t n,
                                                                   uint32_t W, uint32_t H, float* accum, float* denom,
                                                                   float* max_radii) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int32_t r = radii[i];
  if (r <= 0) return;
  float a = accum[i], d = denom[i], m = max_radii[i];
  dn_accumulate_one(g2d[2 * (size_t)i], g2d[2 * (size_t)i + 1], r, W, H, &a, &d, &m);
  accum[i] = a;
  denom[i] = d;
  max_radii[i] = m;
}

// per fate bit k and (round, wave) cell: the number of set bits, from the wave's ballot
__device__ __forceinline__ void dn_count_cells(const uint32_t f, uint32_t j, uint32_t (*cells)[DN_CELLS]) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < DN_FATES; ++k) {
    const unsigned long long m = __ballot((f >> k) & 1u);
    if (lane == 0) cells[k][j * DN_WAVES + wave] = (uint32_t)__popcll(m);
  }
}

__global__ __launch_bounds__(DN_WG) void gs_densify_decide_kernel(const float* __restrict__ scales,
                                                                 const float* __restrict__ opacities,
                                                                 const float* __restrict__ accum,
                                                                 const float* __restrict__ denom,
                                                                 const float* __restrict__ max_radii, uint32_t n,
                                                                 ptgs_densify_params p, uint8_t* __restrict__ fate,
                                                                 uint32_t* __restrict__ block_sums) {
  __shared__ uint32_t cells[DN_FATES][DN_CELLS];
  const uint32_t t = threadIdx.x, base = blockIdx.x * DN_BLOCK;  // (n <= 2^30: no overflow)
  for (uint32_t j = 0; j < DN_ROUNDS; ++j) {
    const uint32_t i = base + j * DN_WG + t;
    uint32_t f = 0;
    if (i < n) {
      const float s[3] = {scales[3 * (size_t)i], scales[3 * (size_t)i + 1], scales[3 * (size_t)i + 2]};
      f = dn_decide(p, s, opacities[i], accum[i], denom[i], max_radii[i]);
      fate[i] = (uint8_t)f;
    }
    dn_count_cells(f, j, cells);
  }
  __syncthreads();
  if (t < (uint32_t)DN_FATES) {
    uint32_t sum = 0;
    for (uint32_t c = 0; c < DN_CELLS; ++c) sum += cells[t][c];
    block_sums[(size_t)blockIdx.x * DN_FATES + t] = sum;
  }
}

// block_sums[b][k] becomes the exclusive prefix over the blocks, totals[k] the sum; one workgroup
__global__ __launch_bounds__(DN_WG) void gs_densify_scan_kernel(uint32_t* block_sums, uint32_t nb, uint32_t* totals) {
  __shared__ uint32_t sc[DN_FATES][DN_WG];
  const uint32_t t = threadIdx.x;
  uint32_t carry[DN_FATES];
#pragma unroll
  for (int k = 0; k < DN_FATES; ++k) carry[k] = 0;
  for (uint32_t c0 = 0; c0 < nb; c0 += DN_WG) {
    const uint32_t b = c0 + t;
    uint32_t v[DN_FATES];
#pragma unroll
    for (int k = 0; k < DN_FATES; ++k) {
      v[k] = b < nb ? block_sums[(size_t)b * DN_FATES + k] : 0u;
      sc[k][t] = v[k];
    }
    __syncthreads();
    for (uint32_t off = 1; off < DN_WG; off <<= 1) {
      uint32_t add[DN_FATES];
#pragma unroll
      for (int k = 0; k < DN_FATES; ++k) add[k] = t >= off ? sc[k][t - off] : 0u;
      __syncthreads();
#pragma unroll
      for (int k = 0; k < DN_FATES; ++k) sc[k][t] += add[k];
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < DN_FATES; ++k) {
      if (b < nb) block_sums[(size_t)b * DN_FATES + k] = carry[k] + (sc[k][t] - v[k]);
      carry[k] += sc[k][DN_WG - 1];
    }
    __syncthreads();
  }
  if (t == 0) {
#pragma unroll
    for (int k = 0; k < DN_FATES; ++k) totals[k] = carry[k];
  }
}

__global__ __launch_bounds__(DN_WG) void gs_densify_scatter_kernel(const uint8_t* __restrict__ fate, uint32_t n,
                                                                  const uint32_t* __restrict__ block_offs,
                                                                  const uint32_t* __restrict__ totals,
                                                                  uint32_t* __restrict__ source) {
  __shared__ uint32_t cells[DN_FATES][DN_CELLS];
  const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, base = blockIdx.x * DN_BLOCK;
  uint32_t f[DN_ROUNDS];
#pragma unroll
  for (uint32_t j = 0; j < DN_ROUNDS; ++j) {
    const uint32_t i = base + j * DN_WG + t;
    f[j] = i < n ? (uint32_t)fate[i] : 0u;
    dn_count_cells(f[j], j, cells);
  }
  __syncthreads();
  if (t < 3) {  // exclusive prefix of the 32 cells of KEEP, CLONE, CHILDREN
    uint32_t run = 0;
    for (uint32_t c = 0; c < DN_CELLS; ++c) {
      const uint32_t v = cells[t][c];
      cells[t][c] = run;
      run += v;
    }
  }
  __syncthreads();
  const uint32_t A = totals[0], B = totals[1], C = totals[2];
  const uint32_t first[3] = {block_offs[(size_t)blockIdx.x * DN_FATES], A + block_offs[(size_t)blockIdx.x * DN_FATES + 1],
                             A + B + block_offs[(size_t)blockIdx.x * DN_FATES + 2]};
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (uint32_t j = 0; j < DN_ROUNDS; ++j) {
    const uint32_t i = base + j * DN_WG + t;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
      const unsigned long long m = __ballot((f[j] >> k) & 1u);
      if ((f[j] >> k) & 1u) {
        const uint32_t at = first[k] + cells[k][j * DN_WAVES + wave] + (uint32_t)__popcll(m & below);
        if (k < 2) {
          source[at] = i | (k << DN_KIND_SHIFT);
        } else {
          source[at] = i | (DN_KIND_CHILD0 << DN_KIND_SHIFT);
          source[at + C] = i | (DN_KIND_CHILD1 << DN_KIND_SHIFT);
        }
      }
    }
  }
}

// ---- apply ----
constexpr uint32_t DN_SEG_MAX = PTGS_DENSIFY_MAX_ROWS + 2;  // the rows, the means, the log-scales
constexpr uint32_t DN_SEG_ZERO_NEW = 1u, DN_SEG_VEC4 = 2u, DN_SEG_MEANS = 4u, DN_SEG_LOG_SCALES = 8u;

struct DnSeg {
  const float* src;
  float* dst;
  uint32_t units;        // elements per row: floats, or float4s with DN_SEG_VEC4
  uint32_t flags;
  uint32_t first_block;  // the segment's blocks are [first_block, the next segment's)
  uint32_t pad;
};
struct DnApply {
  DnSeg seg[DN_SEG_MAX];
  uint32_t nseg, n, n_out;
  const uint32_t* source;
  const float *means, *rotations, *scales, *noise;
};

constexpr uint32_t DN_APPLY_WG = 256, DN_APPLY_BATCH = 4;  // elements in flight per work-item
constexpr uint32_t DN_APPLY_BLOCK = DN_APPLY_WG * DN_APPLY_BATCH;  // elements per workgroup

// One workgroup: DN_APPLY_BLOCK consecutive elements of one array, element first + 256 j + t in batch j (lane-
// contiguous stores). The map entries of the whole batch are loaded first, then the rows' elements, then the
// stores, so the two dependent loads of each element overlap with the others'.
// WIDE: a segment has 2^32 elements or more (64-bit element index and division)
template <bool WIDE>
__global__ __launch_bounds__(DN_APPLY_WG) void gs_densify_apply_kernel(const DnApply a) {
  const uint32_t b = blockIdx.x;
  uint32_t k = 0;
  for (uint32_t j = 1; j < a.nseg; ++j)
    if (b >= a.seg[j].first_block) k = j;  // (uniform in the block)
  const float* __restrict__ src = a.seg[k].src;
  float* __restrict__ dst = a.seg[k].dst;
  const uint32_t units = a.seg[k].units, flags = a.seg[k].flags;
  typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type idx_t;
  const idx_t count = (idx_t)a.n_out * units;
  const idx_t first = (idx_t)(b - a.seg[k].first_block) * DN_APPLY_BLOCK + threadIdx.x;
  uint32_t sv[DN_APPLY_BATCH], col[DN_APPLY_BATCH];
#pragma unroll
  for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j) {
    const idx_t e = first + j * DN_APPLY_WG;
    sv[j] = 0;
    col[j] = 0;
    if (e < count) {
      const uint32_t o = (uint32_t)(e / units);
      col[j] = (uint32_t)(e - (idx_t)o * units);
      sv[j] = a.source[o];
    }
  }
  const bool zero_new = flags & DN_SEG_ZERO_NEW;
  if (flags & DN_SEG_VEC4) {
    float4 v[DN_APPLY_BATCH];
#pragma unroll
    for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j) {
      const uint32_t kind = sv[j] >> DN_KIND_SHIFT, i = sv[j] & DN_INDEX_MASK;
      v[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      if (first + j * DN_APPLY_WG < count && !(zero_new && kind != DN_KIND_ORIGINAL))
        v[j] = reinterpret_cast<const float4*>(src)[(size_t)i * units + col[j]];
    }
#pragma unroll
    for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j)
      if (first + j * DN_APPLY_WG < count) reinterpret_cast<float4*>(dst)[first + j * DN_APPLY_WG] = v[j];
    return;
  }
  float v[DN_APPLY_BATCH];
#pragma unroll
  for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j) {
    const uint32_t kind = sv[j] >> DN_KIND_SHIFT, i = sv[j] & DN_INDEX_MASK;
    v[j] = 0.0f;
    if (first + j * DN_APPLY_WG < count && !(zero_new && kind != DN_KIND_ORIGINAL)) v[j] = src[(size_t)i * units + col[j]];
  }
  if (flags & (DN_SEG_LOG_SCALES | DN_SEG_MEANS)) {  // what a child changes
#pragma unroll
    for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j) {
      const uint32_t kind = sv[j] >> DN_KIND_SHIFT, i = sv[j] & DN_INDEX_MASK;
      if (first + j * DN_APPLY_WG < count && kind >= DN_KIND_CHILD0) {
        if (flags & DN_SEG_LOG_SCALES) {
          v[j] = v[j] - DN_LOG_SPLIT;
        } else {
          const float* z = a.noise + ((size_t)(kind - DN_KIND_CHILD0) * a.n + i) * 3;
          v[j] = dn_child_mean_component(a.means + (size_t)i * 3, a.rotations + (size_t)i * 4,
                                         a.scales + (size_t)i * 3, z, (int)col[j]);
        }
      }
    }
  }
#pragma unroll
  for (uint32_t j = 0; j < DN_APPLY_BATCH; ++j)
    if (first + j * DN_APPLY_WG < count) dst[first + j * DN_APPLY_WG] = v[j];
}

// room for `need` elements of T, a quarter more when the buffer has to grow
template <typename T>
hipError_t dn_ensure(DevBuf& b, size_t need) {
  return b.ensure(need * sizeof(T), need / 4 * sizeof(T));
}

}  // namespace

struct DensifyWorkspace {
  DevBuf fate;        // uint8_t per source Gaussian
  DevBuf block_sums;  // uint32_t [blocks][DN_FATES]: counts, then exclusive offsets
  DevBuf totals;      // DN_FATES words
  DevBuf source;      // uint32_t per output Gaussian
  bool valid = false;  // the latest plan
  uint32_t n = 0, n_out = 0;
};

DensifyWorkspace* densify_workspace_create() { return new DensifyWorkspace(); }

void densify_workspace_destroy(DensifyWorkspace* ws) { delete ws; }

hipError_t densify_accumulate(const float* g2d, const int32_t* radii, uint32_t n, uint32_t W, uint32_t H, float* accum,
                              float* denom, float* max_radii, hipStream_t s) {
  const uint32_t blocks = (uint32_t)(((uint64_t)n + 255) / 256);
  gs_densify_accumulate_kernel<<<blocks, 256, 0, s>>>(g2d, radii, n, W, H, accum, denom, max_radii);
  return hipGetLastError();
}

void densify_plan_empty(DensifyWorkspace* ws) {
  ws->valid = true;
  ws->n = ws->n_out = 0;
}

bool densify_last_plan(const DensifyWorkspace* ws, uint32_t* n, uint32_t* n_out) {
  if (!ws->valid) return false;
  *n = ws->n;
  *n_out = ws->n_out;
  return true;
}

hipError_t densify_plan(DensifyWorkspace* ws, const float* scales, const float* opacities, const float* accum,
                        const float* denom, const float* max_radii, uint32_t n, const ptgs_densify_params& p,
                        ptgs_densify_counts* out, hipStream_t s) {
  ws->valid = false;
  if (n == 0 || n > DN_MAX_N) return hipErrorInvalidValue;
  const uint32_t nb = (n + DN_BLOCK - 1) / DN_BLOCK;
  hipError_t e;
  if ((e = dn_ensure<uint8_t>(ws->fate, (size_t)n)) != hipSuccess) return e;
  if ((e = dn_ensure<uint32_t>(ws->block_sums, (size_t)nb * DN_FATES)) != hipSuccess) return e;
  if ((e = dn_ensure<uint32_t>(ws->totals, (size_t)DN_FATES)) != hipSuccess) return e;
  gs_densify_decide_kernel<<<nb, DN_WG, 0, s>>>(scales, opacities, accum, denom, max_radii, n, p,
                                                ws->fate.as<uint8_t>(), ws->block_sums.as<uint32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  gs_densify_scan_kernel<<<1, DN_WG, 0, s>>>(ws->block_sums.as<uint32_t>(), nb, ws->totals.as<uint32_t>());
  if ((e = hipGetLastError()) != hipSuccess) return e;
  uint32_t h[DN_FATES] = {};
  if ((e = hipMemcpyAsync(h, ws->totals.p, sizeof(h), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  const uint64_t total = (uint64_t)h[0] + h[1] + 2ull * h[2];  // (<= 2 n <= 2^31)
  if (total > 0xFFFFFFFFull) return hipErrorInvalidValue;
  if (total) {
    if ((e = dn_ensure<uint32_t>(ws->source, (size_t)total)) != hipSuccess) return e;
    gs_densify_scatter_kernel<<<nb, DN_WG, 0, s>>>(ws->fate.as<uint8_t>(), n, ws->block_sums.as<uint32_t>(),
                                                   ws->totals.as<uint32_t>(), ws->source.as<uint32_t>());
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  out->survivors = h[0];
  out->clones = h[1];
  out->split_sources = h[2];
  out->pruned_originals = h[3];
  out->pruned_children = 2u * h[4];
  out->total = (uint32_t)total;
  ws->valid = true;
  ws->n = n;
  ws->n_out = (uint32_t)total;
  return hipSuccess;
}

hipError_t densify_apply(const DensifyWorkspace* ws, const float* means, const float* log_scales,
                         const float* rotations, const float* scales, const float* noise, float* means_out,
                         float* log_scales_out, const ptgs_densify_rows* rows, uint32_t n_rows, uint32_t* source_out,
                         hipStream_t s) {
  if (!ws->valid || ws->n_out == 0 || n_rows > PTGS_DENSIFY_MAX_ROWS) return hipErrorInvalidValue;
  DnApply a{};
  a.n = ws->n;
  a.n_out = ws->n_out;
  a.source = ws->source.as<uint32_t>();
  a.means = means;
  a.rotations = rotations;
  a.scales = scales;
  a.noise = noise;
  uint64_t blocks = 0;
  bool wide = false;
  auto add = [&](const float* src, float* dst, uint32_t width, uint32_t flags) {
    DnSeg& g = a.seg[a.nseg++];
    g.src = src;
    g.dst = dst;
    g.units = width;
    g.flags = flags;
    if (!(flags & (DN_SEG_MEANS | DN_SEG_LOG_SCALES)) && width % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0) {
      g.units = width / 4;
      g.flags |= DN_SEG_VEC4;
    }
    const uint64_t elems = (uint64_t)a.n_out * g.units;
    wide = wide || elems + DN_APPLY_BLOCK > 0xFFFFFFFFull;  // (a block's last index must not wrap)
    g.first_block = (uint32_t)(blocks < 0xFFFFFFFFull ? blocks : 0xFFFFFFFFull);
    blocks += (elems + DN_APPLY_BLOCK - 1) / DN_APPLY_BLOCK;
  };
  add(means, means_out, 3, DN_SEG_MEANS);
  add(log_scales, log_scales_out, 3, DN_SEG_LOG_SCALES);
  for (uint32_t k = 0; k < n_rows; ++k) add(rows[k].src, rows[k].dst, rows[k].width, rows[k].zero_new ? DN_SEG_ZERO_NEW : 0u);
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  if (wide)
    gs_densify_apply_kernel<true><<<(uint32_t)blocks, DN_APPLY_WG, 0, s>>>(a);
  else
    gs_densify_apply_kernel<false><<<(uint32_t)blocks, DN_APPLY_WG, 0, s>>>(a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (source_out)
    e = hipMemcpyAsync(source_out, ws->source.p, (size_t)ws->n_out * sizeof(uint32_t), hipMemcpyDeviceToDevice, s);
  return e;
}

}  // namespace ptgs
