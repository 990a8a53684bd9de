// splat_train.hip — what a 3DGS training loop needs on the device besides its stages (splat.hip, splat_backward.hip,
// splat_sh.hip, splat_loss.hip, splat_adam.hip, splat_densify.hip): the leaves of a checkpoint from the Gaussians
// ptgs_gaussians_from_points initialises, and the squared error that PSNR is computed from. The contract is in
// include/ptgs/ptgs.h, the per-element arithmetic in splat_train_math.h (host / device).
//
// Checkpoint init. One launch over the 3N + N + N ROW output floats taken as one range (ROW = 3 (d + 1)^2): a
// work-item owns one output element and reads the one input it comes from, so consecutive work-items touch
// consecutive addresses in every array, an output may be its own input, and the zeros of the SH rows (45 of 48
// floats at degree 3) are stores without a load. No LDS, no atomics.
//
// Image MSE. At most TRAIN_MSE_MAX_WG workgroups, each over a contiguous span of pixels: a work-item adds its
// pixels' three terms in float64 in index order (pixels 256 apart, so a wave reads consecutive pixels), the 256
// sums meet in a halving tree in LDS, and a second launch of one workgroup adds the workgroups' sums the same way.
// Every order is fixed by the sizes alone: two runs give the same bits.
#include "splat_train.h"

#include "splat_train_math.h"

namespace ptgs {
namespace {

constexpr uint32_t TR_WG = 256;

template <uint32_t ROW>
__global__ __launch_bounds__(TR_WG) void gs_checkpoint_init_kernel(const float* scales, const float* opacities,
                                                                  const float* __restrict__ colors, uint32_t n,
                                                                  float* log_scales, float* logits,
                                                                  float* __restrict__ sh) {
  const uint64_t e = (uint64_t)blockIdx.x * TR_WG + threadIdx.x;
  const uint64_t n3 = 3ull * n, n4 = 4ull * n;
  if (e < n3) {
    log_scales[e] = train_log_scale(scales[e]);  // (in place: the element's own input)
  } else if (e < n4) {
    const uint64_t i = e - n3;
    logits[i] = train_logit(opacities[i]);
  } else if (e < n4 + (uint64_t)n * ROW) {
    const uint64_t j = e - n4, i = j / ROW;
    const uint32_t col = (uint32_t)(j - i * ROW);
    sh[j] = col < 3u ? train_rgb2sh(colors[3ull * i + col]) : 0.0f;
  }
}

// the 256 sums of a workgroup in a halving tree; work-item 0 returns the total
__device__ __forceinline__ double tr_tree_sum(double* red, double v) {
  const uint32_t t = threadIdx.x;
  red[t] = v;
  __syncthreads();
  for (uint32_t half = TR_WG / 2u; half > 0u; half >>= 1) {
    if (t < half) red[t] += red[t + half];
    __syncthreads();
  }
  return red[0];
}

template <uint32_t CH>
__global__ __launch_bounds__(TR_WG) void gs_image_mse_kernel(const float* __restrict__ image,
                                                            const float* __restrict__ target, uint64_t pixels,
                                                            uint64_t span, double* __restrict__ partials) {
  __shared__ double red[TR_WG];
  const uint64_t begin = (uint64_t)blockIdx.x * span;
  const uint64_t end = begin + span < pixels ? begin + span : pixels;
  double acc = 0.0;
  for (uint64_t p = begin + threadIdx.x; p < end; p += TR_WG) {
    const float* a = image + 4ull * p;
    const float* b = target + (uint64_t)CH * p;
    const float a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2];
    acc += train_sq_err(a0, b0);
    acc += train_sq_err(a1, b1);
    acc += train_sq_err(a2, b2);
  }
  const double sum = tr_tree_sum(red, acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(TR_WG) void gs_image_mse_final_kernel(const double* __restrict__ partials, uint32_t nwg,
                                                                  double* __restrict__ out_sum) {
  __shared__ double red[TR_WG];
  double acc = 0.0;
  for (uint32_t w = threadIdx.x; w < nwg; w += TR_WG) acc += partials[w];
  const double sum = tr_tree_sum(red, acc);
  if (threadIdx.x == 0) out_sum[0] = sum;
}

}  // namespace

hipError_t train_checkpoint_init(const float* scales, const float* opacities, const float* colors, uint32_t n,
                                 uint32_t sh_degree, float* log_scales, float* logits, float* sh, hipStream_t s) {
  if (n == 0 || sh_degree > 3) return hipErrorInvalidValue;
  const uint32_t row = 3u * (sh_degree + 1u) * (sh_degree + 1u);
  const uint64_t total = (4ull + row) * n;
  const dim3 grid((uint32_t)((total + TR_WG - 1) / TR_WG)), wg(TR_WG);  // (< 2^31: n < 2^32, row <= 48)
  switch (sh_degree) {
    case 0: gs_checkpoint_init_kernel<3><<<grid, wg, 0, s>>>(scales, opacities, colors, n, log_scales, logits, sh); break;
    case 1: gs_checkpoint_init_kernel<12><<<grid, wg, 0, s>>>(scales, opacities, colors, n, log_scales, logits, sh); break;
    case 2: gs_checkpoint_init_kernel<27><<<grid, wg, 0, s>>>(scales, opacities, colors, n, log_scales, logits, sh); break;
    default: gs_checkpoint_init_kernel<48><<<grid, wg, 0, s>>>(scales, opacities, colors, n, log_scales, logits, sh); break;
  }
  return hipGetLastError();
}

hipError_t train_image_mse(const float* image, const float* target, uint32_t channels, uint64_t pixels,
                           double* partials, double* out_sum, hipStream_t s) {
  if (pixels == 0 || (channels != 3 && channels != 4)) return hipErrorInvalidValue;
  // a span is a whole number of workgroup strides, so that every work-item's pixels stay 256 apart
  const uint64_t strides = (pixels + TR_WG - 1) / TR_WG;
  const uint64_t per = (strides + TRAIN_MSE_MAX_WG - 1) / TRAIN_MSE_MAX_WG;
  const uint64_t span = per * TR_WG;
  const uint32_t nwg = (uint32_t)((pixels + span - 1) / span);  // <= TRAIN_MSE_MAX_WG
  if (channels == 4)
    gs_image_mse_kernel<4><<<nwg, TR_WG, 0, s>>>(image, target, pixels, span, partials);
  else
    gs_image_mse_kernel<3><<<nwg, TR_WG, 0, s>>>(image, target, pixels, span, partials);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  gs_image_mse_final_kernel<<<1, TR_WG, 0, s>>>(partials, nwg, out_sum);
  return hipGetLastError();
}

}  // namespace ptgs
