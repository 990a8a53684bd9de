// splat_loss.h — the 3DGS training loss, fused L1 + D-SSIM with its gradient (see splat_loss.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptgs {

constexpr uint32_t LOSS_MAX_SIDE = 16384;

struct LossWorkspace;  // the partial maps and the per-workgroup sums (one per context, grown on demand)
LossWorkspace* loss_workspace_create();
void loss_workspace_destroy(LossWorkspace* ws);

// contract in ptgs.h (arguments checked by the caller); grad may be null: the loss terms only. Enqueues two or
// three kernels on s and never waits for them; growing the workspace frees the old one first.
hipError_t image_loss_l1_dssim(LossWorkspace* ws, const float* image, const float* target, uint32_t channels,
                               uint32_t W, uint32_t H, float lambda, float grad_scale, float* loss_out, float* grad,
                               hipStream_t s);

// The L1 on rendered inverse depth against a view-depth target (contract in ptgs.h, arguments checked by the
// caller); grad may be null. Two kernels on s, no host wait; its per-workgroup sums (16 bytes per 1024 pixels)
// are a buffer of their own in the workspace, so it does not disturb image_loss_l1_dssim's.
hipError_t image_loss_invdepth_l1(LossWorkspace* ws, const float* invdepth, const float* target_depth, uint32_t W,
                                  uint32_t H, float weight, float grad_scale, float* terms, float* grad, hipStream_t s);

}  // namespace ptgs
