"""torch.autograd through the 3DGS rasterizer: splat() renders with ptgs_splat_gaussians and
differentiates with ptgs_splat_gaussians_backward (HIP kernels on both sides; there is no eager fallback).

    img = autograd.splat(renderer, means, scales, rotations, opacities, colors, ubo, W, H, bg=(0, 0, 0))
    loss(img).backward()

scales are linear and opacities in [0, 1] (post-activation), rotations un-normalised (w, x, y, z), colors
linear RGB. splat_sh() takes a checkpoint's parameters instead (log-scales, opacity logits, SH coefficients: what
load_gaussian_ply returns and a 3DGS trainer optimises):

    img = autograd.splat_sh(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W, H,
                            camera_pos=eye)

Its forward is activate_gaussians, sh_colors and splat_gaussians, its backward splat_gaussians_backward,
sh_colors_backward and activate_gaussians_backward: nothing is evaluated in torch. The backward pass consumes
the frame its forward left in the renderer's workspace, so no other splat call of that renderer may come
between the two (the backward then raises PtgsError). torch is imported on first use.

l1_dssim() is the training loss of such a frame (Renderer.l1_dssim_loss, one HIP call for the value and the
gradient):

    loss = autograd.l1_dssim(renderer, img, target)       # 0.8 * L1 + 0.2 * (1 - SSIM)
    loss.backward()

Depth supervision: splat_depth() and splat_sh_depth() take the arguments of splat() and splat_sh() and return
(img, invdepth), invdepth [H, W] being the frame's expected inverse depth sum(alpha T / d) (Renderer.
splat_gaussians_invdepth); invdepth_l1() is the trainer's L1 on it against a view-depth target (trace_depth):

    img, inv = autograd.splat_sh_depth(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W, H)
    loss = autograd.l1_dssim(renderer, img, target) + autograd.invdepth_l1(renderer, inv, target_depth, weight=w)
    loss.backward()                                       # one ptgs_splat_gaussians_backward_depth
"""
from __future__ import annotations

from . import _abi

_FN = None
_FN_SH = None
_FN_LOSS = None
_FN_DEPTH = None
_FN_SH_DEPTH = None
_FN_DEPTH_LOSS = None


def _publishing(renderer):
    if not renderer._publish & _abi.FLAG_SPLAT_PUBLISH:  # the backward needs the published frame
        renderer._publish |= _abi.FLAG_SPLAT_PUBLISH
        renderer.set_flags(getattr(renderer, "_flags", 0))


def _function_sh():
    global _FN_SH
    if _FN_SH is not None:
        return _FN_SH
    import torch

    class _SplatSh(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, active_degree, camera_pos, means2d_grad, means, log_scales,
                    rotations, opacity_logits, sh):
            means, sh = means.detach().contiguous(), sh.detach().contiguous()
            scales, opacities = renderer.activate_gaussians(log_scales.detach().contiguous(),
                                                            opacity_logits.detach().contiguous())
            colors = renderer.sh_colors(means, sh, camera_pos, active_degree=active_degree)
            g = {"means": means, "scales": scales, "rotations": rotations.detach().contiguous(),
                 "opacities": opacities, "colors": colors}
            _publishing(renderer)
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            # kept for the backward: the activated values and the colours (g), and the coefficients
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g, ctx.sh = renderer, ubo, (W, H), bg, g, sh
            ctx.active_degree, ctx.camera_pos, ctx.means2d_grad = active_degree, camera_pos, means2d_grad
            return out

        @staticmethod
        def backward(ctx, dL_dout):
            W, H = ctx.size
            r, g = ctx.renderer, ctx.g
            need = dict(zip(("means", "log_scales", "rotations", "opacity_logits", "sh"), ctx.needs_input_grad[8:]))
            gr = r.splat_gaussians_backward(g, ctx.ubo, W, H, dL_dout.contiguous().float(), bg=ctx.bg,
                                            want_means2d=ctx.means2d_grad is not None)
            if ctx.means2d_grad is not None:
                ctx.means2d_grad.copy_(gr["means2d"])
            d_sh = d_ls = d_lo = None
            if need["sh"] or need["means"]:  # (the direction part adds into the rasterizer's dL/d means)
                d_sh, _ = r.sh_colors_backward(g["means"], ctx.sh, ctx.camera_pos, gr["colors"],
                                               active_degree=ctx.active_degree, dL_dmeans=gr["means"],
                                               want_means=need["means"])
            if need["log_scales"] or need["opacity_logits"]:
                d_ls, d_lo = r.activate_gaussians_backward(g["scales"], g["opacities"], gr["scales"], gr["opacities"],
                                                           out=(gr["scales"], gr["opacities"]))
            grads = (gr["means"], d_ls, gr["rotations"], d_lo, d_sh)
            return (None,) * 8 + tuple(v if n else None for v, n in zip(grads, need.values()))

    _FN_SH = _SplatSh
    return _FN_SH


def _function():
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class _Splat(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, means, scales, rotations, opacities, colors):
            g = {"means": means.detach().contiguous(), "scales": scales.detach().contiguous(),
                 "rotations": rotations.detach().contiguous(), "opacities": opacities.detach().contiguous(),
                 "colors": colors.detach().contiguous()}
            if not renderer._publish & _abi.FLAG_SPLAT_PUBLISH:  # the backward needs the published frame
                renderer._publish |= _abi.FLAG_SPLAT_PUBLISH
                renderer.set_flags(getattr(renderer, "_flags", 0))
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g = renderer, ubo, (W, H), bg, g
            return out

        @staticmethod
        def backward(ctx, dL_dout):
            W, H = ctx.size
            gr = ctx.renderer.splat_gaussians_backward(ctx.g, ctx.ubo, W, H, dL_dout.contiguous().float(), bg=ctx.bg)
            keys = ("means", "scales", "rotations", "opacities", "colors")
            grads = tuple(gr[k] if need else None for k, need in zip(keys, ctx.needs_input_grad[5:]))
            return (None, None, None, None, None) + grads

    _FN = _Splat
    return _FN


def splat(renderer, means, scales, rotations, opacities, colors, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0)):
    """RGBA32F [H, W, 4] of the Gaussians seen from `ubo`, differentiable with respect to the five tensors
    (float32 device tensors: means [N, 3], scales [N, 3], rotations [N, 4], opacities [N], colors [N, 3])."""
    return _function().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg), means, scales, rotations,
                             opacities, colors)


def splat_sh(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0),
             active_degree=None, camera_pos=None, means2d_grad=None):
    """RGBA32F [H, W, 4] of a checkpoint's Gaussians seen from `ubo`, differentiable with respect to the five
    tensors (float32 device tensors: means [N, 3], log_scales [N, 3], rotations [N, 4], opacity_logits [N],
    sh [N, (d+1)^2, 3]). active_degree (default d) bands are evaluated; camera_pos (default ubo.camera_pos) is
    the eye the colours are seen from. means2d_grad: a float32 [N, 2] device tensor that the backward pass
    fills with dL/d(2D mean), the densification statistic."""
    import torch
    cam = tuple(float(v) for v in (ubo.camera_pos if camera_pos is None else camera_pos))[:3]
    if means2d_grad is not None and (not torch.is_tensor(means2d_grad) or means2d_grad.dtype != torch.float32 or
                                     tuple(means2d_grad.shape) != (int(means.shape[0]), 2) or
                                     not means2d_grad.is_cuda):
        raise _abi.PtgsError("means2d_grad must be a float32 [N, 2] device tensor")
    return _function_sh().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg),
                                None if active_degree is None else int(active_degree), cam, means2d_grad, means,
                                log_scales, rotations, opacity_logits, sh)


def _function_loss():
    global _FN_LOSS
    if _FN_LOSS is not None:
        return _FN_LOSS
    import torch

    class _L1Dssim(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, target, lam, image):
            img = image.detach().contiguous()
            grad = torch.empty_like(img) if ctx.needs_input_grad[3] else None
            terms, grad = renderer.l1_dssim_loss(img, target.detach().contiguous(), lam=lam, grad_out=grad)
            ctx.grad = grad
            return terms[0]

        @staticmethod
        def backward(ctx, dL_dloss):
            grad, ctx.grad = ctx.grad, None  # (scaled in place: a second backward would scale it twice)
            if grad is None:
                raise _abi.PtgsError("l1_dssim: the gradient was already consumed by an earlier backward")
            return None, None, None, grad.mul_(dL_dloss)

    _FN_LOSS = _L1Dssim
    return _FN_LOSS


def l1_dssim(renderer, image, target, lam: float = 0.2):
    """The 3DGS training loss (1 - lam) * mean|image - target| + lam * (1 - SSIM(image, target)) as a 0-dim
    tensor, differentiable with respect to image (RGBA32F [H, W, 4], e.g. splat_sh's output; target
    [H, W, 3 or 4]; float32 device tensors). The forward is the one call ptgs_image_loss_l1_dssim, which
    leaves the value and the gradient; the backward multiplies that gradient in place by the incoming scalar
    gradient, on the device (the scalar is never read on the host): the only torch arithmetic. A trainer
    that wants no torch op at all calls Renderer.l1_dssim_loss(img, target, grad_out=g, grad_scale=...) and
    then img.backward(g)."""
    return _function_loss().apply(renderer, target, float(lam), image)


def _rasterizer_backward(ctx, g, dL_dout, dL_dinv, **kw):
    """The rasterizer's backward for (img, invdepth) outputs: a missing incoming gradient counts as zeros, and
    without the inverse-depth one the call is the plain backward."""
    import torch
    W, H = ctx.size
    if dL_dout is None:
        dL_dout = torch.zeros((H, W, 4), dtype=torch.float32, device=g["means"].device)
    if dL_dinv is not None:
        dL_dinv = dL_dinv.contiguous().float()
    return ctx.renderer.splat_gaussians_backward(g, ctx.ubo, W, H, dL_dout.contiguous().float(), bg=ctx.bg,
                                                 dL_dinvdepth=dL_dinv, **kw)


def _function_depth():
    global _FN_DEPTH
    if _FN_DEPTH is not None:
        return _FN_DEPTH
    import torch

    class _SplatDepth(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, means, scales, rotations, opacities, colors):
            g = {"means": means.detach().contiguous(), "scales": scales.detach().contiguous(),
                 "rotations": rotations.detach().contiguous(), "opacities": opacities.detach().contiguous(),
                 "colors": colors.detach().contiguous()}
            _publishing(renderer)
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            inv = renderer.splat_gaussians_invdepth(W, H, torch.empty((H, W), dtype=torch.float32, device=means.device))
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g = renderer, ubo, (W, H), bg, g
            ctx.set_materialize_grads(False)
            return out, inv

        @staticmethod
        def backward(ctx, dL_dout, dL_dinv):
            keys = ("means", "scales", "rotations", "opacities", "colors")
            if dL_dout is None and dL_dinv is None:
                return (None,) * 10
            gr = _rasterizer_backward(ctx, ctx.g, dL_dout, dL_dinv)
            grads = tuple(gr[k] if need else None for k, need in zip(keys, ctx.needs_input_grad[5:]))
            return (None, None, None, None, None) + grads

    _FN_DEPTH = _SplatDepth
    return _FN_DEPTH


def _function_sh_depth():
    global _FN_SH_DEPTH
    if _FN_SH_DEPTH is not None:
        return _FN_SH_DEPTH
    import torch

    class _SplatShDepth(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, active_degree, camera_pos, means2d_grad, means, log_scales,
                    rotations, opacity_logits, sh):
            means, sh = means.detach().contiguous(), sh.detach().contiguous()
            scales, opacities = renderer.activate_gaussians(log_scales.detach().contiguous(),
                                                            opacity_logits.detach().contiguous())
            colors = renderer.sh_colors(means, sh, camera_pos, active_degree=active_degree)
            g = {"means": means, "scales": scales, "rotations": rotations.detach().contiguous(),
                 "opacities": opacities, "colors": colors}
            _publishing(renderer)
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            inv = renderer.splat_gaussians_invdepth(W, H, torch.empty((H, W), dtype=torch.float32, device=means.device))
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g, ctx.sh = renderer, ubo, (W, H), bg, g, sh
            ctx.active_degree, ctx.camera_pos, ctx.means2d_grad = active_degree, camera_pos, means2d_grad
            ctx.set_materialize_grads(False)
            return out, inv

        @staticmethod
        def backward(ctx, dL_dout, dL_dinv):
            if dL_dout is None and dL_dinv is None:
                return (None,) * 13
            r, g = ctx.renderer, ctx.g
            need = dict(zip(("means", "log_scales", "rotations", "opacity_logits", "sh"), ctx.needs_input_grad[8:]))
            gr = _rasterizer_backward(ctx, g, dL_dout, dL_dinv, want_means2d=ctx.means2d_grad is not None)
            if ctx.means2d_grad is not None:
                ctx.means2d_grad.copy_(gr["means2d"])
            d_sh = d_ls = d_lo = None
            if need["sh"] or need["means"]:  # (the direction part adds into the rasterizer's dL/d means)
                d_sh, _ = r.sh_colors_backward(g["means"], ctx.sh, ctx.camera_pos, gr["colors"],
                                               active_degree=ctx.active_degree, dL_dmeans=gr["means"],
                                               want_means=need["means"])
            if need["log_scales"] or need["opacity_logits"]:
                d_ls, d_lo = r.activate_gaussians_backward(g["scales"], g["opacities"], gr["scales"], gr["opacities"],
                                                           out=(gr["scales"], gr["opacities"]))
            grads = (gr["means"], d_ls, gr["rotations"], d_lo, d_sh)
            return (None,) * 8 + tuple(v if n else None for v, n in zip(grads, need.values()))

    _FN_SH_DEPTH = _SplatShDepth
    return _FN_SH_DEPTH


def splat_depth(renderer, means, scales, rotations, opacities, colors, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0)):
    """splat() with the frame's expected inverse depth: (RGBA32F [H, W, 4], invdepth [H, W]), both differentiable
    with respect to the five tensors. The backward takes both incoming gradients in one
    ptgs_splat_gaussians_backward_depth call; an output that takes no part in the loss counts as a zero gradient,
    and without an inverse-depth gradient the call is the plain backward."""
    return _function_depth().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg), means, scales,
                                   rotations, opacities, colors)


def splat_sh_depth(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W: int, H: int,
                   bg=(0.0, 0.0, 0.0), active_degree=None, camera_pos=None, means2d_grad=None):
    """splat_sh() with the frame's expected inverse depth: (RGBA32F [H, W, 4], invdepth [H, W]); the arguments are
    splat_sh()'s, the backward as in splat_depth()."""
    import torch
    cam = tuple(float(v) for v in (ubo.camera_pos if camera_pos is None else camera_pos))[:3]
    if means2d_grad is not None and (not torch.is_tensor(means2d_grad) or means2d_grad.dtype != torch.float32 or
                                     tuple(means2d_grad.shape) != (int(means.shape[0]), 2) or
                                     not means2d_grad.is_cuda):
        raise _abi.PtgsError("means2d_grad must be a float32 [N, 2] device tensor")
    return _function_sh_depth().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg),
                                      None if active_degree is None else int(active_degree), cam, means2d_grad,
                                      means, log_scales, rotations, opacity_logits, sh)


def _function_depth_loss():
    global _FN_DEPTH_LOSS
    if _FN_DEPTH_LOSS is not None:
        return _FN_DEPTH_LOSS
    import torch

    class _InvDepthL1(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, target_depth, weight, invdepth):
            inv = invdepth.detach().contiguous()
            grad = torch.empty_like(inv) if ctx.needs_input_grad[3] else None
            terms, grad = renderer.invdepth_l1_loss(inv, target_depth.detach().contiguous(), weight=weight,
                                                    grad_out=grad)
            ctx.grad = grad
            return terms[0]

        @staticmethod
        def backward(ctx, dL_dloss):
            grad, ctx.grad = ctx.grad, None  # (scaled in place: a second backward would scale it twice)
            if grad is None:
                raise _abi.PtgsError("invdepth_l1: the gradient was already consumed by an earlier backward")
            return None, None, None, grad.mul_(dL_dloss)

    _FN_DEPTH_LOSS = _InvDepthL1
    return _FN_DEPTH_LOSS


def invdepth_l1(renderer, invdepth, target_depth, weight: float = 1.0):
    """weight * mean over all pixels of |invdepth - 1 / target_depth| on the supervised pixels (target_depth > 0,
    +inf included; Renderer.invdepth_l1_loss) as a 0-dim tensor, differentiable with respect to invdepth
    ([H, W], e.g. splat_sh_depth's second output; target_depth [H, W] a view depth, e.g. trace_depth's). It works
    like l1_dssim: one HIP call leaves the value and the gradient, the backward scales the gradient in place."""
    return _function_depth_loss().apply(renderer, target_depth, float(weight), invdepth)
