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

The camera pose: all four splat functions take view=, a float32 [4, 4] tensor that replaces ubo.view and receives
dL/d view (ptgs_splat_gaussians_backward_pose; for the SH forms the eye's gradient as well,
ptgs_gaussians_sh_colors_backward_eye, chained back into view in torch). se3_view() is the parametrisation:

    xi = torch.zeros(6, requires_grad=True)               # (translation, rotation), what the optimiser steps
    img, inv = autograd.splat_sh_depth(renderer, ..., ubo, W, H, view=autograd.se3_view(view0, xi))
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


def _sh_chain(ctx, r, g, gr, need, need_view, need_eye):
    """The rest of a splat_sh backward after the rasterizer's (gr): means2d_grad, sh_colors_backward (with the eye
    sum when the eye takes a gradient) and activate_gaussians_backward. Returns the gradients of (means, log_scales,
    rotations, opacity_logits, sh, view, eye)."""
    if ctx.means2d_grad is not None:
        ctx.means2d_grad.copy_(gr["means2d"])
    d_sh = d_ls = d_lo = d_eye = None
    if need_eye:
        d_sh, _, d_eye = r.sh_colors_backward(g["means"], ctx.sh, ctx.camera_pos, gr["colors"],
                                              active_degree=ctx.active_degree, dL_dmeans=gr["means"],
                                              want_means=need["means"], want_eye=True)
        d_eye = d_eye.to(ctx.pose_devices[1])
    elif need["sh"] or need["means"]:  # (the direction part adds into the rasterizer's dL/d means)
        d_sh, _ = r.sh_colors_backward(g["means"], ctx.sh, ctx.camera_pos, gr["colors"],
                                       active_degree=ctx.active_degree, dL_dmeans=gr["means"],
                                       want_means=need["means"])
    if need["log_scales"] or need["opacity_logits"]:
        d_ls, d_lo = r.activate_gaussians_backward(g["scales"], g["opacities"], gr["scales"], gr["opacities"],
                                                   out=(gr["scales"], gr["opacities"]))
    grads = (gr["means"], d_ls, gr["rotations"], d_lo, d_sh)
    d_view = gr["view"].to(ctx.pose_devices[0]) if need_view else None
    return tuple(v if n else None for v, n in zip(grads, need.values())) + (d_view, d_eye)


def _function_sh():
    global _FN_SH
    if _FN_SH is not None:
        return _FN_SH
    import torch

    class _SplatSh(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, active_degree, camera_pos, means2d_grad, means, log_scales,
                    rotations, opacity_logits, sh, view=None, eye=None):
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
            ctx.pose_devices = tuple(None if t is None else t.device for t in (view, eye))
            return out

        @staticmethod
        def backward(ctx, dL_dout):
            W, H = ctx.size
            r, g = ctx.renderer, ctx.g
            need = dict(zip(("means", "log_scales", "rotations", "opacity_logits", "sh"), ctx.needs_input_grad[8:]))
            need_view, need_eye = ctx.needs_input_grad[13:15]
            gr = r.splat_gaussians_backward(g, ctx.ubo, W, H, dL_dout.contiguous().float(), bg=ctx.bg,
                                            want_means2d=ctx.means2d_grad is not None,
                                            **({"want_view": True} if need_view else {}))
            return (None,) * 8 + _sh_chain(ctx, r, g, gr, need, need_view, need_eye)

    _FN_SH = _SplatSh
    return _FN_SH


def _function():
    global _FN
    if _FN is not None:
        return _FN
    import torch

    class _Splat(torch.autograd.Function):
        @staticmethod
        def forward(ctx, renderer, ubo, W, H, bg, means, scales, rotations, opacities, colors, view=None):
            g = {"means": means.detach().contiguous(), "scales": scales.detach().contiguous(),
                 "rotations": rotations.detach().contiguous(), "opacities": opacities.detach().contiguous(),
                 "colors": colors.detach().contiguous()}
            if not renderer._publish & _abi.FLAG_SPLAT_PUBLISH:  # the backward needs the published frame
                renderer._publish |= _abi.FLAG_SPLAT_PUBLISH
                renderer.set_flags(getattr(renderer, "_flags", 0))
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g = renderer, ubo, (W, H), bg, g
            ctx.view_device = None if view is None else view.device
            return out

        @staticmethod
        def backward(ctx, dL_dout):
            W, H = ctx.size
            need_view = ctx.needs_input_grad[10]
            gr = ctx.renderer.splat_gaussians_backward(ctx.g, ctx.ubo, W, H, dL_dout.contiguous().float(), bg=ctx.bg,
                                                       **({"want_view": True} if need_view else {}))
            keys = ("means", "scales", "rotations", "opacities", "colors")
            grads = tuple(gr[k] if need else None for k, need in zip(keys, ctx.needs_input_grad[5:]))
            return (None, None, None, None, None) + grads + (gr["view"].to(ctx.view_device) if need_view else None,)

    _FN = _Splat
    return _FN


def _posed_ubo(ubo, view):
    """A copy of `ubo` whose view is the float32 [4, 4] tensor `view` (math indexing; ptgs_ubo.view is
    column-major). The caller's ubo is not modified."""
    import torch
    if not torch.is_tensor(view) or view.dtype != torch.float32 or tuple(view.shape) != (4, 4):
        raise _abi.PtgsError("view must be a float32 [4, 4] tensor")
    posed = type(ubo).from_buffer_copy(ubo)
    posed.view[:] = [float(v) for v in view.detach().cpu().t().reshape(-1)]
    return posed


def _posed_eye(ubo, view, camera_pos):
    """(the eye as three floats, the eye as a tensor that takes a gradient or None). With view= the eye defaults to
    the eye of the view, -R^T t, computed in torch: autograd chains its gradient back into view."""
    import torch
    if view is not None and camera_pos is None:
        camera_pos = -(view[:3, :3].t() @ view[:3, 3])
    if torch.is_tensor(camera_pos):
        if view is None:
            raise _abi.PtgsError("a tensor camera_pos needs view=")
        if camera_pos.dtype != torch.float32 or camera_pos.numel() != 3:
            raise _abi.PtgsError("camera_pos must be three floats or a float32 tensor of 3 elements")
        return tuple(float(v) for v in camera_pos.detach().cpu().reshape(3)), camera_pos
    return tuple(float(v) for v in (ubo.camera_pos if camera_pos is None else camera_pos))[:3], None


def splat(renderer, means, scales, rotations, opacities, colors, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0), view=None):
    """RGBA32F [H, W, 4] of the Gaussians seen from `ubo`, differentiable with respect to the five tensors
    (float32 device tensors: means [N, 3], scales [N, 3], rotations [N, 4], opacities [N], colors [N, 3]).
    view: a float32 [4, 4] tensor in math indexing, on the CPU or on the device (e.g. se3_view(view0, xi)); it
    replaces ubo.view in a copy of ubo and receives its gradient on its own device
    (ptgs_splat_gaussians_backward_pose)."""
    if view is not None:
        ubo = _posed_ubo(ubo, view)
    return _function().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg), means, scales, rotations,
                             opacities, colors, view)


def splat_sh(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0),
             active_degree=None, camera_pos=None, means2d_grad=None, view=None):
    """RGBA32F [H, W, 4] of a checkpoint's Gaussians seen from `ubo`, differentiable with respect to the five
    tensors (float32 device tensors: means [N, 3], log_scales [N, 3], rotations [N, 4], opacity_logits [N],
    sh [N, (d+1)^2, 3]). active_degree (default d) bands are evaluated; camera_pos (default ubo.camera_pos) is
    the eye the colours are seen from. means2d_grad: a float32 [N, 2] device tensor that the backward pass
    fills with dL/d(2D mean), the densification statistic.
    view: as in splat(). camera_pos may then be a float32 tensor of 3 elements too, which receives its gradient
    (ptgs_gaussians_sh_colors_backward_eye); it defaults to the eye of view, -R^T t, computed in torch, so that
    the eye's gradient is chained back into view."""
    import torch
    if view is not None:
        ubo = _posed_ubo(ubo, view)
    cam, eye = _posed_eye(ubo, view, camera_pos)
    if means2d_grad is not None and (not torch.is_tensor(means2d_grad) or means2d_grad.dtype != torch.float32 or
                                     tuple(means2d_grad.shape) != (int(means.shape[0]), 2) or
                                     not means2d_grad.is_cuda):
        raise _abi.PtgsError("means2d_grad must be a float32 [N, 2] device tensor")
    return _function_sh().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg),
                                None if active_degree is None else int(active_degree), cam, means2d_grad, means,
                                log_scales, rotations, opacity_logits, sh, view, eye)


def se3_view(view0, xi):
    """exp(hat(xi)) @ view0 for a 6-vector xi = (translation, rotation): the view matrix view0 ([4, 4], math
    indexing) moved by a twist in camera space, the parametrisation to give an optimiser (xi a leaf at zeros,
    view=se3_view(view0, xi)). Plain torch on 4x4 matrices, differentiable; exactly view0 at xi = 0."""
    import torch
    view0 = torch.as_tensor(view0, dtype=xi.dtype, device=xi.device)
    z = xi.new_zeros(())
    v, w = xi[:3], xi[3:]
    hat = torch.stack([torch.stack([z, -w[2], w[1], v[0]]), torch.stack([w[2], z, -w[0], v[1]]),
                       torch.stack([-w[1], w[0], z, v[2]]), torch.stack([z, z, z, z])])
    return torch.linalg.matrix_exp(hat) @ view0


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
        def forward(ctx, renderer, ubo, W, H, bg, means, scales, rotations, opacities, colors, view=None):
            g = {"means": means.detach().contiguous(), "scales": scales.detach().contiguous(),
                 "rotations": rotations.detach().contiguous(), "opacities": opacities.detach().contiguous(),
                 "colors": colors.detach().contiguous()}
            _publishing(renderer)
            out = torch.empty((H, W, 4), dtype=torch.float32, device=means.device)
            renderer.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True)
            inv = renderer.splat_gaussians_invdepth(W, H, torch.empty((H, W), dtype=torch.float32, device=means.device))
            ctx.renderer, ctx.ubo, ctx.size, ctx.bg, ctx.g = renderer, ubo, (W, H), bg, g
            ctx.view_device = None if view is None else view.device
            ctx.set_materialize_grads(False)
            return out, inv

        @staticmethod
        def backward(ctx, dL_dout, dL_dinv):
            keys = ("means", "scales", "rotations", "opacities", "colors")
            if dL_dout is None and dL_dinv is None:
                return (None,) * 11
            need_view = ctx.needs_input_grad[10]
            gr = _rasterizer_backward(ctx, ctx.g, dL_dout, dL_dinv, **({"want_view": True} if need_view else {}))
            grads = tuple(gr[k] if need else None for k, need in zip(keys, ctx.needs_input_grad[5:]))
            return (None, None, None, None, None) + grads + (gr["view"].to(ctx.view_device) if need_view else None,)

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
                    rotations, opacity_logits, sh, view=None, eye=None):
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
            ctx.pose_devices = tuple(None if t is None else t.device for t in (view, eye))
            ctx.set_materialize_grads(False)
            return out, inv

        @staticmethod
        def backward(ctx, dL_dout, dL_dinv):
            if dL_dout is None and dL_dinv is None:
                return (None,) * 15
            r, g = ctx.renderer, ctx.g
            need = dict(zip(("means", "log_scales", "rotations", "opacity_logits", "sh"), ctx.needs_input_grad[8:]))
            need_view, need_eye = ctx.needs_input_grad[13:15]
            gr = _rasterizer_backward(ctx, g, dL_dout, dL_dinv, want_means2d=ctx.means2d_grad is not None,
                                      **({"want_view": True} if need_view else {}))
            return (None,) * 8 + _sh_chain(ctx, r, g, gr, need, need_view, need_eye)

    _FN_SH_DEPTH = _SplatShDepth
    return _FN_SH_DEPTH


def splat_depth(renderer, means, scales, rotations, opacities, colors, ubo, W: int, H: int, bg=(0.0, 0.0, 0.0),
                view=None):
    """splat() with the frame's expected inverse depth: (RGBA32F [H, W, 4], invdepth [H, W]), both differentiable
    with respect to the five tensors. The backward takes both incoming gradients in one
    ptgs_splat_gaussians_backward_depth call; an output that takes no part in the loss counts as a zero gradient,
    and without an inverse-depth gradient the call is the plain backward. view: as in splat(); the inverse depth
    passes gradient to it too."""
    if view is not None:
        ubo = _posed_ubo(ubo, view)
    return _function_depth().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg), means, scales,
                                   rotations, opacities, colors, view)


def splat_sh_depth(renderer, means, log_scales, rotations, opacity_logits, sh, ubo, W: int, H: int,
                   bg=(0.0, 0.0, 0.0), active_degree=None, camera_pos=None, means2d_grad=None, view=None):
    """splat_sh() with the frame's expected inverse depth: (RGBA32F [H, W, 4], invdepth [H, W]); the arguments are
    splat_sh()'s (view and a tensor camera_pos included), the backward as in splat_depth()."""
    import torch
    if view is not None:
        ubo = _posed_ubo(ubo, view)
    cam, eye = _posed_eye(ubo, view, camera_pos)
    if means2d_grad is not None and (not torch.is_tensor(means2d_grad) or means2d_grad.dtype != torch.float32 or
                                     tuple(means2d_grad.shape) != (int(means.shape[0]), 2) or
                                     not means2d_grad.is_cuda):
        raise _abi.PtgsError("means2d_grad must be a float32 [N, 2] device tensor")
    return _function_sh_depth().apply(renderer, ubo, int(W), int(H), tuple(float(b) for b in bg),
                                      None if active_degree is None else int(active_degree), cam, means2d_grad,
                                      means, log_scales, rotations, opacity_logits, sh, view, eye)


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
