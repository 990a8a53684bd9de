"""torch.autograd through the 3DGS rasterizer: splat() renders with ptgs_splat_gaussians and
differentiates with ptgs_splat_gaussians_backward (HIP kernels on both sides; there is no eager fallback).

    img = autograd.splat(renderer, means, scales, rotations, opacities, colors, ubo, W, H, bg=(0, 0, 0))
    loss(img).backward()

scales are linear and opacities in [0, 1] (post-activation), rotations un-normalised (w, x, y, z), colors
linear RGB: chain the activations and the SH colour in torch. The backward pass consumes the frame its
forward left in the renderer's workspace, so no other splat call of that renderer may come between the two
(the backward then raises PtgsError). torch is imported on first use.
"""
from __future__ import annotations

from . import _abi

_FN = None


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
