"""The optimizer of a 3DGS training run on the HIP kernels of csrc/splat_adam.hip: Adam over the five leaves of a
checkpoint in one launch, stepping only the Gaussians the view saw (the sparse Adam of Kerbl et al.'s trainer), the
SH DC term at its own rate, and the opacity reset. Nothing N-sized is evaluated in torch.

    opt = GaussianAdam(params, {"means": 0.00016 * extent, "log_scales": 0.005, "rotations": 0.001,
                                "opacity_logits": 0.025, "sh": 0.0025 / 20, "sh_dc": 0.0025})
    for it, view in enumerate(views, 1):
        opt.zero_grad()
        img = autograd.splat_sh(renderer, *leaves, ubo, W, H, means2d_grad=m2d)
        loss(img).backward()
        opt.set_lr("means", expon_lr(it, 0.00016 * extent, 0.0000016 * extent, 30_000))
        opt.step(renderer)                               # masked by the frame's own radii
        if it % 3000 == 0:
            opt.reset_opacity(renderer)

params is the dict of the five leaf tensors ("means", "log_scales", "rotations", "opacity_logits", "sh").
densify.densify_and_prune(..., optimizer=opt) moves the moments with their rows. torch is imported on first use.
"""
from __future__ import annotations

import math

from . import _abi
from .densify import PARAM_KEYS

SH_DC = "sh_dc"  # the key of lr that gives the first 3 floats of every SH row (the DC term) their own rate


def expon_lr(step: int, lr_init: float, lr_final: float, max_steps: int, delay_steps: int = 0,
             delay_mult: float = 1.0) -> float:
    """The reference trainer's get_expon_lr_func as a plain host function: log-linear interpolation from lr_init
    (step 0) to lr_final (max_steps and beyond), times a sine ramp from delay_mult to 1 over the first
    delay_steps. 0 when both ends are 0 or step < 0."""
    if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
        return 0.0
    if delay_steps > 0:
        rate = delay_mult + (1.0 - delay_mult) * math.sin(0.5 * math.pi * min(max(step / delay_steps, 0.0), 1.0))
    else:
        rate = 1.0
    t = min(max(step / max_steps, 0.0), 1.0)
    return rate * math.exp(math.log(lr_init) * (1.0 - t) + math.log(lr_final) * t)


def _bump(tensors):
    """Tell autograd the tensors changed in place (no kernel); torch builds without the call: nothing."""
    import torch
    inc = getattr(torch.autograd.graph, "increment_version", None)
    if inc is not None:
        for t in tensors:
            inc(t)


class GaussianAdam:
    """Adam over the five leaves of a checkpoint, one ptgs_gaussians_adam_step per step.

    lr: a rate per leaf, and optionally "sh_dc": the first 3 floats of every SH row then step with lr["sh_dc"]
    and the rest with lr["sh"] (the trainer's f_dc / f_rest). exp_avg / exp_avg_sq: dicts of zero-initialised
    moments shaped like the leaves; step_count: the steps taken (the bias correction is global, as in the
    trainer's sparse Adam). The leaves are written through raw pointers, after the backward; where the installed
    torch has torch.autograd.graph.increment_version their version counters are bumped, otherwise they change
    behind autograd's back (safe once the backward has run: nothing saved is read again)."""

    def __init__(self, params: dict, lr: dict, betas=(0.9, 0.999), eps: float = 1e-15):
        import torch
        missing = [k for k in PARAM_KEYS if k not in params]
        if missing:
            raise _abi.PtgsError(f"params lacks {missing}")
        no_lr = [k for k in PARAM_KEYS if k not in lr]
        if no_lr:
            raise _abi.PtgsError(f"lr lacks {no_lr}")
        unknown = [k for k in lr if k not in PARAM_KEYS and k != SH_DC]
        if unknown:
            raise _abi.PtgsError(f"lr has unknown keys {unknown}")
        self.params = {k: params[k] for k in PARAM_KEYS}
        for k, p in self.params.items():
            if p.dtype != torch.float32 or not p.is_cuda or not p.is_contiguous():
                raise _abi.PtgsError(f"{k} must be a contiguous float32 device tensor")
        self.lr = {k: float(v) for k, v in lr.items()}
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.exp_avg = {k: torch.zeros_like(p.detach()) for k, p in self.params.items()}
        self.exp_avg_sq = {k: torch.zeros_like(p.detach()) for k, p in self.params.items()}
        self.step_count = 0

    def set_lr(self, key: str, value: float):
        """A new rate for one key of lr (the position schedule: set_lr("means", expon_lr(...)))."""
        if key not in self.lr:
            raise _abi.PtgsError(f"no rate {key!r} (have {sorted(self.lr)})")
        self.lr[key] = float(value)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params.values():
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    def step(self, renderer, masked: bool = True, radii=None, stream=None):
        """One step over the leaves whose .grad is not None (the others are skipped, as torch does), in one C
        call. masked: only the Gaussians the published frame saw step (radii: int32 [N] to use instead of the
        frame's own; see Renderer.adam_step). Launches no torch kernel and waits for nothing."""
        self.step_count += 1
        rows, touched = [], []
        for k in PARAM_KEYS:
            p = self.params[k]
            g = p.grad
            if g is None:
                continue
            if not g.is_contiguous():
                raise _abi.PtgsError(f"the gradient of {k} is not contiguous")
            r = (p.detach(), g, self.exp_avg[k], self.exp_avg_sq[k], self.lr[k])
            if k == "sh" and SH_DC in self.lr:
                r += (3, self.lr[SH_DC])
            rows.append(r)
            touched += [p, self.exp_avg[k], self.exp_avg_sq[k]]
        if not rows:
            return
        renderer.adam_step(rows, step=self.step_count, betas=self.betas, eps=self.eps, radii=radii, masked=masked,
                           stream=stream)
        _bump(touched)

    def reset_opacity(self, renderer, max_opacity: float = 0.01, stream=None):
        """The trainer's reset_opacity: logits capped at logit(max_opacity), the opacity's moments zeroed."""
        k = "opacity_logits"
        renderer.opacity_reset(self.params[k].detach(), max_opacity, self.exp_avg[k], self.exp_avg_sq[k], stream=stream)
        _bump([self.params[k], self.exp_avg[k], self.exp_avg_sq[k]])
