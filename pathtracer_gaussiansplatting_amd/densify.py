"""Densification and pruning of a 3DGS training run (densify_and_prune of Kerbl et al.'s trainer) on the HIP
kernels of csrc/splat_densify.hip: nothing N-sized is evaluated in torch.

    stats = DensifyStats(n, device)
    for view in views:                                   # the training loop
        m2d = torch.zeros((n, 2), device=device)
        img = autograd.splat_sh(renderer, *leaves, ubo, W, H, means2d_grad=m2d)
        loss(img).backward(); optimizer.step()
        stats.update(renderer, m2d, W, H)                # right after the backward: uses that frame's radii
    params, counts, stats = densify_and_prune(renderer, params, stats, scale_split=0.01 * extent,
                                              max_scale=0.1 * extent, optimizer=optimizer)

params is the dict of the five leaf tensors of a checkpoint ("means", "log_scales", "rotations",
"opacity_logits", "sh"); the call returns five new leaves. With a torch.optim.Adam its exp_avg / exp_avg_sq move
with their rows (zeros for new Gaussians), `step` is kept and the param groups point at the new leaves, so the
optimizer keeps running; an optim.GaussianAdam is treated alike (its ten moment arrays, its step_count, its
leaves). torch is imported on first use.
"""
from __future__ import annotations

from . import _abi

PARAM_KEYS = ("means", "log_scales", "rotations", "opacity_logits", "sh")
_MOMENTS = ("exp_avg", "exp_avg_sq")


class DensifyStats:
    """The statistic densify_and_prune decides on: per Gaussian the summed NDC-scaled norm of dL/d(2D mean) over
    the views that saw it (accum), their number (denom) and the largest screen radius (max_radii)."""

    def __init__(self, n: int, device="cuda"):
        import torch
        self.n = int(n)
        self.accum = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.denom = torch.zeros(self.n, dtype=torch.float32, device=device)
        self.max_radii = torch.zeros(self.n, dtype=torch.float32, device=device)

    def update(self, renderer, means2d_grad, W: int, H: int, radii=None, stream=None):
        """One view: means2d_grad [N, 2] as the backward left it; radii default to the published frame's."""
        renderer.densify_accumulate(means2d_grad, W, H, self.accum, self.denom, self.max_radii, radii=radii,
                                    stream=stream)

    def reset(self):
        for t in (self.accum, self.denom, self.max_radii):
            t.zero_()


def _adam_state(optimizer, p):
    """(group, index, state) of leaf p in a torch.optim.Adam; state is None before the first step."""
    for g in optimizer.param_groups:
        for k, q in enumerate(g["params"]):
            if q is p:
                st = optimizer.state.get(p)
                return g, k, (st if st else None)
    raise _abi.PtgsError("a parameter is not in the optimizer's param groups")


def densify_and_prune(renderer, params: dict, stats: DensifyStats, *, grad_threshold: float = 0.0002,
                      scale_split: float, min_opacity: float = 0.005, max_scale: float = 0.0,
                      max_screen_radius: float = 0.0, optimizer=None, generator=None, stream=None):
    """Clone the small Gaussians whose averaged statistic reaches grad_threshold (largest scale <= scale_split),
    split the large ones into two children (scales / 1.6, means drawn from the parent), and prune what is more
    transparent than min_opacity, larger than max_scale or wider on screen than max_screen_radius (0 disables
    either). Returns (new_params, counts, new_stats): five new leaf tensors (requires_grad as before) in the
    trainer's order (survivors, clones, first children, second children), the ptgs_densify_counts and fresh,
    zeroed DensifyStats of the new size. generator: the torch.Generator (on the parameters' device) the
    children's normal draws come from."""
    import torch
    missing = [k for k in PARAM_KEYS if k not in params]
    if missing:
        raise _abi.PtgsError(f"params lacks {missing}")
    p = {k: params[k] for k in PARAM_KEYS}
    n = int(p["means"].shape[0])
    if stats.n != n:
        raise _abi.PtgsError(f"the statistic covers {stats.n} gaussians, the parameters {n}")
    dev = p["means"].device
    d = {k: v.detach().contiguous() for k, v in p.items()}
    scales, opacities = renderer.activate_gaussians(d["log_scales"], d["opacity_logits"], stream=stream)
    counts = renderer.densify_plan(scales, opacities, stats.accum, stats.denom, stats.max_radii,
                                   grad_threshold=grad_threshold, scale_split=scale_split, min_opacity=min_opacity,
                                   max_scale=max_scale, max_screen_radius=max_screen_radius, stream=stream)
    noise = torch.randn((2, n, 3), dtype=torch.float32, device=dev, generator=generator)
    rows = [(d["rotations"], False), (d["opacity_logits"], False), (d["sh"], False)]
    moved = []  # (key, moment name) in the order of the rows after the three above
    states = {}
    from .optim import GaussianAdam
    ours = isinstance(optimizer, GaussianAdam)
    if ours:
        if any(optimizer.params[k] is not p[k] for k in PARAM_KEYS):
            raise _abi.PtgsError("a parameter is not the GaussianAdam's own leaf")
        for k in PARAM_KEYS:
            for m in _MOMENTS:
                rows.append((getattr(optimizer, m)[k].view(n, -1), True))
                moved.append((k, m))
    elif optimizer is not None:
        if not isinstance(optimizer, torch.optim.Adam) or any(g.get("amsgrad") for g in optimizer.param_groups):
            raise _abi.PtgsError("densify_and_prune moves the state of a torch.optim.Adam without amsgrad")
        for k in PARAM_KEYS:
            states[k] = _adam_state(optimizer, p[k])
            st = states[k][2]
            if st is None:
                continue
            for m in _MOMENTS:
                rows.append((st[m].detach().contiguous().view(n, -1), True))
                moved.append((k, m))
    means_out, ls_out, outs, _ = renderer.densify_apply(counts.total, d["means"], d["log_scales"], d["rotations"],
                                                        scales, noise, rows, stream=stream)
    new = {"means": means_out, "log_scales": ls_out, "rotations": outs[0], "opacity_logits": outs[1], "sh": outs[2]}
    new = {k: v.requires_grad_(p[k].requires_grad) for k, v in new.items()}
    if ours:  # step_count stays as it is
        optimizer.params = dict(new)
        for (k, m), t in zip(moved, outs[3:]):
            getattr(optimizer, m)[k] = t.view(new[k].shape)
    elif optimizer is not None:
        moments = {km: t for km, t in zip(moved, outs[3:])}
        for k in PARAM_KEYS:
            group, at, st = states[k]
            group["params"][at] = new[k]
            if st is not None:
                del optimizer.state[p[k]]
                kept = {name: v for name, v in st.items() if name not in _MOMENTS}  # `step` stays as it is
                for m in _MOMENTS:
                    kept[m] = moments[(k, m)].view(new[k].shape)
                optimizer.state[new[k]] = kept
    return new, counts, DensifyStats(counts.total, dev)
