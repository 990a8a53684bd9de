"""Gradient reference for the forward's hard cases: splat_forward_ref.CASES (needles, giants, near-plane, sub-pixel,
tied and opacity-edge Gaussians, long lists, 1x1 to 130x9 frames) differentiated by splat_depth_ref.evaluate.

Nothing here comes from oracle/: the frame handed to the evaluation (radii, ranges, vals, K) is built from
splat_forward_ref's own float64 run, its visibility, its radii and, per tile in row-major order, its depth order
restricted to the tile's members. The upstream gradients dL_dout (seeded normal) and dL_dinv (seeded normal times
splat_depth_ref.DINV_SCALE) are exactly 0 on the forward reference's mask (its border_pixels: every pixel a decision
that float32 could take either way reaches), so a pixel whose membership, order, skip, clamp or stop is in doubt
contributes exactly nothing to any gradient. The forward's mask does not cover the EWA clamp decision, which changes
the gradient and not the image: a visible Gaussian whose |x / d| / limx or |y / d| / limy lies within CLAMP_MARGIN
relative of 1 has the pixels of its tile rectangle masked as well ("clamp_doubt"; none today).

tests/test_splat_hard_grad_ref.py checks the reference on the CPU; tests/test_splat_backward_hard_gpu.py compares
the GPU with it.
"""
import numpy as np
import torch

import splat_depth_ref as Z
import splat_forward_ref as F
import splat_grad_ref as R

TILE = F.TILE
CASES = tuple(k for k in F.CASES if k != "over")
CLAMP_MARGIN = 1e-4
BOUND_CAP = 1e-2  # max(1e-4, 8 e32) may not exceed this: a blown-up float32 yardstick must not hide a failure
_DL_SEED = {k: 1200 + i for i, k in enumerate(CASES)}
_DINV_SEED = {k: 1700 + i for i, k in enumerate(CASES)}
PARTS = (("grads", "backward_depth"), ("grads_color", "backward"), ("grads_depth", "depth only"))


def frame_of(r64, W, H):
    """The frame as splat_depth_ref.evaluate and splat_grad_ref.subsets read it, from a splat_forward_ref.render
    float64 run: radii (0: culled), ranges [tiles, 2] and vals (per tile, row-major, the members in depth order)."""
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    order, member = r64["order"], r64["tiles_member"]
    lists = [order[member[order, ty, tx]] for ty in range(gy) for tx in range(gx)]
    ends = np.cumsum([len(v) for v in lists])
    ranges = np.stack([ends - [len(v) for v in lists], ends], 1).astype(np.int64)
    vals = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
    radii = np.where(r64["vis"], r64["radius"], 0).astype(np.int64)
    assert len(vals) == r64["K"] and ((radii > 0) == r64["vis"]).all()
    return {"radii": radii, "ranges": ranges, "vals": vals, "K": int(r64["K"])}


def clamp_ratio(g, ubo):
    """(|x / d| / limx, |y / d| / limy) per Gaussian in float64: beyond the EWA clamp where above 1."""
    view = np.asarray(ubo.view, np.float64).reshape(4, 4).T
    pv = np.c_[np.asarray(g["means"], np.float64), np.ones(len(g["means"]))] @ view.T
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(pv[:, 0] / -pv[:, 2]) / (1.3 / float(ubo.proj[0])),
                np.abs(pv[:, 1] / -pv[:, 2]) / (1.3 / abs(float(ubo.proj[5]))))


def _rect_pixels(rect, W, H):
    m = np.zeros((H, W), bool)
    for x0, y0, x1, y1 in rect:
        m[y0 * TILE:min(H, y1 * TILE), x0 * TILE:min(W, x1 * TILE)] = True
    return m


_CACHE = {}


def case_reference(name):
    """{"name", "g", "ubo", "W", "H", "bg", "fwd" (splat_forward_ref.case_reference: the image and inverse depth
    references and their bounds), "frame", "mask", "clamp_doubt" (indices), "clamp_margin" (the closest visible
    Gaussian's relative distance to the clamp), "dL", "dinv", "r64", "r32"}. Computed once per session and never
    modified."""
    if name not in _CACHE:
        fwd = F.case_reference(name)
        g, ubo, W, H, bg = fwd["g"], fwd["ubo"], fwd["W"], fwd["H"], fwd["bg"]
        frame = frame_of(fwd["r64"], W, H)
        vis = frame["radii"] > 0
        dist = np.minimum(*(np.abs(r - 1.0) for r in clamp_ratio(g, ubo)))
        doubt = np.flatnonzero(vis & ~(dist > CLAMP_MARGIN))
        mask = fwd["mask"] | _rect_pixels(fwd["r64"]["rect"][doubt], W, H)
        dL = np.random.default_rng(_DL_SEED[name]).normal(size=(H, W, 4)).astype(np.float32)
        dinv = (np.random.default_rng(_DINV_SEED[name]).normal(size=(H, W)) * Z.DINV_SCALE).astype(np.float32)
        dL[mask] = 0.0
        dinv[mask] = 0.0
        c = {"name": name, "g": g, "ubo": ubo, "W": W, "H": H, "bg": bg, "fwd": fwd, "frame": frame, "mask": mask,
             "clamp_doubt": doubt, "clamp_margin": float(dist[vis].min()) if vis.any() else np.inf, "dL": dL,
             "dinv": dinv}
        for key, dt in (("r64", torch.float64), ("r32", torch.float32)):
            c[key] = Z.evaluate(g, ubo, W, H, bg, frame, dL, dinv, dt)
        _CACHE[name] = c
    return _CACHE[name]


def checked(c):
    """[(part of the reference, the call that computes it, keys)]: what a comparison covers. The colours do not enter
    the inverse depth: their depth-only gradient is exactly zero on both sides and is asserted as such."""
    return [(which, label, [k for k in R.GRAD_KEYS if not (which == "grads_depth" and k == "colors")])
            for which, label in PARTS]
