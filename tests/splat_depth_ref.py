"""Reference for the 3DGS depth supervision (ptgs_splat_gaussians_invdepth, ptgs_splat_gaussians_backward_depth,
ptgs_image_loss_invdepth_l1), independent of the code under test.

evaluate() restates splat_grad_ref.evaluate (the forward as ptgs.h states it: membership and order from the CPU
oracle's frame, the projection written out, the blend tile by tile in torch on the CPU, the discrete decisions
taken from a detached evaluation) and adds the expected inverse depth
    D[pixel] = sum wgt / d,    d = -(view * mean).z,    wgt = alpha T   (the colour's weights; no background term)
torch.autograd differentiates three scalars on the one graph: sum(rgba dL_dout) + sum(D dL_dinv) ("grads", what
the backward with both gradients computes), its colour part alone ("grads_color") and its depth part alone
("grads_depth"). The cases are splat_grad_ref.CASES with the same dL_dout; dL_dinv is seeded normal times
DINV_SCALE, a constant chosen so that in every case the depth-only gradient of the means is within 10x of the
colour-only one (tests/test_splat_depth_ref.py asserts it): otherwise the colour part would hide a wrong depth part.

invdepth_l1() restates the loss: f32 terms, f64 sum.
"""
import numpy as np
import torch

import splat_grad_ref as R

TILE = R.TILE
GRAD_KEYS = R.GRAD_KEYS
# |d means| of the depth part over the colour part with a unit-normal dL_dinv is 0.077 (posed) to 0.31 (deep_stop) in
# the float64 reference: 1 / d is about 0.15 where a colour is about 0.5. 5 puts every case between 0.38 and 1.6.
DINV_SCALE = 5.0
_DINV_SEED = {k: v + 500 for k, v in R._DL_SEED.items()}


def view_depth(means, view, dtype):
    """d = -(view * mean).z for means [n, 3] (torch), view the ubo's column-major float[16]."""
    V = torch.tensor(np.asarray(view, np.float64).reshape(4, 4).T, dtype=dtype)
    return -(means @ V[2, :3] + V[2, 3])


def evaluate(g, ubo, W, H, bg, frame, dL_dout, dL_dinv, dtype=torch.float64, border=None):
    """g: dict of numpy arrays; frame: oracle.splat_gaussians(g, ubo, W, H, bg); dL_dout [H, W, 4], dL_dinv [H, W].
    Returns {"image" [H, W, 4], "invdepth" [H, W], "grads" / "grads_color" / "grads_depth" {GRAD_KEYS + "invd":
    numpy float64}, "borderline", "border_pixels" [H, W] bool (as splat_grad_ref.evaluate counts them), "clamped",
    "stopped", "empty" [H, W] bool: the pixels of tiles without a list}.
    "invd" is dL/d(1 / d) per Gaussian, the tenth sum of the blend backward.
    border: the relative window around a threshold that counts as borderline (default splat_grad_ref.BORDER)."""
    border = R.BORDER if border is None else border
    n = g["means"].shape[0]
    leaf = {k: torch.tensor(np.asarray(g[k], np.float64), dtype=dtype, requires_grad=True)
            for k in ("means", "scales", "rotations", "opacities", "colors")}
    vis = np.flatnonzero(frame["radii"] > 0)
    slot = np.full(n, -1, np.int64)
    slot[vis] = np.arange(len(vis))
    vt = torch.from_numpy(vis)
    m2d, conic = R._project(leaf["means"][vt], leaf["scales"][vt], leaf["rotations"][vt], ubo.view, ubo.proj, W, H)
    invd = 1.0 / view_depth(leaf["means"][vt], ubo.view, dtype)
    opac, cols = leaf["opacities"][vt], leaf["colors"][vt]
    bgt = torch.tensor(np.asarray(bg, np.float64), dtype=dtype)
    go = torch.tensor(np.asarray(dL_dout, np.float64), dtype=dtype)
    gd = torch.tensor(np.asarray(dL_dinv, np.float64), dtype=dtype)
    gx_t, gy_t = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ranges = np.asarray(frame["ranges"]).reshape(-1, 2)
    image = torch.zeros((H, W, 4), dtype=dtype)
    depth = torch.zeros((H, W), dtype=dtype)
    empty = np.zeros((H, W), bool)
    loss_c = torch.zeros((), dtype=dtype)
    loss_d = torch.zeros((), dtype=dtype)
    borderline = clamped_n = stopped_n = 0
    border_pixels = np.zeros((H, W), bool)
    for t in range(gx_t * gy_t):
        ty_, tx_ = divmod(t, gx_t)
        ys = torch.arange(ty_ * TILE, min(H, (ty_ + 1) * TILE))
        xs = torch.arange(tx_ * TILE, min(W, (tx_ + 1) * TILE))
        py, px = torch.meshgrid(ys, xs, indexing="ij")
        py, px = py.reshape(-1), px.reshape(-1)
        ids = frame["vals"][ranges[t, 0]:ranges[t, 1]].astype(np.int64)
        npx = px.numel()
        if len(ids) == 0:
            rgba = torch.cat([bgt.expand(npx, 3), torch.zeros((npx, 1), dtype=dtype)], 1)
            D = torch.zeros(npx, dtype=dtype)
            empty[py.numpy(), px.numpy()] = True
        else:
            s = torch.from_numpy(slot[ids])
            assert int(s.min()) >= 0  # a listed Gaussian is visible
            dx = px.to(dtype)[:, None] - m2d[s, 0][None, :]
            dy = py.to(dtype)[:, None] - m2d[s, 1][None, :]
            a, b, c = conic[s, 0][None, :], conic[s, 1][None, :], conic[s, 2][None, :]
            power = -0.5 * (a * dx * dx + c * dy * dy) - b * dx * dy
            e = opac[s][None, :] * torch.exp(power)
            ed = e.detach()
            skip = ed < 1.0 / 255.0
            clamp = ed > 0.99
            alpha = torch.where(clamp, torch.full_like(e, 0.99), e)
            alpha = torch.where(skip, torch.zeros_like(e), alpha)
            # the stop: the first entry whose T - alpha T falls below 1e-4 ends the pixel (before it)
            keep = torch.cumprod(1.0 - alpha.detach(), 1)
            stop = keep < 1e-4
            first = torch.where(stop.any(1), stop.to(torch.int64).argmax(1), torch.full((npx,), len(ids)))
            pos = torch.arange(len(ids))[None, :]
            active = pos < first[:, None]
            seen = pos <= first[:, None]  # evaluated entries (the stopping one included)
            near_skip = seen & ((ed * 255.0 - 1.0).abs() < border)
            near_clamp = seen & ((ed / 0.99 - 1.0).abs() < border)
            near_stop = (seen & ((keep / 1e-4 - 1.0).abs() < border)).any(1)
            borderline += int(near_skip.sum()) + int(near_clamp.sum()) + int(near_stop.sum())
            border_pixels[py.numpy(), px.numpy()] = (near_skip.any(1) | near_clamp.any(1) | near_stop).numpy()
            clamped_n += int((active & clamp & ~skip).sum())
            stopped_n += int(stop.any(1).sum())
            alpha = alpha * active.to(dtype)
            Tincl = torch.cumprod(1.0 - alpha, 1)
            Texcl = torch.cat([torch.ones((npx, 1), dtype=dtype), Tincl[:, :-1]], 1)
            wgt = alpha * Texcl
            Tf = Tincl[:, -1]
            rgb = wgt @ cols[s] + Tf[:, None] * bgt[None, :]
            rgba = torch.cat([rgb, (1.0 - Tf)[:, None]], 1)
            D = wgt @ invd[s]
        image[py, px] = rgba.detach()
        depth[py, px] = D.detach()
        loss_c = loss_c + (rgba * go[py, px]).sum()
        loss_d = loss_d + (D * gd[py, px]).sum()

    def grads_of(scalar):
        out = {k: np.zeros(tuple(v.shape), np.float64) for k, v in leaf.items()}
        out["means2d"], out["conics"], out["invd"] = np.zeros((n, 2)), np.zeros((n, 3)), np.zeros(n)
        if scalar.requires_grad and len(vis):
            wrt = list(leaf.values()) + [m2d, conic, invd]
            got = torch.autograd.grad(scalar, wrt, retain_graph=True, allow_unused=True)
            for k, v in zip(leaf, got):
                if v is not None:
                    out[k] = v.double().numpy().copy()
            for k, v in zip(("means2d", "conics", "invd"), got[len(leaf):]):
                if v is not None:
                    out[k][vis] = v.double().numpy()
        return out

    return {"image": image.double().numpy(), "invdepth": depth.double().numpy(), "empty": empty,
            "grads": grads_of(loss_c + loss_d), "grads_color": grads_of(loss_c), "grads_depth": grads_of(loss_d),
            "borderline": borderline, "border_pixels": border_pixels, "clamped": clamped_n, "stopped": stopped_n}


def make_dinv(name, W, H):
    rng = np.random.default_rng(_DINV_SEED[name])
    return (rng.normal(size=(H, W)) * DINV_SCALE).astype(np.float32)


_CACHE = {}


def case_reference(name, oracle):
    """The case of splat_grad_ref with its upstream inverse-depth gradient "dinv" and the float64 / float32
    reference runs "r64" / "r32" (computed once per session). The oracle frame is splat_grad_ref's own."""
    if name not in _CACHE:
        base = R.case_reference(name, oracle)
        c = {k: base[k] for k in ("name", "g", "ubo", "W", "H", "bg", "dL", "frame")}
        c["dinv"] = make_dinv(name, c["W"], c["H"])
        for key, dt in (("r64", torch.float64), ("r32", torch.float32)):
            c[key] = evaluate(c["g"], c["ubo"], c["W"], c["H"], c["bg"], c["frame"], c["dL"], c["dinv"], dt)
        _CACHE[name] = c
    return _CACHE[name]


_FRAME_DINV_SEED = {k: v + 500 for k, v in R._FRAME_DL_SEED.items()}
_FRAME_CACHE = {}


def frame_case_reference(name, oracle):
    """case_reference() for a splat_grad_ref.FRAME_CASES entry. "dL" is splat_grad_ref's masked one and "dinv" is
    exactly 0 on the same "mask" (the border_pixels of splat_grad_ref's first float64 evaluation; this module's
    evaluate() takes the same decisions, tests/test_splat_depth_ref.py compares the two masks)."""
    if name not in _FRAME_CACHE:
        base = R.frame_case_reference(name, oracle)
        c = {k: base[k] for k in ("name", "g", "ubo", "W", "H", "bg", "dL", "frame", "mask")}
        rng = np.random.default_rng(_FRAME_DINV_SEED[name])
        c["dinv"] = (rng.normal(size=(c["H"], c["W"])) * DINV_SCALE).astype(np.float32)
        c["dinv"][c["mask"]] = 0.0
        for key, dt in (("r64", torch.float64), ("r32", torch.float32)):
            c[key] = evaluate(c["g"], c["ubo"], c["W"], c["H"], c["bg"], c["frame"], c["dL"], c["dinv"], dt)
        _FRAME_CACHE[name] = c
    return _FRAME_CACHE[name]


def part(c, which):
    """The case as splat_grad_ref.check_bounds / subsets read it, with "grads_color" or "grads_depth" (which) in
    the place of "grads": the bound and the subsets are then those of that part."""
    return dict(c, r64={"grads": c["r64"][which]}, r32={"grads": c["r32"][which]})


def invdepth_l1(D, t, weight=1.0, grad_scale=1.0):
    """ptgs_image_loss_invdepth_l1 restated: D, t float32 [H, W] (t a view depth). Returns (terms float64 [3] before
    their rounding to f32: (weight mean, mean, supervised pixels), grad float32 [H, W])."""
    D, t = np.asarray(D, np.float32), np.asarray(t, np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        sup = t > np.float32(0.0)  # (False for NaN; True for +inf)
        diff = (D - np.float32(1.0) / t).astype(np.float32)
    term = np.where(sup, np.abs(diff), np.float32(0.0)).astype(np.float32)
    mean = float(term.astype(np.float64).sum()) / float(D.size)
    k = np.float32(float(np.float32(weight)) * float(np.float32(grad_scale)) / float(D.size))  # (the C floats)
    grad = np.where(sup, k * np.sign(diff), np.float32(0.0)).astype(np.float32)
    return np.array([float(np.float32(weight)) * mean, mean, float(sup.sum())]), grad
