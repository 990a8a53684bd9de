"""Reference for the 3DGS backward pass (ptgs_splat_gaussians_backward), independent of the code under test.

The function differentiated is the forward as ptgs.h states it. Membership and order (which Gaussians each
tile holds, in which order) come from the CPU oracle's frame (oracle.splat_gaussians: ranges, vals); the
projection is written out as in gs_preprocess_one and the blend is evaluated tile by tile, 256 pixels x
the tile's list, in torch on the CPU (float64 by default). The discrete decisions (alpha < 1/255 skip,
T < 1e-4 stop, the 0.99 clamp) are taken from a detached evaluation and applied as masks; torch.autograd
gives the gradients. evaluate() also counts the borderline decisions, so that the tests can insist on
cases without any (a decision within 1e-3 relative of its threshold could fall either way in float32).

The cases of tests/test_splat_grad_ref.py (CPU) and tests/test_splat_backward_gpu.py (GPU) are built here, and the
training-size FRAME_CASES of tests/test_splat_backward_frames_gpu.py, whose borderline pixels take no part.
"""
import numpy as np
import torch

from pathtracer_gaussiansplatting_amd import Camera, Ubo
from pathtracer_gaussiansplatting_amd import synthetic as Y

TILE = 16
BORDER = 1e-3
GRAD_KEYS = ("colors", "opacities", "means2d", "conics", "means", "scales", "rotations")


def make_ubo(W, H, eye=(0.0, 0.0, 0.0), center=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0)):
    """Camera.look_at(eye, center, up) with aspect W / H; the default is the identity camera at the origin looking
    down -Z (synthetic.gaussians_c2's frame)."""
    pose = Camera(aspect=W / H).look_at(list(eye), list(center), list(up))
    u = Ubo()
    u.view[:] = [float(x) for x in pose.view]
    u.proj[:] = [float(x) for x in pose.proj]
    return u


def _project(means, scales, rots, view, proj, W, H):
    """gs_preprocess_one for the given (visible) Gaussians: means2d [n, 2], conic [n, 3] (a, b, c)."""
    dt = means.dtype
    V = torch.tensor(np.asarray(view, np.float64).reshape(4, 4).T, dtype=dt)  # row-major
    P = torch.tensor(np.asarray(proj, np.float64).reshape(4, 4).T, dtype=dt)
    MVP = P @ V
    ones = torch.ones_like(means[:, :1])
    mh = torch.cat([means, ones], 1)
    pv = mh @ V.T
    ph = mh @ MVP.T
    d = -pv[:, 2]
    pw = 1.0 / (ph[:, 3] + 1e-7)
    m2d = torch.stack([((ph[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((ph[:, 1] * pw + 1.0) * H - 1.0) * 0.5], 1)
    q = rots / rots.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = R * scales[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    p00, p11 = float(proj[0]), float(proj[5])
    fx, fy = p00 * W * 0.5, p11 * H * 0.5
    limx, limy = 1.3 / p00, 1.3 / abs(p11)
    tx = torch.clamp(pv[:, 0] / d, -limx, limx) * d  # (autograd: a clamped tx depends on the mean through d only)
    ty = torch.clamp(pv[:, 1] / d, -limy, limy) * d
    zero = torch.zeros_like(d)
    J = torch.stack([fx / d, zero, fx * tx / (d * d), zero, fy / d, fy * ty / (d * d)], 1).reshape(-1, 2, 3)
    T = J @ V[:3, :3]
    cov = T @ Sigma @ T.transpose(1, 2)
    ca, cb, cc = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = ca * cc - cb * cb
    conic = torch.stack([cc / det, -cb / det, ca / det], 1)
    return m2d, conic


def evaluate(g, ubo, W, H, bg, frame, dL_dout, dtype=torch.float64):
    """g: dict of float32 numpy arrays; frame: oracle.splat_gaussians(g, ubo, W, H, bg); dL_dout [H, W, 4].
    Returns {"image" [H, W, 4], "grads" {GRAD_KEYS: numpy float64}, "borderline", "border_pixels", "clamped",
    "stopped", "tiles"}: borderline = pairs whose o exp(power) lies within 1e-3 relative of 1/255 or of 0.99 +
    pixels whose stop test lies within 1e-3 relative of 1e-4; border_pixels = bool [H, W], the pixels with any
    of these among their evaluated entries; clamped = pairs blended at 0.99; stopped = pixels that stop
    on T < 1e-4; tiles = per tile {"n": the list's length, "first": per pixel inside the image the position of
    the entry that stops it (n: none), "quads": per entry the 8x8 quadrants (bit (x >= 8) + 2 (y >= 8)) holding a
    pixel that evaluates it with alpha >= 1/255}."""
    n = g["means"].shape[0]
    leaf = {k: torch.tensor(np.asarray(g[k], np.float64), dtype=dtype, requires_grad=True)
            for k in ("means", "scales", "rotations", "opacities", "colors")}
    vis = np.flatnonzero(frame["radii"] > 0)
    slot = np.full(n, -1, np.int64)
    slot[vis] = np.arange(len(vis))
    vt = torch.from_numpy(vis)
    m2d, conic = _project(leaf["means"][vt], leaf["scales"][vt], leaf["rotations"][vt], ubo.view, ubo.proj, W, H)
    if m2d.requires_grad:  # (not under torch.no_grad(): a run for the image and the counts alone)
        m2d.retain_grad()
        conic.retain_grad()
    opac, cols = leaf["opacities"][vt], leaf["colors"][vt]
    bgt = torch.tensor(np.asarray(bg, np.float64), dtype=dtype)
    go = torch.tensor(np.asarray(dL_dout, np.float64), dtype=dtype)
    gx_t, gy_t = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ranges = np.asarray(frame["ranges"]).reshape(-1, 2)
    image = torch.zeros((H, W, 4), dtype=dtype)
    loss = torch.zeros((), dtype=dtype)
    borderline = clamped_n = stopped_n = 0
    border_pixels = np.zeros((H, W), bool)
    tiles = []
    for t in range(gx_t * gy_t):
        ty_, tx_ = divmod(t, gx_t)
        ys = torch.arange(ty_ * TILE, min(H, (ty_ + 1) * TILE))
        xs = torch.arange(tx_ * TILE, min(W, (tx_ + 1) * TILE))
        py, px = torch.meshgrid(ys, xs, indexing="ij")
        py, px = py.reshape(-1), px.reshape(-1)
        ids = frame["vals"][ranges[t, 0]:ranges[t, 1]].astype(np.int64)
        npx = px.numel()
        tiles.append({"n": len(ids), "first": np.zeros(npx, np.int64), "quads": np.zeros(len(ids), np.uint8)})
        if len(ids) == 0:
            rgba = torch.cat([bgt.expand(npx, 3), torch.zeros((npx, 1), dtype=dtype)], 1)
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
            near_skip = seen & ((ed * 255.0 - 1.0).abs() < BORDER)
            near_clamp = seen & ((ed / 0.99 - 1.0).abs() < BORDER)
            near_stop = (seen & ((keep / 1e-4 - 1.0).abs() < BORDER)).any(1)
            borderline += int(near_skip.sum()) + int(near_clamp.sum()) + int(near_stop.sum())
            border_pixels[py.numpy(), px.numpy()] = (near_skip.any(1) | near_clamp.any(1) | near_stop).numpy()
            clamped_n += int((active & clamp & ~skip).sum())
            stopped_n += int(stop.any(1).sum())
            tiles[t]["first"] = first.numpy().copy()
            quad = ((px % TILE) >= 8).to(torch.int64) + 2 * ((py % TILE) >= 8).to(torch.int64)
            hit = seen & ~skip
            for qd in range(4):
                tiles[t]["quads"] |= (hit[quad == qd].any(0).numpy().astype(np.uint8) << qd)
            alpha = alpha * active.to(dtype)
            one_m = 1.0 - alpha
            Tincl = torch.cumprod(one_m, 1)
            Texcl = torch.cat([torch.ones((npx, 1), dtype=dtype), Tincl[:, :-1]], 1)
            wgt = alpha * Texcl
            Tf = Tincl[:, -1]
            rgb = wgt @ cols[s] + Tf[:, None] * bgt[None, :]
            rgba = torch.cat([rgb, (1.0 - Tf)[:, None]], 1)
        image[py, px] = rgba.detach()
        loss = loss + (rgba * go[py, px]).sum()
    grads = {k: np.zeros(tuple(v.shape), np.float64) for k, v in leaf.items()}
    grads["means2d"] = np.zeros((n, 2), np.float64)
    grads["conics"] = np.zeros((n, 3), np.float64)
    if loss.requires_grad and len(vis):
        loss.backward()
        for k, v in leaf.items():
            if v.grad is not None:
                grads[k] = v.grad.double().numpy().copy()
        if m2d.grad is not None:
            grads["means2d"][vis] = m2d.grad.double().numpy()
            grads["conics"][vis] = conic.grad.double().numpy()
    return {"image": image.double().numpy(), "grads": grads, "borderline": borderline,
            "border_pixels": border_pixels, "clamped": clamped_n, "stopped": stopped_n, "tiles": tiles}


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------------------
# cases: built from synthetic.gaussians_c2 with scales enlarged as needed (the structural properties are
# asserted by the tests from the oracle's frame and the reference, never assumed). The seeds are ones for which
# the reference counts no borderline decision (tests/test_splat_grad_ref.py checks it).
# ---------------------------------------------------------------------------------------------------------
BG = (0.1, 0.2, 0.3)


def _case_edges(seed=7):
    """(a) 40x24: partial tiles on both edges, empty tiles, a Gaussian inside the near plane and one behind."""
    g = Y.gaussians_c2(40, seed=seed)
    g["means"][:, 0] = np.abs(g["means"][:, 0]) * 0.9 + 0.6  # the right part of the view: the left tiles stay empty
    g["scales"] *= 4.0
    g["means"][5] = [0.02, 0.01, -0.1]   # d = 0.1 <= 0.2
    g["means"][9] = [0.3, -0.2, 3.0]     # behind the camera
    return g, 40, 24


def _case_batches(seed=22):
    """(b) 64x48: a tile above 256 pairs (two batches) next to sparse ones, Gaussians spanning >= 4 tiles."""
    g = Y.gaussians_c2(520, seed=seed)
    g["means"][:420, 0] = g["means"][:420, 0] * 0.1 - 2.6  # a dense cluster inside one tile
    g["means"][:420, 1] = g["means"][:420, 1] * 0.15 + 1.3
    g["means"][:420, 2] = g["means"][:420, 2] * 0.25 - 6.0
    g["scales"][500:] *= 12.0  # a few wide ones: rects over several tiles
    g["means"][500:, 0] *= 0.5
    return g, 64, 48


def _case_opaque(seed=14):
    """(c) 32x32: opacities of exactly 1.0 in dense layers: pairs clamped at 0.99 and pixels that stop."""
    g = Y.gaussians_c2(120, seed=seed)
    g["means"][:, 0] *= 0.25
    g["means"][:, 1] *= 0.25
    g["scales"] *= 8.0
    g["opacities"][:40] = 1.0
    return g, 32, 32


# The posed cases: an off-axis eye, a centre off the box axis and a tilted up vector, so that every entry of the
# view rotation and the translation are non-zero (asserted by the tests). A case that returns a pose is rendered
# with it; its Gaussians are placed in camera space (pixel, depth) and moved to the world with the inverse view.
POSE = ((5.0, 2.5, 1.0), (0.3, -0.2, -8.0), (0.4, 1.0, 0.1))


def _view_proj(W, H, pose):
    u = make_ubo(W, H, *pose)
    return (np.asarray(u.view, np.float64).reshape(4, 4).T, np.asarray(u.proj, np.float64).reshape(4, 4).T)


def _cam_to_world(cam_pts, view):
    inv = np.linalg.inv(view)
    return np.asarray(cam_pts, np.float64) @ inv[:3, :3].T + inv[:3, 3]


def _pixels_to_cam(px, py, d, proj, W, H):
    """Camera-space points that project to the pixel coordinates (px, py) at view depth d."""
    px, py, d = (np.asarray(v, np.float64) for v in (px, py, d))
    return np.stack([((2.0 * px + 1.0) / W - 1.0) * d / proj[0, 0], ((2.0 * py + 1.0) / H - 1.0) * d / proj[1, 1],
                     -d], -1)


def _small_in_tile(rng, n, tile_x, tile_y, W, H, view, proj, opac, depth=(5.0, 9.0), box=(4.5, 10.5),
                   sigma_px=(0.1, 0.5)):
    """n small Gaussians whose means fall at tile-local pixels `box` of one tile, so that their 3-sigma rects
    (radius <= 4 px) touch that tile only; sigma_px: the scales' range in pixels (before the 0.3 dilation)."""
    px = 16 * tile_x + rng.uniform(box[0], box[1], n)
    py = 16 * tile_y + rng.uniform(box[0], box[1], n)
    d = rng.uniform(depth[0], depth[1], n)
    fx = proj[0, 0] * W * 0.5
    return {"means": _cam_to_world(_pixels_to_cam(px, py, d, proj, W, H), view),
            "scales": rng.uniform(sigma_px[0], sigma_px[1], (n, 3)) * (d / fx)[:, None],
            "rotations": rng.normal(size=(n, 4)),
            "opacities": rng.uniform(opac[0], opac[1], n),
            "colors": rng.uniform(0.0, 1.0, (n, 3))}


def _concat(parts):
    return {k: np.concatenate([np.asarray(p[k]) for p in parts], 0) for k in parts[0]}


def _case_posed(seed=1):
    """(e) 44x40 at POSE: partial tiles, the view a general rotation and translation. Gaussian 11 has opacity
    exactly 0.0 (exactly zero gradients), Gaussian 23 a rotation scaled by 1e-3 (the / |q| path)."""
    g = Y.gaussians_c2(150, seed=seed)
    g["scales"] *= 6.0
    g["opacities"][11] = 0.0
    g["rotations"][23] *= 1e-3
    return g, 44, 40, POSE


CLAMP_WIDE = 6  # the last Gaussians of the case clamp: 2 beyond the clamp in x only, 2 in y only, 2 in both


def _case_clamp(seed=23):
    """(f) 48x40 at POSE: six Gaussians outside the frustum at |x / d| and / or |y / d| of 1.35 to 1.6 half-angle
    tangents (the EWA clamp acts at 1.3), wide enough to reach the image."""
    W, H = 48, 40
    g = Y.gaussians_c2(80, seed=seed)
    g["scales"] *= 3.0
    view, proj = _view_proj(W, H, POSE)
    rng = np.random.default_rng(5000 + seed)
    tanx, tany = 1.0 / proj[0, 0], 1.0 / abs(proj[1, 1])
    d = rng.uniform(5.0, 9.0, CLAMP_WIDE)
    beyond = rng.uniform(1.35, 1.6, (CLAMP_WIDE, 2)) * rng.choice([-1.0, 1.0], (CLAMP_WIDE, 2))
    within = rng.uniform(-0.8, 0.8, (CLAMP_WIDE, 2))
    fx = np.where(np.array([1, 1, 0, 0, 1, 1], bool), beyond[:, 0], within[:, 0])
    fy = np.where(np.array([0, 0, 1, 1, 1, 1], bool), beyond[:, 1], within[:, 1])
    cam = np.stack([fx * tanx * d, fy * tany * d, -d], -1)
    wide = {"means": _cam_to_world(cam, view), "scales": rng.uniform(0.5, 1.2, (CLAMP_WIDE, 3)),
            "rotations": rng.normal(size=(CLAMP_WIDE, 4)), "opacities": rng.uniform(0.3, 0.9, CLAMP_WIDE),
            "colors": rng.uniform(0.0, 1.0, (CLAMP_WIDE, 3))}
    return _concat([g, wide]), W, H, POSE


CHUNK_TILES = {(0, 0): 64, (2, 0): 65, (1, 2): 256, (3, 2): 257}  # (tile x, tile y): the list's length


def _case_chunks(seed=23):
    """(g) 60x44 at POSE: four tiles whose lists hold exactly 64, 65, 256 and 257 pairs (the reduction round's
    and the staged batch's boundaries), small Gaussians of low opacity that touch their own tile only."""
    W, H = 60, 44
    view, proj = _view_proj(W, H, POSE)
    rng = np.random.default_rng(6000 + seed)
    parts = [_small_in_tile(rng, n, tx, ty, W, H, view, proj, (0.05, 0.35)) for (tx, ty), n in CHUNK_TILES.items()]
    return _concat(parts), W, H, POSE


DEEP_WALK_TILE, DEEP_MIXED_TILE = (0, 0), (2, 1)


def _case_deep(seed=48):
    """(h) 48x32 at POSE: tile (0, 0) holds 530 faint pairs (three batches, pixels that never stop); tile (2, 1)
    holds 50 layers of opacity 0.8 over one corner in front of 250 faint pairs (pixels that stop inside the
    first batch next to pixels that walk into the second)."""
    W, H = 48, 32
    view, proj = _view_proj(W, H, POSE)
    rng = np.random.default_rng(7000 + seed)
    walk = _small_in_tile(rng, 530, *DEEP_WALK_TILE, W, H, view, proj, (0.02, 0.12))
    front = _small_in_tile(rng, 50, *DEEP_MIXED_TILE, W, H, view, proj, (0.8, 0.8), depth=(3.0, 4.0), box=(4.5, 6.5),
                           sigma_px=(0.3, 0.6))
    back = _small_in_tile(rng, 250, *DEEP_MIXED_TILE, W, H, view, proj, (0.05, 0.35))
    return _concat([walk, front, back]), W, H, POSE


def _case_deep_stop(seed=2):
    """(i) 16x16 at POSE, one tile: 120 layers of opacity 0.8, each wide enough to cover the tile (their alpha
    1/255 contour lies outside the image), in front of 180 faint pairs: every pixel stops inside the first batch
    of a list of 300."""
    W, H = 16, 16
    view, proj = _view_proj(W, H, POSE)
    rng = np.random.default_rng(8000 + seed)
    front = _small_in_tile(rng, 120, 0, 0, W, H, view, proj, (0.8, 0.8), depth=(3.0, 4.0), box=(5.0, 10.0),
                           sigma_px=(7.0, 9.0))
    back = _small_in_tile(rng, 180, 0, 0, W, H, view, proj, (0.05, 0.35))
    return _concat([front, back]), W, H, POSE


CASES = {"edges": _case_edges, "batches": _case_batches, "opaque": _case_opaque, "posed": _case_posed,
         "clamp": _case_clamp, "chunks": _case_chunks, "deep": _case_deep, "deep_stop": _case_deep_stop}
_DL_SEED = {"batches": 1000, "edges": 1001, "opaque": 1002, "posed": 1003, "clamp": 1004, "chunks": 1005,
            "deep": 1006, "deep_stop": 1007}


def make_case(name, **kw):
    """(g, ubo, W, H, bg, dL_dout): (d) every case has a non-zero background and a seeded random-normal upstream
    gradient on all four channels."""
    g, W, H, *pose = CASES[name](**kw)
    g = {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}
    rng = np.random.default_rng(_DL_SEED[name])
    dL = rng.normal(size=(H, W, 4)).astype(np.float32)
    return g, make_ubo(W, H, *(pose[0] if pose else ())), W, H, BG, dL


# ---------------------------------------------------------------------------------------------------------
# frame cases: training-size frames (tens of thousands of pairs, lists of several staged batches, tile indices
# beyond 64). At that size some evaluated alpha always lies within BORDER of a threshold, so these cases do not
# insist on zero borderline decisions: frame_case_reference() sets the upstream gradient to exactly 0 at the
# pixels where the float64 reference counts one (evaluate()'s "border_pixels"). A pixel with a zero upstream
# gradient contributes exactly nothing to any gradient, whichever way its decisions fall, so the comparison on
# all other pixels needs no allowance for decisions. They are kept apart from CASES, whose tests assert
# borderline == 0.
# ---------------------------------------------------------------------------------------------------------
def tile_order(g, W, H, pose=()):
    """The Gaussians reordered by the 16x16 tile of their 2D mean (projected in float64, clipped to the grid),
    row-major and stable: the order a trainer gives its parameters to stay on the fused front end (the backward
    refuses `ids`, so the spatial order is the caller's)."""
    view, proj = _view_proj(W, H, pose)
    ph = np.c_[np.asarray(g["means"], np.float64), np.ones(len(g["means"]))] @ (proj @ view).T
    pw = 1.0 / (ph[:, 3] + 1e-7)
    mx, my = ((ph[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((ph[:, 1] * pw + 1.0) * H - 1.0) * 0.5
    gx, gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    tx = np.clip(np.floor(mx / TILE), 0, gx - 1).astype(np.int64)
    ty = np.clip(np.floor(my / TILE), 0, gy - 1).astype(np.int64)
    order = np.argsort(ty * gx + tx, kind="stable")
    return {k: np.asarray(v)[order] for k, v in g.items()}


def _frame_field(seed=9):
    """320x180, 20x12 tiles with a partial bottom row: 20000 Gaussians, tens of thousands of pairs, dozens of lists
    above 256 and above 512 pairs, 79 workgroups of the projection backward."""
    W, H = 320, 180
    return tile_order(Y.gaussians_c2(20000, seed=seed), W, H), W, H


def _frame_layers(seed=9):
    """208x120: scales x3 and every third opacity exactly 1.0: pixels that stop and pairs blended at 0.99 in
    quantity, all over the image."""
    W, H = 208, 120
    g = Y.gaussians_c2(8000, seed=seed)
    g["scales"] = g["scales"] * np.float32(3.0)
    g["opacities"][::3] = 1.0
    return tile_order(g, W, H), W, H


def _frame_crowd(seed=9):
    """160x96: the field's Gaussians on a quarter of its pixels: lists above 2048 pairs (more than eight staged
    batches), above the fused rows' capacity."""
    W, H = 160, 96
    return tile_order(Y.gaussians_c2(20000, seed=seed), W, H), W, H


# (tile x, tile y): Gaussians placed there. wide: 125 x 3 tiles (the last column and the last row partial);
# tall: 3 x 69 tiles (likewise). The partial tiles' means lie inside the image (box).
WIDE_TILES = {(0, 0): 40, (63, 1): 70, (64, 1): 130, (123, 0): 300, (124, 2): 60}
TALL_TILES = {(0, 0): 40, (1, 33): 70, (2, 67): 280, (1, 68): 300}


def _frame_placed(W, H, placed, seed):
    view, proj = _view_proj(W, H, POSE)
    rng = np.random.default_rng(seed)
    parts = []
    for (tx, ty), n in placed.items():
        partial = 16 * (tx + 1) > W or 16 * (ty + 1) > H
        parts.append(_small_in_tile(rng, n, tx, ty, W, H, view, proj, (0.05, 0.35),
                                    box=(1.5, 6.5) if partial else (4.5, 10.5)))
    return _concat(parts), W, H, POSE


def _frame_wide(seed=31):
    """1992x40 at POSE: pixel x up to 1991 (float32 resolves 1.2e-4 there), grid_x = 125."""
    return _frame_placed(1992, 40, WIDE_TILES, 9000 + seed)


def _frame_tall(seed=32):
    """40x1096 at POSE: pixel y up to 1095, grid_y = 69 with grid_x = 3."""
    return _frame_placed(40, 1096, TALL_TILES, 9000 + seed)


FRAME_CASES = {"field": _frame_field, "layers": _frame_layers, "crowd": _frame_crowd, "wide": _frame_wide,
               "tall": _frame_tall}
_FRAME_DL_SEED = {"field": 1100, "layers": 1101, "crowd": 1102, "wide": 1103, "tall": 1104}
MASK_CAP = 0.01  # at most this share of a frame case's pixels may be masked (a cap, not a measurement)


def make_frame_case(name):
    """(g, ubo, W, H, bg, dL_dout) of a FRAME_CASES entry, dL_dout not yet masked."""
    g, W, H, *pose = FRAME_CASES[name]()
    g = {k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}
    rng = np.random.default_rng(_FRAME_DL_SEED[name])
    dL = rng.normal(size=(H, W, 4)).astype(np.float32)
    return g, make_ubo(W, H, *(pose[0] if pose else ())), W, H, BG, dL


def touched_runs(frame, W, H):
    """The (256-Gaussian chunk, tile) runs the frame's pairs touch, as the front ends count them."""
    ranges = np.asarray(frame["ranges"]).reshape(-1, 2).astype(np.int64)
    tile = np.repeat(np.arange(len(ranges)), ranges[:, 1] - ranges[:, 0])
    vals = np.concatenate([np.asarray(frame["vals"][a:b], np.int64) for a, b in ranges]) if len(ranges) else tile
    return len(np.unique(tile * (1 << 32) + vals // 256))


def ewa_clamped(g, ubo, frame):
    """(in x, in y): per Gaussian, visible in the oracle frame and beyond the EWA clamp (|pv.x / d| > 1.3 / P00,
    |pv.y / d| > 1.3 / |P11|), computed in float64 from the ubo."""
    view = np.asarray(ubo.view, np.float64).reshape(4, 4).T
    pv = np.c_[np.asarray(g["means"], np.float64), np.ones(len(g["means"]))] @ view.T
    d = -pv[:, 2]
    vis = np.asarray(frame["radii"]) > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        cx = np.abs(pv[:, 0] / d) > 1.3 / float(ubo.proj[0])
        cy = np.abs(pv[:, 1] / d) > 1.3 / abs(float(ubo.proj[5]))
    return vis & cx, vis & cy


def subsets(c, key):
    """[(label, indices)]: the subsets of Gaussians on which the error bound is checked besides the whole array:
    each quarter of the visible Gaussians ranked by the norm of their float64 reference gradient in `key` (q1: the
    smallest), and the Gaussians beyond the EWA clamp where there are any."""
    ref = c["r64"]["grads"][key]
    vis = np.flatnonzero(np.asarray(c["frame"]["radii"]) > 0)
    order = vis[np.argsort(np.linalg.norm(ref[vis].reshape(len(vis), -1), axis=1), kind="stable")]
    out = [(f"q{i + 1}", part) for i, part in enumerate(np.array_split(order, 4))]
    cx, cy = ewa_clamped(c["g"], c["ubo"], c["frame"])
    if (cx | cy).any():
        out.append(("clamped", np.flatnonzero(cx | cy)))
    return out


def check_bounds(c, key, got, label):
    """Relative L2 of `got` against the float64 reference in `key`, on the whole array and on every subset,
    each against max(1e-4, 8 e32) with e32 the float32 reference's error on the same rows. Prints every value;
    returns the failures."""
    ref, r32 = c["r64"]["grads"][key], c["r32"]["grads"][key]
    got = np.asarray(got, np.float64).reshape(ref.shape)
    failed = []
    for name, idx in [("all", np.arange(len(ref)))] + subsets(c, key):
        e32 = rel_l2(r32[idx], ref[idx])
        bound = max(1e-4, 8.0 * e32)
        err = rel_l2(got[idx], ref[idx])
        print(f"{c['name']} {key} {name} ({len(idx)}): {label} rel L2 {err:.2e}  e32 {e32:.2e}  bound {bound:.1e}")
        if not err <= bound:
            failed.append((key, name, err, bound))
    return failed


_CACHE = {}


def case_reference(name, oracle):
    """The case, its oracle frame and its float64 / float32 reference runs (computed once per session)."""
    if name not in _CACHE:
        g, ubo, W, H, bg, dL = make_case(name)
        frame = oracle.splat_gaussians(g, ubo, W, H, bg=bg)
        r64 = evaluate(g, ubo, W, H, bg, frame, dL, torch.float64)
        r32 = evaluate(g, ubo, W, H, bg, frame, dL, torch.float32)
        _CACHE[name] = {"name": name, "g": g, "ubo": ubo, "W": W, "H": H, "bg": bg, "dL": dL, "frame": frame, "r64": r64, "r32": r32}
    return _CACHE[name]


_FRAME_CACHE = {}


def frame_case_reference(name, oracle):
    """case_reference() for a FRAME_CASES entry, plus "mask": the border_pixels of a first float64 evaluation.
    "dL" is exactly 0 there, and "r64" / "r32" are computed with that masked gradient. The mask comes from the
    float64 reference alone."""
    if name not in _FRAME_CACHE:
        g, ubo, W, H, bg, dL = make_frame_case(name)
        frame = oracle.splat_gaussians(g, ubo, W, H, bg=bg)
        with torch.no_grad():
            mask = evaluate(g, ubo, W, H, bg, frame, dL, torch.float64)["border_pixels"]
        dL[mask] = 0.0
        r64 = evaluate(g, ubo, W, H, bg, frame, dL, torch.float64)
        r32 = evaluate(g, ubo, W, H, bg, frame, dL, torch.float32)
        _FRAME_CACHE[name] = {"name": name, "g": g, "ubo": ubo, "W": W, "H": H, "bg": bg, "dL": dL, "frame": frame,
                              "mask": mask, "r64": r64, "r32": r32}
    return _FRAME_CACHE[name]
