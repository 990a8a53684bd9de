"""Reference for the camera-pose gradient of the 3DGS backward (ptgs_splat_gaussians_backward_pose and
ptgs_gaussians_sh_colors_backward_eye), independent of the code under test.

The blend depends on the view only through each visible Gaussian's 2D mean, conic and 1 / d. So
    dL/d view = the VJP of the projection (splat_grad_ref._project restated with V a leaf tensor, plus 1 / d)
                applied to the per-Gaussian cotangents "means2d", "conics", "invd" of splat_depth_ref.evaluate
in float64 as the reference and in float32 (the float32 run's own cotangents through the float32 projection) for
e32, the error float32 itself makes: the bound of the host and GPU tests is max(1e-4, 8 e32) per block (single
entries are off by up to 6e-5 of themselves in float32, so the bounds are on blocks). Row 3 of the view is held at
(0, 0, 0, 1): the gradient is the 3x4 of the rows 0..2, G[r][c] = dL/d view[r][c] in math indexing.

tests/test_splat_pose_grad_ref.py checks the chain against central finite differences of splat_depth_ref.evaluate.
"""
import numpy as np
import torch

import sh_grad_ref as S
import splat_depth_ref as Z
import splat_grad_ref as R
import splat_hard_grad_ref as HG

PARTS = ("grads", "grads_color", "grads_depth")
BLOCKS = {"all": (slice(0, 3), slice(0, 4)), "rotation": (slice(0, 3), slice(0, 3)),
          "translation": (slice(0, 3), slice(3, 4))}


def view_matrix(ubo):
    """The ubo's view as a float64 [4, 4] in math indexing (ptgs_ubo.view is column-major)."""
    return np.asarray(ubo.view, np.float64).reshape(4, 4).T.copy()


def project(means, scales, rots, V, proj, W, H):
    """splat_grad_ref._project with the view a torch tensor V [4, 4] (math indexing) that may be a leaf, proj the
    ubo's constant column-major float[16]. Returns (means2d [n, 2], conic [n, 3], 1 / d [n], pv [n, 4]); pv =
    (x, y, -d, 1) is the camera-space point."""
    dt = means.dtype
    P = torch.tensor(np.asarray(proj, np.float64).reshape(4, 4).T, dtype=dt)
    mh = torch.cat([means, torch.ones_like(means[:, :1])], 1)
    pv = mh @ V.T
    ph = mh @ (P @ V).T
    d = -pv[:, 2]
    pw = 1.0 / (ph[:, 3] + 1e-7)
    m2d = torch.stack([((ph[:, 0] * pw + 1.0) * W - 1.0) * 0.5, ((ph[:, 1] * pw + 1.0) * H - 1.0) * 0.5], 1)
    q = rots / rots.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    Rm = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                      2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                      2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    M = Rm * scales[:, None, :]
    Sigma = M @ M.transpose(1, 2)
    p00, p11 = float(proj[0]), float(proj[5])
    fx, fy = p00 * W * 0.5, p11 * H * 0.5
    limx, limy = 1.3 / p00, 1.3 / abs(p11)
    tx = torch.clamp(pv[:, 0] / d, -limx, limx) * d  # (autograd: a clamped tx depends on the view through d only)
    ty = torch.clamp(pv[:, 1] / d, -limy, limy) * d
    zero = torch.zeros_like(d)
    J = torch.stack([fx / d, zero, fx * tx / (d * d), zero, fy / d, fy * ty / (d * d)], 1).reshape(-1, 2, 3)
    T = J @ V[:3, :3]
    cov = T @ Sigma @ T.transpose(1, 2)
    ca, cb, cc = cov[:, 0, 0] + 0.3, cov[:, 0, 1], cov[:, 1, 1] + 0.3
    det = ca * cc - cb * cb
    conic = torch.stack([cc / det, -cb / det, ca / det], 1)
    return m2d, conic, 1.0 / d, pv


def view_grad(g, view, proj, W, H, vis, cot, dtype=torch.float64, per_gaussian=False):
    """dL/d view [3, 4] (numpy float64) from the cotangents cot = {"means2d", "conics", "invd"} (arrays over all
    Gaussians; the rows `vis` are used): the VJP of project() with the view a leaf, evaluated in `dtype`.
    per_gaussian: also dL/d pv [len(vis), 4], the gradient at each Gaussian's camera-space point."""
    vt = np.asarray(vis)
    leaf = [torch.tensor(np.asarray(g[k], np.float64)[vt], dtype=dtype) for k in ("means", "scales", "rotations")]
    V = torch.tensor(np.asarray(view, np.float64), dtype=dtype, requires_grad=True)
    if len(vt) == 0:
        return (np.zeros((3, 4)), np.zeros((0, 4))) if per_gaussian else np.zeros((3, 4))
    m2d, conic, invd, pv = project(*leaf, V, proj, W, H)
    c = [torch.tensor(np.asarray(cot[k], np.float64)[vt], dtype=dtype) for k in ("means2d", "conics", "invd")]
    scalar = (m2d * c[0]).sum() + (conic * c[1]).sum() + (invd * c[2]).sum()
    if per_gaussian:
        dV, dpv = torch.autograd.grad(scalar, [V, pv])
        return dV.double().numpy()[:3].copy(), dpv.double().numpy().copy()
    (dV,) = torch.autograd.grad(scalar, [V])
    return dV.double().numpy()[:3].copy()


_CACHE = {}


def _reference(c):
    vis = np.flatnonzero(c["frame"]["radii"] > 0)
    V = view_matrix(c["ubo"])
    out = {}
    for which in PARTS:
        out[which] = {"r64": view_grad(c["g"], V, c["ubo"].proj, c["W"], c["H"], vis, c["r64"][which], torch.float64),
                      "r32": view_grad(c["g"], V, c["ubo"].proj, c["W"], c["H"], vis, c["r32"][which], torch.float32)}
    return out


def case_reference(name, oracle):
    """splat_depth_ref.case_reference(name) plus "pose": {part: {"r64", "r32"}}, dL/d view [3, 4] of the full,
    the colour-only and the depth-only loss (computed once per session)."""
    if name not in _CACHE:
        c = dict(Z.case_reference(name, oracle))
        c["pose"] = _reference(c)
        _CACHE[name] = c
    return _CACHE[name]


_FRAME_CACHE = {}


def frame_case_reference(name, oracle):
    """case_reference() for a splat_grad_ref.FRAME_CASES entry (its masked upstream gradients)."""
    if name not in _FRAME_CACHE:
        c = dict(Z.frame_case_reference(name, oracle))
        c["pose"] = _reference(c)
        _FRAME_CACHE[name] = c
    return _FRAME_CACHE[name]


_HARD_CACHE = {}


def hard_case_reference(name):
    """splat_hard_grad_ref.case_reference(name) (the forward's hard cases, their own frame and masked upstream
    gradients) plus "pose"."""
    if name not in _HARD_CACHE:
        c = dict(HG.case_reference(name))
        c["pose"] = _reference(c)
        _HARD_CACHE[name] = c
    return _HARD_CACHE[name]


def check_blocks(ref, r32, got, label, cap=None):
    """Relative L2 of `got` [3, 4] against the float64 reference on the whole 3x4, the rotation block and the
    translation column, each against max(1e-4, 8 e32). Prints every value; returns the failures.
    cap: 8 e32 counts up to `cap` only (splat_hard_grad_ref.BOUND_CAP on the hard cases)."""
    got = np.asarray(got, np.float64).reshape(3, 4)
    failed = []
    for name, idx in BLOCKS.items():
        e32 = R.rel_l2(r32[idx], ref[idx])
        bound = max(1e-4, 8.0 * e32 if cap is None else min(8.0 * e32, cap))
        err = R.rel_l2(got[idx], ref[idx])
        print(f"{label} view {name}: rel L2 {err:.2e}  e32 {e32:.2e}  bound {bound:.1e}")
        if not (np.linalg.norm(ref[idx]) > 0 and err <= bound):
            failed.append((label, name, err, bound))
    return failed


class FdUbo:
    """A duck-typed ubo with float64 view / proj (column-major lists), for finite differences of
    splat_depth_ref.evaluate with the frame held fixed."""

    def __init__(self, V, proj):
        self.view = [float(v) for v in np.asarray(V, np.float64).T.reshape(-1)]
        self.proj = [float(v) for v in proj]


def fd_view_grad(c, step):
    """Central finite differences of sum(image dL) + sum(invdepth dinv) (splat_depth_ref.evaluate, float64, the
    frame held fixed) over the 12 entries of the view's rows 0..2. Returns ([3, 4], the borderline count summed
    over the evaluations).
    A case with a "mask" (splat_hard_grad_ref: both upstream gradients exactly 0 on it) holds borderline decisions by
    construction, all of them under the mask, where a pixel adds exactly nothing to the loss whichever way its
    decisions fall. Outside the mask every decision is at least BORDER (relative) from its threshold at the case's
    own view (tests/test_splat_hard_grad_ref.py::test_mask). For such a case the count is the pixels outside the mask
    with a decision within BORDER / 2 of its threshold at a perturbed view: 0 means that no step moved a decision by
    half the gap it would have to cross to flip."""
    V0 = view_matrix(c["ubo"])
    dL, dinv = c["dL"].astype(np.float64), c["dinv"].astype(np.float64)
    out, border = np.zeros((3, 4)), 0

    def loss(V):
        nonlocal border
        with torch.no_grad():
            e = Z.evaluate(c["g"], FdUbo(V, c["ubo"].proj), c["W"], c["H"], c["bg"], c["frame"], dL, dinv,
                           border=0.5 * R.BORDER if "mask" in c else None)
        border += int((e["border_pixels"] & ~c["mask"]).sum()) if "mask" in c else e["borderline"]
        return float((e["image"] * dL).sum() + (e["invdepth"] * dinv).sum())

    for r in range(3):
        for k in range(4):
            Vp, Vm = V0.copy(), V0.copy()
            Vp[r, k] += step
            Vm[r, k] -= step
            out[r, k] = (loss(Vp) - loss(Vm)) / (2.0 * step)
    return out, border


# ---------------------------------------------------------------------------------------------------------
# se3_view restated (float64 numpy): exp(hat(xi)) @ view0, xi = (translation, rotation)
# ---------------------------------------------------------------------------------------------------------
def se3_exp(xi):
    xi = np.asarray(xi, np.float64)
    A = np.zeros((4, 4))
    w = xi[3:]
    A[:3, :3] = [[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]]
    A[:3, 3] = xi[:3]
    out, term = np.eye(4), np.eye(4)
    for k in range(1, 30):  # (|xi| well below 1: the series is at double precision long before 30 terms)
        term = term @ A / k
        out = out + term
    return out


# ---------------------------------------------------------------------------------------------------------
# pose descent on `posed`: the camera starts at se3(XI0) @ (the true view) and takes STEPS plain gradient steps
# xi <- xi - LR * dL/dxi on L = (|image - image*|^2 + DEPTH_WEIGHT |D - D*|^2) / 2, image* and D* the true pose's
# float64 reference maps, each step on the oracle's frame of the current pose (its float32 view).
# The pose error is pose_error(): how far the pose puts the scene from where the true pose puts it, the RMS over
# the visible Gaussians of |(view - view*) (mean, 1)| in world units. |xi| is not used: it adds radians to lengths,
# and a sideways translation and the rotation that turns the scene back (0.06 against 0.008 rad at depth 7) nearly
# cancel in the image, so plain gradient steps on a photometric loss leave that combination for hundreds of steps
# while the scene is already in place; the run prints |xi| beside the error.
# XI0 is 6 cm-scale in every translation and 0.5 degree-scale in every rotation component; LR is a step per block
# (a radian moves a pixel about depth times as far as a unit of translation, so the curvatures differ by about
# depth^2: gradient over offset is about 1.4e3 and 1.4e5 at XI0), the largest of (4, 8, 12) x (1e-4, 1e-6) with
# which the float64 reference still descends (at 12 it oscillates); STEPS is where that run has reached 0.16 of
# the initial error (0.25 is asked of it; the GPU run gets 0.5).
# ---------------------------------------------------------------------------------------------------------
XI0 = (0.06, -0.04, 0.05, 0.008, -0.006, 0.01)
LR = (8e-4, 8e-6)  # (translation, rotation)
STEPS = 16
DEPTH_WEIGHT = 25.0


def pose_error(c, xi):
    """RMS over the case's visible Gaussians of |(se3(xi) view* - view*) (mean, 1)|."""
    V0 = view_matrix(c["ubo"])
    vis = c["frame"]["radii"] > 0
    mh = np.c_[np.asarray(c["g"]["means"], np.float64), np.ones(len(vis))][vis]
    D = ((se3_exp(xi) @ V0 - V0) @ mh.T)[:3]
    return float(np.sqrt((D ** 2).sum(0).mean()))


def descent_ubo(c, xi):
    """The case's ubo with the view se3(xi) @ (its own view), rounded to float32 as the renderer takes it."""
    u = type(c["ubo"]).from_buffer_copy(c["ubo"])
    V = se3_exp(xi) @ view_matrix(c["ubo"])
    u.view[:] = [float(np.float32(v)) for v in V.T.reshape(-1)]
    return u


def descent_xi_grad(dview, view0, xi):
    """dL/dxi from dL/d view [3, 4] at view = se3(xi) @ view0, through a float64 torch restatement of se3."""
    x = torch.tensor(np.asarray(xi, np.float64), requires_grad=True)
    z = x.new_zeros(())
    hat = torch.stack([torch.stack([z, -x[5], x[4], x[0]]), torch.stack([x[5], z, -x[3], x[1]]),
                       torch.stack([-x[4], x[3], z, x[2]]), torch.stack([z, z, z, z])])
    V = torch.linalg.matrix_exp(hat) @ torch.tensor(np.asarray(view0, np.float64))
    (V[:3] * torch.tensor(np.asarray(dview, np.float64))).sum().backward()
    return x.grad.numpy().copy()


def descent_step(xi, gxi):
    lr = np.array([LR[0]] * 3 + [LR[1]] * 3)
    return np.asarray(xi, np.float64) - lr * np.asarray(gxi, np.float64)


def reference_descent(c, oracle, log=None):
    """The float64 reference's run: returns pose_error before each step and after the last."""
    g, W, H, bg = c["g"], c["W"], c["H"], c["bg"]
    target_img, target_inv = c["r64"]["image"], c["r64"]["invdepth"]
    view0 = view_matrix(c["ubo"])
    xi = np.asarray(XI0, np.float64)
    errs = [pose_error(c, xi)]
    for _ in range(STEPS):
        u = descent_ubo(c, xi)
        frame = oracle.splat_gaussians(g, u, W, H, bg=bg)
        with torch.no_grad():
            e = Z.evaluate(g, u, W, H, bg, frame, np.zeros((H, W, 4)), np.zeros((H, W)))
        dL, dinv = e["image"] - target_img, DEPTH_WEIGHT * (e["invdepth"] - target_inv)
        r = Z.evaluate(g, u, W, H, bg, frame, dL, dinv)
        vis = np.flatnonzero(frame["radii"] > 0)
        dview = view_grad(g, view_matrix(u), u.proj, W, H, vis, r["grads"])
        # (the step's view is the rounded one; xi is the unrounded parameter it was made from)
        xi = descent_step(xi, descent_xi_grad(dview, view0, xi))
        errs.append(pose_error(c, xi))
        if log:
            log(f"step {len(errs) - 1}: loss {0.5 * ((dL ** 2).sum() + (dinv ** 2).sum() / DEPTH_WEIGHT):.4f} "
                f"pose error {errs[-1]:.5f} |xi| {np.linalg.norm(xi):.5f}")
    return errs


# ---------------------------------------------------------------------------------------------------------
# the SH eye: dL/d camera_pos of sh_grad_ref.torch_colors with the camera a leaf
# ---------------------------------------------------------------------------------------------------------
def eye_grad(means, sh, cam, active, dcol, dtype=torch.float64):
    """dL/d cam [3] (numpy float64) of sum(colors dcol), colors = sh_grad_ref.torch_colors, in `dtype`."""
    m = torch.tensor(np.asarray(means, np.float64), dtype=dtype)
    s = torch.tensor(np.asarray(sh, np.float64), dtype=dtype)
    c = torch.tensor(np.asarray(cam, np.float32).astype(np.float64), dtype=dtype, requires_grad=True)
    _, colors = S.torch_colors(m, s, c, active)
    scalar = (colors * torch.tensor(np.asarray(dcol, np.float64), dtype=dtype)).sum()
    if not scalar.requires_grad:  # (degree 0: the colour does not see the camera)
        return np.zeros(3)
    (dc,) = torch.autograd.grad(scalar, [c])
    return dc.double().numpy().copy()


# ---------------------------------------------------------------------------------------------------------
# the first n Gaussians of a case (the reduction's boundaries): a case of its own, with its own oracle frame
# ---------------------------------------------------------------------------------------------------------
_SUBSET_CACHE = {}


def subset_reference(name, n, oracle):
    """The case `name` cut to its first n Gaussians (the whole case when it has no more), with its own frame."""
    base = Z.case_reference(name, oracle)
    n = min(n, len(base["g"]["means"]))
    key = (name, n)
    if key not in _SUBSET_CACHE:
        c = {k: base[k] for k in ("ubo", "W", "H", "bg", "dL", "dinv")}
        c["name"] = f"{name}[:{n}]"
        c["g"] = {k: np.ascontiguousarray(v[:n]) for k, v in base["g"].items()}
        c["frame"] = oracle.splat_gaussians(c["g"], c["ubo"], c["W"], c["H"], bg=c["bg"])
        for k, dt in (("r64", torch.float64), ("r32", torch.float32)):
            c[k] = Z.evaluate(c["g"], c["ubo"], c["W"], c["H"], c["bg"], c["frame"], c["dL"], c["dinv"], dt)
        c["pose"] = _reference(c)
        _SUBSET_CACHE[key] = c
    return _SUBSET_CACHE[key]


# ---------------------------------------------------------------------------------------------------------
# end to end: checkpoint parameters (log-scales, logits, degree-1 SH) seen from view = se3(xi) @ view0, the eye
# the view's own (-R^T t), a loss on the image and on the inverse depth; dL/dxi chained through the eye
# ---------------------------------------------------------------------------------------------------------
E2E_XI = (0.02, -0.015, 0.01, 0.004, -0.003, 0.005)


def e2e_params(c):
    """(means, log_scales, rotations, opacity_logits, sh) float32 from the case's Gaussians (opacities clipped to
    [0.02, 0.98] so that the logits are finite)."""
    g = c["g"]
    rng = np.random.default_rng(92)
    op = np.clip(g["opacities"], 0.02, 0.98)
    return {"means": g["means"], "log_scales": np.log(g["scales"]).astype(np.float32), "rotations": g["rotations"],
            "opacity_logits": np.log(op / (1.0 - op)).astype(np.float32),
            "sh": rng.normal(scale=0.4, size=(len(g["means"]), 4, 3)).astype(np.float32)}


def _e2e_frame(c, oracle, params, view32, dtype):
    V = np.asarray(view32, np.float32)
    eye = (-(V[:3, :3].T @ V[:3, 3])).astype(np.float32)
    scales = np.exp(params["log_scales"]).astype(np.float32)
    opac = (1.0 / (1.0 + np.exp(-params["opacity_logits"].astype(np.float64)))).astype(np.float32)
    m = torch.tensor(params["means"].astype(np.float64), dtype=dtype)
    s = torch.tensor(params["sh"].astype(np.float64), dtype=dtype)
    with torch.no_grad():
        _, cols = S.torch_colors(m, s, torch.tensor(eye.astype(np.float64), dtype=dtype), 1)
    g = {"means": params["means"], "scales": scales, "rotations": params["rotations"], "opacities": opac,
         "colors": cols.double().numpy()}
    u = type(c["ubo"]).from_buffer_copy(c["ubo"])
    u.view[:] = [float(v) for v in V.T.reshape(-1)]
    frame = oracle.splat_gaussians({k: np.ascontiguousarray(v, np.float32) for k, v in g.items()}, u, c["W"], c["H"],
                                   bg=c["bg"])
    return V, eye, g, u, frame


def e2e_upstream(c, oracle, params, view32):
    """(dL_dout, dL_dinv, mask): the case's upstream gradients, exactly 0 on the pixels where the float64
    reference of this frame counts a borderline decision (as splat_grad_ref.frame_case_reference masks a frame)."""
    V, eye, g, u, frame = _e2e_frame(c, oracle, params, view32, torch.float64)
    with torch.no_grad():
        mask = Z.evaluate(g, u, c["W"], c["H"], c["bg"], frame, c["dL"], c["dinv"])["border_pixels"]
    dL, dinv = c["dL"].copy(), c["dinv"].copy()
    dL[mask] = 0.0
    dinv[mask] = 0.0
    return dL, dinv, mask


def e2e_reference(c, oracle, params, view32, view0, xi, dL, dinv, dtype=torch.float64):
    """{"xi": dL/dxi [6], "view": the direct dL/d view [3, 4], "eye": dL/d eye [3], "total": dL/d view with the
    eye's share} of sum(image dL) + sum(invdepth dinv). view32: the float32 view the renderer was given ([4, 4],
    math indexing), taken as exact; the activations and the eye are formed in float32 as the code under test forms
    them (they are its inputs' roundings, 1e-7 relative), everything behind them in `dtype`."""
    W, H, bg = c["W"], c["H"], c["bg"]
    V, eye, g, u, frame = _e2e_frame(c, oracle, params, view32, dtype)
    r = Z.evaluate(g, u, W, H, bg, frame, dL, dinv, dtype)
    vis = np.flatnonzero(frame["radii"] > 0)
    dview = view_grad(g, V.astype(np.float64), u.proj, W, H, vis, r["grads"], dtype)
    deye = eye_grad(params["means"], params["sh"], eye, 1, r["grads"]["colors"], dtype)
    Vt = torch.tensor(V.astype(np.float64), requires_grad=True)
    e = -(Vt[:3, :3].t() @ Vt[:3, 3])
    ((e * torch.tensor(deye)).sum() + (Vt[:3] * torch.tensor(dview)).sum()).backward()
    total = Vt.grad.numpy()[:3].copy()
    return {"xi": descent_xi_grad(total, view0, xi), "view": dview, "eye": deye, "total": total,
            "image": r["image"], "invdepth": r["invdepth"]}


# ---------------------------------------------------------------------------------------------------------
# the second-stage sum (csrc/splat_partial_sum.h, gs_sum_partial_rows<K, BLOCK>) past its first pass: work-item t
# adds the rows t + j BLOCK, j < 4, then steps by 4 BLOCK. One row is 256 Gaussians. Pose finish (BLOCK 256): j = 1
# from row 256 (n > 65 536), the second step from row 1024 (n > 262 144). Eye finish (BLOCK 1024): j = 1 from row
# 1024 (n > 262 144), the second step from row 4096 (n > 1 048 576).
#
# rows_reference(): a cloud of n Gaussians of which only those at `layout` are visible. They are `chunks`
# Gaussians (each touches its own tile only); every other index holds a `chunks` Gaussian with its mean reflected
# through the eye, behind the camera, culled. The reference's cost is that of the visible ones.
# ---------------------------------------------------------------------------------------------------------
ROWS_SOURCE = "chunks"
ROWS_N = 1281 * 256 - 200  # 1281 rows, a partial last workgroup (56 Gaussians)
ROWS_AT = (0, 255, 256, 257, 511, 512, 767, 768, 1023, 1024, 1025, 1279, 1280)
ROWS_LANES = (0, 1, 62, 63, 64, 127, 128, 255)
ROWS = tuple(r * 256 + l for r in ROWS_AT for l in ROWS_LANES if r * 256 + l < ROWS_N)
ROWS_PREFIXES = (65536, 65537, 262144, 262145)  # rows = 256 / 257 and 1024 / 1025
LANES_N = 65536
LANES = tuple(j * 256 + j for j in range(256))  # row j, lane j: every lane of every wave carries a row alone
ROW_SHARE_MIN = 0.01  # every occupied row's own share of |dL/d view|, on each block
LANE_SHARE_FACTOR = 10.0  # every LANES Gaussian's own share over the block's bound max(1e-4, 8 e32)

_ROWS_CACHE = {}


def rows_inputs(layout, n, oracle, pick=None):
    """The cloud described above, without a reference: {"name", "g", "ubo", "W", "H", "bg", "dL", "dinv" (the source
    case's), "pick"}. The Gaussian at layout[k] is the source case's pick[k] (default k)."""
    layout = tuple(int(i) for i in layout)
    pick = tuple(range(len(layout))) if pick is None else tuple(int(i) for i in pick)
    base = Z.case_reference(ROWS_SOURCE, oracle)
    m = len(base["g"]["means"])
    assert len(pick) == len(layout) <= m and len(set(pick)) == len(pick) and max(pick) < m
    assert list(layout) == sorted(set(layout)) and layout[-1] < n
    eye = np.asarray(R.POSE[0], np.float64)
    g = {k: np.ascontiguousarray(v[np.arange(n) % m]) for k, v in base["g"].items()}
    g["means"] = (2.0 * eye[None, :] - g["means"].astype(np.float64)).astype(np.float32)
    for k, v in base["g"].items():
        g[k][np.asarray(layout)] = v[np.asarray(pick)]
    c = {k: base[k] for k in ("ubo", "W", "H", "bg", "dL", "dinv")}
    c.update(name=f"{ROWS_SOURCE} {len(layout)} of {n}", g=g, pick=pick)
    return c


def rows_reference(layout, n, oracle, pick=None):
    """rows_inputs() plus {"frame" (the oracle's), "vis" (= layout), "borderline" (0), "cot" ({key: the float64
    cotangents of the full loss at the visible Gaussians}), "pose"}. Computed once per (layout, n, pick). The
    per-Gaussian reference arrays (20 doubles per Gaussian, part and precision) are not kept."""
    key = (tuple(int(i) for i in layout), int(n), None if pick is None else tuple(int(i) for i in pick))
    if key in _ROWS_CACHE:
        return _ROWS_CACHE[key]
    c = rows_inputs(layout, n, oracle, pick)
    c["frame"] = oracle.splat_gaussians(c["g"], c["ubo"], c["W"], c["H"], bg=c["bg"])
    vis = np.flatnonzero(c["frame"]["radii"] > 0)
    assert np.array_equal(vis, np.asarray(key[0])), (len(vis), len(key[0]))  # the visible set is exactly the layout
    for k, dt in (("r64", torch.float64), ("r32", torch.float32)):
        c[k] = Z.evaluate(c["g"], c["ubo"], c["W"], c["H"], c["bg"], c["frame"], c["dL"], c["dinv"], dt)
        assert c[k]["borderline"] == 0, (k, c[k]["borderline"])
    c["pose"] = _reference(c)
    c["cot"] = {k: c["r64"]["grads"][k][vis].copy() for k in ("means2d", "conics", "invd")}
    c["vis"], c["borderline"] = vis, 0
    del c["r64"], c["r32"]
    _ROWS_CACHE[key] = c
    return c


def rows_prefix(n, oracle):
    """ROWS cut to its first n Gaussians: a case of its own."""
    return rows_reference(tuple(i for i in ROWS if i < n), n, oracle)


def compact_of(c, oracle):
    """The visible Gaussians of a rows_reference() case alone, in order: one partial row (at most 256)."""
    k = len(c["vis"])
    assert k <= 256
    return rows_reference(tuple(range(k)), k, oracle, c["pick"])


def gaussian_shares(c):
    """[len(vis), 3, 4] float64: each visible Gaussian's own dL/d view of the full loss (view_grad restricted to it)."""
    V = view_matrix(c["ubo"])
    g = {k: c["g"][k][c["vis"]] for k in ("means", "scales", "rotations")}
    return np.stack([view_grad(g, V, c["ubo"].proj, c["W"], c["H"], [i], c["cot"]) for i in range(len(c["vis"]))])


def block_shares(c, groups):
    """{block: [len(groups)]}: |sum of the group's Gaussians' shares| / |dL/d view| on each block; groups: lists of
    positions in c["vis"]."""
    s = gaussian_shares(c)
    total = c["pose"]["grads"]["r64"]
    return {name: np.array([np.linalg.norm(s[np.asarray(grp)].sum(0)[idx]) for grp in groups]) /
            np.linalg.norm(total[idx]) for name, idx in BLOCKS.items()}


def lanes_pick(oracle):
    """The 256 Gaussians of the source case with the largest own share of its dL/d view (the smallest of the three
    blocks' shares ranks a Gaussian), in index order."""
    base = case_reference(ROWS_SOURCE, oracle)
    vis = np.flatnonzero(base["frame"]["radii"] > 0)
    assert len(vis) == len(base["g"]["means"])
    c = {"ubo": base["ubo"], "W": base["W"], "H": base["H"], "g": base["g"], "vis": vis, "pose": base["pose"],
         "cot": {k: base["r64"]["grads"][k] for k in ("means2d", "conics", "invd")}}
    sh = block_shares(c, [[i] for i in range(len(vis))])
    worst = np.minimum.reduce([sh[name] for name in BLOCKS])
    return tuple(sorted(np.argsort(-worst, kind="stable")[:256].tolist()))


def lanes_reference(oracle):
    return rows_reference(LANES, LANES_N, oracle, lanes_pick(oracle))


# ---------------------------------------------------------------------------------------------------------
# the eye finish (BLOCK 1024) past its first pass: sh_grad_ref.inputs(deg, n) at sizes whose rows reach the
# j >= 1 loads (row 1024) and the second step (row 4096). A row's class is row // 1024. A random sum grows like
# sqrt(n), so a short class is a small share of dL/d eye: dcol of the Gaussians of the classes below is multiplied by
# the factor beside it, chosen so that every class's own share (eye_grad of that class's Gaussians alone, over the
# whole) is at least EYE_SHARE_MIN (tests/test_splat_pose_grad_ref.py asserts it).
# ---------------------------------------------------------------------------------------------------------
EYE_N_J1 = (262144, 262145)  # rows 1024 and 1025 (the single Gaussian of row 1024 is class 1)
EYE_N_STEP = 4097 * 256 - 100  # 1 048 732: 4097 rows, the last one partial (156 Gaussians), class 4
EYE_SHARE_MIN = 0.05
# (degree, n): {class: factor on its Gaussians' dcol}
# (measured shares without the factors: 0.09% for the one Gaussian of class 1 at 262 145; class 4 at 1 048 732 is
# 0.37% at degree 1 and 2.1% at degree 3. With them: 8.6%, 8.9%, 8.7%.)
EYE_DENSE = {(3, 262144): {}, (3, 262145): {1: 96.0}, (1, EYE_N_STEP): {4: 24.0}, (3, EYE_N_STEP): {4: 4.0}}


def eye_classes(n):
    """[(class, slice of Gaussians)]: rows [1024 k, 1024 k + 1024) of 256 Gaussians each."""
    per = 1024 * 256
    return [(k, slice(k * per, min(n, (k + 1) * per))) for k in range((n + per - 1) // per)]


def eye_dense_inputs(deg, n):
    """(means, sh, dcol) of sh_grad_ref.inputs(deg, n) with EYE_DENSE's factors applied to dcol (float32)."""
    means, sh, dcol = S.inputs(deg, n, False)
    dcol = dcol.copy()
    for k, sl in eye_classes(n):
        dcol[sl] *= np.float32(EYE_DENSE[(deg, n)].get(k, 1.0))
    dcol.setflags(write=False)
    return means, sh, dcol


def eye_sparse_dcol(deg, n):
    """sh_grad_ref.inputs(deg, n)'s dcol kept at index r * 256 + (r % 256) of every row r and zero elsewhere: each
    workgroup holds one Gaussian that counts, each at another lane."""
    dcol = S.inputs(deg, n, False)[2]
    r = np.arange((n + 255) // 256)
    at = r * 256 + (r % 256)
    at = at[at < n]
    out = np.zeros_like(dcol)
    out[at] = dcol[at]
    return out, at
