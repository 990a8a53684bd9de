"""A 3DGS training run on the HIP stages of this library, from a point cloud and captured views to a checkpoint:

    views = load_dataset("dataset", "train")                     # what capture_dataset wrote
    params = init_params(renderer, xyz, rgb, sh_degree=3)        # points3d.ply -> the five leaves
    trainer = Trainer(renderer, params, views, TrainConfig())
    trainer.train(30_000, log_every=1000)
    print(trainer.evaluate(load_dataset("dataset", "test")))     # PSNR / SSIM per view
    trainer.save("point_cloud.ply")                              # load_gaussian_ply reads it back

One iteration is autograd.splat_sh (activate, SH colour, rasterizer), autograd.l1_dssim, their backwards,
DensifyStats.update, GaussianAdam.step (masked by the frame's radii) and what schedule() orders for that
iteration: densify_and_prune, the opacity reset, the active SH degree, the position rate. schedule() restates the
control flow of the reference trainer (Kerbl et al., gaussian-splatting train.py `training()` and
arguments/__init__.py `OptimizationParams`); the differences are listed there. The loop itself launches no
N-sized or pixel-sized torch kernel of its own and never reads the loss back: between two iterations the host only
picks the next view. torch is imported on first use.
"""
from __future__ import annotations

import json
import math
import os
from dataclasses import dataclass

import numpy as np

from . import _abi, autograd
from .capture import save_gaussian_ply
from .densify import PARAM_KEYS, DensifyStats, densify_and_prune
from .optim import SH_DC, GaussianAdam, expon_lr


@dataclass
class TrainConfig:
    """The reference trainer's defaults (arguments/__init__.py OptimizationParams; opacity_lr is its value since the
    sparse-Adam change). Rates are per leaf; the position rate is scaled by the scene extent and decays
    log-linearly from position_lr_init to position_lr_final over position_lr_max_steps (optim.expon_lr)."""
    iterations: int = 30_000
    position_lr_init: float = 1.6e-4
    position_lr_final: float = 1.6e-6
    position_lr_max_steps: int = 30_000
    sh_lr: float = 0.0025 / 20.0        # f_rest: feature_lr / 20
    sh_dc_lr: float = 0.0025            # f_dc: feature_lr
    opacity_lr: float = 0.025
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    lambda_dssim: float = 0.2
    densify_from: int = 500
    densify_until: int = 15_000
    densify_interval: int = 100
    densify_grad_threshold: float = 0.0002
    opacity_reset_interval: int = 3000
    sh_degree_interval: int = 1000
    min_opacity: float = 0.005
    percent_dense: float = 0.01
    bg: tuple = (0.0, 0.0, 0.0)
    seed: int = 0


@dataclass
class Schedule:
    """What iteration `it` does besides the render, the loss, the backward and the Adam step."""
    sh_degree: int            # the bands splat_sh evaluates
    lr_means: float           # the position rate of this step
    gather_stats: bool        # DensifyStats.update after the backward
    densify: dict | None      # densify_and_prune's keyword arguments when it runs after this step
    reset_opacity: bool       # GaussianAdam.reset_opacity after this step (after a densification of the same step)


def schedule(it: int, cfg: TrainConfig, extent: float, max_degree: int) -> Schedule:
    """The events of iteration `it` (1-based), a pure host function; the Trainer does exactly this.

    Restated from the reference's train.py `training()`:
      gaussians.update_learning_rate(iteration)                       -> lr_means = expon_lr(it, ...) x extent
      if iteration % 1000 == 0: gaussians.oneupSHdegree()              -> sh_degree (see below)
      if iteration < opt.densify_until_iter: add_densification_stats   -> gather_stats
        if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
          size_threshold = 20 if iteration > opt.opacity_reset_interval else None
          gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, scene.cameras_extent, size_threshold)
        if iteration % opt.opacity_reset_interval == 0: gaussians.reset_opacity()
    and from gaussian_model.py: the split threshold percent_dense x extent (densify_and_clone / _split) and, with a
    size threshold, the prune of world scales above 0.1 x extent (densify_and_prune).
    Differences from the reference, on purpose:
      - sh_degree = min((it - 1) // sh_degree_interval, max_degree): the degree rises with iteration 1001, 2001, ...;
        the reference raises it before the render of iteration 1000, one iteration earlier.
      - the last densification runs after iteration densify_until itself, on the statistic gathered up to the
        iteration before (gathering stops at it < densify_until as in the reference, whose strict gate drops that
        last densification).
      - the optimizer steps before the densification of its iteration, not after it.
    The opacity reset is gated like the reference's (it < densify_until): an ungated reset would clear the opacities
    of iteration 30 000, the checkpoint that is saved."""
    it = int(it)
    if it < 1:
        raise _abi.PtgsError("iterations count from 1")
    degree = min((it - 1) // int(cfg.sh_degree_interval), int(max_degree))
    lr = expon_lr(it, cfg.position_lr_init * extent, cfg.position_lr_final * extent, cfg.position_lr_max_steps)
    densify = None
    if cfg.densify_from < it <= cfg.densify_until and it % cfg.densify_interval == 0:
        late = it > cfg.opacity_reset_interval
        densify = {"grad_threshold": cfg.densify_grad_threshold, "scale_split": cfg.percent_dense * extent,
                   "min_opacity": cfg.min_opacity, "max_scale": 0.1 * extent if late else 0.0,
                   "max_screen_radius": 20.0 if late else 0.0}
    reset = it < cfg.densify_until and it % cfg.opacity_reset_interval == 0
    return Schedule(degree, lr, it < cfg.densify_until, densify, reset)


@dataclass
class View:
    """One training or evaluation view: the camera as a ptgs_ubo (view, proj, camera_pos), the image size, the eye the
    SH colours are seen from and the target, a float32 device tensor [H, W, 3] (None for a camera without an image)."""
    ubo: _abi.Ubo
    W: int
    H: int
    camera_pos: tuple
    target: object = None
    name: str = ""


def view_from_c2w(c2w, fov_y_rad: float, W: int, H: int, target=None, name: str = "", near: float = 0.1,
                  far: float = 10000.0) -> View:
    """A View from a camera-to-world matrix (4 x 4, math indexing: what transforms_*.json stores, the inverse of the
    view). The view is its float64 inverse rounded to float32; the projection is ptgs_camera_perspective's."""
    m = np.asarray(c2w, np.float64).reshape(4, 4)
    view = np.linalg.inv(m)
    u = _abi.Ubo()
    u.view[:] = [float(np.float32(v)) for v in view.T.reshape(-1)]  # column-major
    proj = np.zeros(16, np.float32)
    _abi.check(_abi.load_library().ptgs_camera_perspective(np.float32(fov_y_rad), W / H, near, far, _abi.fptr(proj)),
               "ptgs_camera_perspective")
    u.proj[:] = [float(x) for x in proj]
    eye = tuple(float(np.float32(v)) for v in m[:3, 3])
    u.camera_pos[:] = eye
    u.fov, u.height = float(np.float32(fov_y_rad)), float(H)
    return View(u, int(W), int(H), eye, target, name)


def load_dataset(root: str, split: str = "train", images: bool = True, size=None, device="cuda") -> list:
    """The views of transforms_<split>.json as ptgs_write_transforms_json writes it (capture_dataset): per frame the
    rows of inverse(view) (scene.transform_matrix_rows) and the file path of its JPEG, with camera_angle_x =
    2 atan(tan(fov_y / 2) aspect). Each image is decoded with scene.decode_image and uploaded as float32
    [H, W, 3] = u8 / 255. images=False reads the cameras alone; size=(W, H) is then required (with images it is
    checked against the files)."""
    from .scene import decode_image
    with open(os.path.join(root, f"transforms_{split}.json")) as f:
        meta = json.load(f)
    fov_x = float(meta["camera_angle_x"])
    views = []
    for fr in meta["frames"]:
        target = None
        if images:
            import torch
            path = os.path.join(root, fr["file_path"] + ".jpg")
            with open(path, "rb") as f:
                px = decode_image(f.read())
            if size is not None and (px.shape[1], px.shape[0]) != tuple(size):
                raise _abi.PtgsError(f"{path} is {px.shape[1]} x {px.shape[0]}, not {size[0]} x {size[1]}")
            W, H = int(px.shape[1]), int(px.shape[0])
            target = (torch.from_numpy(np.ascontiguousarray(px[..., :3])).to(device).to(torch.float32) / 255.0)
        elif size is None:
            raise _abi.PtgsError("load_dataset(images=False) needs size=(W, H)")
        else:
            W, H = int(size[0]), int(size[1])
        fov_y = 2.0 * math.atan(math.tan(0.5 * fov_x) * H / W)
        views.append(view_from_c2w(fr["transform_matrix"], fov_y, W, H, target, fr["file_path"]))
    return views


def scene_extent(views) -> float:
    """The reference's getNerfppNorm radius (scene/dataset_readers.py): 1.1 x the largest distance of a camera from
    the cameras' centroid."""
    c = np.asarray([v.camera_pos for v in views], np.float64).reshape(-1, 3)
    if len(c) == 0:
        raise _abi.PtgsError("no views")
    return float(1.1 * np.max(np.linalg.norm(c - c.mean(0, keepdims=True), axis=1)))


def init_params(renderer, xyz, rgb=None, sh_degree: int = 3) -> dict:
    """The five leaves of a checkpoint from a point cloud (create_from_pcd): gaussians_from_points (kNN scales,
    identity rotations, opacity 0.1, colours rgb / 255) and then checkpoint_init in place (log, logit, RGB2SH
    into zeroed SH rows). xyz: float32 device tensor [N, 3]; rgb: uint8 device tensor [N, 3] or None (black)."""
    g = renderer.gaussians_from_points(xyz, rgb)
    ls, lo, sh = renderer.checkpoint_init(g["scales"], g["opacities"], g["colors"], sh_degree)
    p = {"means": g["means"], "log_scales": ls, "rotations": g["rotations"], "opacity_logits": lo, "sh": sh}
    return {k: p[k].requires_grad_(True) for k in PARAM_KEYS}


class Trainer:
    """The training loop. params: the dict of the five leaves (float32 device tensors, e.g. init_params' or a loaded
    checkpoint's); views: View objects with targets, all used for training; extent defaults to
    scene_extent(views). .params holds the current leaves (new tensors after a densification), .iteration the
    iterations done, .optimizer / .stats the GaussianAdam and DensifyStats, .last_counts the latest
    densification's ptgs_densify_counts."""

    def __init__(self, renderer, params: dict, views, cfg: TrainConfig | None = None, extent: float | None = None):
        import torch
        self.renderer = renderer
        self.cfg = cfg if cfg is not None else TrainConfig()
        self.views = list(views)
        if not self.views or any(v.target is None for v in self.views):
            raise _abi.PtgsError("the trainer needs at least one view, each with a target")
        self.extent = float(scene_extent(self.views) if extent is None else extent)
        self.params = {k: params[k] if params[k].requires_grad else params[k].requires_grad_(True)
                       for k in PARAM_KEYS}
        self.max_degree = renderer._sh_degree(self.params["sh"])
        c = self.cfg
        self.optimizer = GaussianAdam(self.params, {
            "means": c.position_lr_init * self.extent, "log_scales": c.scaling_lr, "rotations": c.rotation_lr,
            "opacity_logits": c.opacity_lr, "sh": c.sh_lr, SH_DC: c.sh_dc_lr})
        dev = self.params["means"].device
        self.stats = DensifyStats(self.count, dev)
        self.iteration = 0
        self.last_counts = None
        self._order = np.random.default_rng(c.seed)  # the views' order, on the host
        self._queue = []
        self._noise = torch.Generator(device=dev)    # the split children's draws
        self._noise.manual_seed(int(c.seed))
        self._m2d = torch.empty((self.count, 2), dtype=torch.float32, device=dev)  # every backward overwrites it

    @property
    def count(self) -> int:
        return int(self.params["means"].shape[0])

    def _next_view(self) -> View:
        if not self._queue:  # a new epoch: every view once, in a fresh order
            self._queue = [int(k) for k in self._order.permutation(len(self.views))]
        return self.views[self._queue.pop(0)]

    def step(self):
        """One iteration on the next view; returns the loss as a 0-dim device tensor (not read back)."""
        import torch
        it = self.iteration + 1
        s = schedule(it, self.cfg, self.extent, self.max_degree)
        v, r, opt, p = self._next_view(), self.renderer, self.optimizer, self.params
        opt.zero_grad()
        opt.set_lr("means", s.lr_means)
        m2d = self._m2d if s.gather_stats else None
        img = autograd.splat_sh(r, p["means"], p["log_scales"], p["rotations"], p["opacity_logits"], p["sh"], v.ubo,
                                v.W, v.H, bg=self.cfg.bg, active_degree=s.sh_degree, camera_pos=v.camera_pos,
                                means2d_grad=m2d)
        loss = autograd.l1_dssim(r, img, v.target, lam=self.cfg.lambda_dssim)
        loss.backward()
        # the statistic and the mask read the radii of the frame just published: no splat call before them
        if s.gather_stats:
            self.stats.update(r, m2d, v.W, v.H)
        opt.step(r, masked=True)
        self.iteration = it
        if s.densify is not None:
            self.params, self.last_counts, self.stats = densify_and_prune(r, p, self.stats, optimizer=opt,
                                                                          generator=self._noise, **s.densify)
            self._m2d = torch.empty((self.count, 2), dtype=torch.float32, device=self._m2d.device)
        if s.reset_opacity:
            opt.reset_opacity(r)
        return loss.detach()

    def train(self, n: int, log_every: int = 0):
        """n iterations; log_every > 0 prints the loss every that many (the only read-back of the loop). Returns the
        last loss (a device scalar)."""
        loss = None
        for _ in range(int(n)):
            loss = self.step()
            if log_every and self.iteration % log_every == 0:
                print(f"iteration {self.iteration}: loss {float(loss):.6f}  gaussians {self.count}")
        return loss

    def active_degree(self) -> int:
        """The SH bands of the latest iteration (of the first before any)."""
        return schedule(max(self.iteration, 1), self.cfg, self.extent, self.max_degree).sh_degree

    def render(self, view: View, out=None):
        """The current Gaussians seen from `view`, RGBA32F [H, W, 4]: activate_gaussians and splat_gaussians_sh with
        the active degree. It replaces the published frame (call it between steps)."""
        import torch
        p = {k: t.detach() for k, t in self.params.items()}
        scales, opacities = self.renderer.activate_gaussians(p["log_scales"], p["opacity_logits"])
        g = {"means": p["means"], "scales": scales, "rotations": p["rotations"], "opacities": opacities, "sh": p["sh"]}
        if out is None:
            out = torch.empty((view.H, view.W, 4), dtype=torch.float32, device=p["means"].device)
        self.renderer.splat_gaussians_sh(g, view.ubo, view.W, view.H, out, active_degree=self.active_degree(),
                                         bg=self.cfg.bg)
        return out

    def evaluate(self, views=None) -> list:
        """Per view {"name", "mse", "psnr", "ssim"}: the squared error from image_mse (PSNR = -10 log10(mse), inf on
        equal images), SSIM from the loss's own terms. Reads two scalars back per view."""
        out = []
        for v in (self.views if views is None else views):
            img = self.render(v)
            total = self.renderer.image_mse(img, v.target)
            terms, _ = self.renderer.l1_dssim_loss(img, v.target, lam=self.cfg.lambda_dssim)
            mse = float(total.cpu()[0]) / (3.0 * v.W * v.H)
            out.append({"name": v.name, "mse": mse, "psnr": -10.0 * math.log10(mse) if mse > 0.0 else math.inf,
                        "ssim": float(terms.cpu()[2])})
        return out

    def save(self, path: str):
        """The current leaves as a checkpoint PLY (capture.save_gaussian_ply; load_gaussian_ply reads it back)."""
        save_gaussian_ply(path, self.params)
