"""References of the training additions (pathtracer_gaussiansplatting_amd/train.py, csrc/splat_train.hip),
independent of the code under test, and the cases of tests/test_train_ref.py (CPU) and tests/test_train_gpu.py.

  np_log2x / checkpoint_init   the contract of ptgs_gaussians_checkpoint_init in numpy float32: every operand is a
                               float32 array or scalar, the expressions are those of include/ptgs/ptgs.h and of
                               detmath.h's log2x, left to right.
  image_sq_err                 ptgs_image_mse's sum in float64 (d = a - b and d * d in float32, then widened).
  RefTrainer                   a training run composed of the existing references, none of them edited: the oracle's
                               frame and splat_grad_ref.evaluate (float64) for the rasterizer and its backward,
                               sh_grad_ref for the SH colour, loss_ref.loss_and_grad for the loss, the activations'
                               chain rule written out, and adam_ref's masked Adam (the float32 contract) for the step.
  the scene                    make_scene(): 64 x 48 (4 x 3 tiles), 40 Gaussians, 6 training views and a held-out one.
"""
import numpy as np
import torch

import adam_ref as A
import loss_ref as L
import sh_grad_ref as S
import splat_grad_ref as R

from pathtracer_gaussiansplatting_amd import TrainConfig

F = np.float32
LN2 = F(0.69314718055994531)
C0 = F(0.28209479177387814)
KEYS = ("means", "log_scales", "rotations", "opacity_logits", "sh")
SIZES = (1, 255, 256, 257, 1000)


# ---------------------------------------------------------------------------------------------------------
# ptgs_gaussians_checkpoint_init
# ---------------------------------------------------------------------------------------------------------
def np_log2x(x):
    """detmath.h log2x on a float32 array: -1e30 where x is not positive, the subnormal rescale, the mantissa moved
    to [sqrt(1/2), sqrt(2)), the atanh series by Horner, every operation in float32."""
    x = np.ascontiguousarray(x, F)
    bad = ~(x > 0)
    xs = np.where(bad, F(1), x)
    u = xs.view(np.uint32)
    e = ((u >> 23) & 0xFF).astype(np.int32) - 127
    sub = e == -127
    with np.errstate(all="ignore"):
        scaled = np.ascontiguousarray(xs * F(8388608.0), F)
    u2 = scaled.view(np.uint32)
    e = np.where(sub, ((u2 >> 23) & 0xFF).astype(np.int32) - 127 - 23, e)
    u = np.where(sub, u2, u)
    m = ((u & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).astype(np.uint32).view(F)
    big = m > F(1.41421356)
    m = np.where(big, m * F(0.5), m)
    e = np.where(big, e + 1, e)
    s = (m - F(1)) / (m + F(1))
    s2 = s * s
    p = np.full_like(s, F(0.2222222222))
    for c in (0.2857142857, 0.4, 0.6666666667, 2.0):
        p = p * s2 + F(c)
    ln = s * p
    out = e.astype(F) + ln * F(1.44269504088896341)
    assert out.dtype == F
    return np.where(bad, F(-1.0e30), out)


def checkpoint_init(scales, opacities, colors, sh_degree):
    """(log_scales [N, 3], opacity_logits [N], sh [N, (d+1)^2, 3]) float32, as the contract writes them."""
    scales, o, colors = np.asarray(scales, F), np.asarray(opacities, F), np.asarray(colors, F)
    with np.errstate(all="ignore"):
        ls = np_log2x(scales.reshape(-1)).reshape(scales.shape) * LN2
        lo = (np_log2x(o) - np_log2x(F(1) - o)) * LN2
        sh = np.zeros((len(o), (sh_degree + 1) ** 2, 3), F)
        sh[:, 0, :] = (colors - F(0.5)) / C0
    assert ls.dtype == F and lo.dtype == F and sh.dtype == F
    return ls, lo, sh


def init_case(n, seed=0):
    """(scales [n, 3], opacities [n], colors [n, 3]) float32: scales log-uniform over 1e-5 .. 30, opacities over
    (0, 1) with both ends approached, colours over [0, 1]; then the values where log2x changes path: 1, the mantissa
    threshold and its neighbours, a subnormal, the initialisation's own 0.1 and sqrt(1e-7), opacity 0.5 and its
    neighbours (1 - o == o)."""
    rng = np.random.default_rng([seed, n])
    scales = np.exp(rng.uniform(np.log(1e-5), np.log(30.0), (n, 3))).astype(F)
    o = rng.uniform(0.0, 1.0, n)
    o = np.where(rng.random(n) < 0.2, 10.0 ** rng.uniform(-7, -1, n), o)
    o = np.where(rng.random(n) < 0.2, 1.0 - 10.0 ** rng.uniform(-7, -1, n), o).astype(F)
    o = np.clip(o, F(1e-7), np.nextafter(F(1), F(0)))
    colors = rng.uniform(0.0, 1.0, (n, 3)).astype(F)
    t = F(1.41421356)
    special = [F(1), t, np.nextafter(t, F(2)), np.nextafter(t, F(1)), F(1e-40), F(0.1), np.sqrt(F(1e-7)), F(2), F(0.5)]
    flat = scales.reshape(-1)
    for k, v in enumerate(special[:flat.size]):
        flat[(k * 31) % flat.size if flat.size > 9 * 31 else k] = v
    for k, v in enumerate([F(0.1), F(0.5), np.nextafter(F(0.5), F(1)), np.nextafter(F(0.5), F(0))][:n]):
        o[(k * 53) % n if n > 4 * 53 else k] = v
    if n > 2:
        colors[0], colors[1] = (0.0, 0.5, 1.0), (128 / 255, 128 / 255, 128 / 255)
    return scales, o, colors


def pack_init(scales, opacities, colors, sh_degree, in_place):
    """The case file of tests/native/train_host.cpp init."""
    return (np.asarray([len(opacities), sh_degree, int(in_place)], np.uint32).tobytes() + scales.tobytes() +
            opacities.tobytes() + colors.tobytes())


def unpack_init(blob, n, sh_degree):
    row = 3 * (sh_degree + 1) ** 2
    a = np.frombuffer(blob, F)
    assert a.size == 4 * n + n * row
    return a[:3 * n].reshape(n, 3), a[3 * n:4 * n], a[4 * n:].reshape(n, row // 3, 3)


# ---------------------------------------------------------------------------------------------------------
# ptgs_image_mse
# ---------------------------------------------------------------------------------------------------------
MSE_SIZES = ((1, 1), (17, 9), (64, 48), (333, 129))  # (W, H)


def image_sq_err(image, target):
    """sum over rgb of (double)(d * d), d = a - b in float32; the sum in float64 (pairwise: exact to ~1e-16)."""
    d = np.asarray(image, F)[..., :3] - np.asarray(target, F)[..., :3]
    sq = d * d
    assert sq.dtype == F
    return float(sq.astype(np.float64).sum())


def mse_case(W, H, channels):
    image, target = L.make_inputs(H, W, channels, seed=5)
    return image, target


# ---------------------------------------------------------------------------------------------------------
# the scene of the training runs
# ---------------------------------------------------------------------------------------------------------
W, H = 64, 48
N_TRUE = 40
BG = (0.0, 0.0, 0.0)
# The seed and the step count are fixed on the reference run by the pose descent's rule (splat_pose_grad_ref.py):
# the float64 reference must have reached 0.16 of its initial held-out MSE, is asked 0.25, and the GPU is asked 0.5.
# Seed 0, the first tried, ends 120 steps at 0.123 (0.486, 0.334, 0.242, 0.169, 0.145, 0.123 every 20 steps); seeds
# 1 to 6 end at 0.090, 0.137, 0.171, 0.093, 0.207 and 0.131.
SCENE_SEED = 0
STEPS = 120
RATE_SCALE = 10.0     # the runs' rates: 10 x the trainer's defaults, with extent 1
REF_ASKED, GPU_ASKED, REF_MUST_REACH = 0.25, 0.5, 0.16
# the reference run's held-out MSE every 20 steps, recorded (test_train_ref.test_reference_run recomputes it and
# compares): what the GPU run prints beside its own without spending the reference's 9 s again
REF_TRAJECTORY = ((0, 4.911e-03), (20, 2.388e-03), (40, 1.641e-03), (60, 1.189e-03), (80, 8.315e-04), (100, 7.137e-04),
                  (120, 6.048e-04))
# the largest absolute error of the restated logarithms against float64 on init_case(1000, 9), with headroom: measured
# 1.04e-6 (log-scales) and 1.36e-6 (logits), numpy's float32 log 5.3e-7 and 9.0e-7 (test_checkpoint_init_against_float64)
LOG_ABS_ERR = 2e-6


def run_config(**kw):
    """The trainer's defaults with every rate x RATE_SCALE and no densification, reset or degree step in reach."""
    c = TrainConfig()
    for k in ("position_lr_init", "position_lr_final", "sh_lr", "sh_dc_lr", "opacity_lr", "scaling_lr", "rotation_lr"):
        setattr(c, k, getattr(c, k) * RATE_SCALE)
    c.bg, c.seed = BG, SCENE_SEED
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def small_config():
    """The events run: densify from 20 every 20 until 80, reset every 50, a degree every 30."""
    return run_config(densify_from=20, densify_interval=20, densify_until=80, opacity_reset_interval=50,
                      sh_degree_interval=30)


def _orbit(k, n, radius, height):
    a = 2.0 * np.pi * (k + 0.25) / n
    return (radius * np.cos(a), height, radius * np.sin(a))


def make_scene(seed=SCENE_SEED):
    """{"truth": the 40 true Gaussians (float32, splat_gaussians layout), "eyes": 6 training eyes on an orbit of
    radius 6 at heights 1.5 and -1 looking at the origin, "held_out": the 7th eye, between two of them at height
    0.4, "xyz": the start's points (true means + N(0, 0.03)), "rgb": grey 128}."""
    rng = np.random.default_rng(seed)
    box = np.array([1.3, 1.0, 1.0])
    truth = {"means": rng.uniform(-1.0, 1.0, (N_TRUE, 3)) * box,
             "scales": rng.uniform(0.12, 0.35, (N_TRUE, 3)),
             "rotations": rng.normal(size=(N_TRUE, 4)),
             "opacities": rng.uniform(0.5, 0.95, N_TRUE),
             "colors": rng.uniform(0.0, 1.0, (N_TRUE, 3))}
    truth = {k: np.ascontiguousarray(v, F) for k, v in truth.items()}
    eyes = [_orbit(k, 6, 6.0, 1.5 if k % 2 == 0 else -1.0) for k in range(6)]
    held = _orbit(0.5, 6, 6.0, 0.4)
    xyz = (truth["means"].astype(np.float64) + rng.normal(0.0, 0.03, (N_TRUE, 3))).astype(F)
    return {"truth": truth, "eyes": eyes, "held_out": held, "xyz": xyz, "rgb": np.full((N_TRUE, 3), 128, np.uint8)}


def eye_ubo(eye):
    u = R.make_ubo(W, H, eye, (0.0, 0.0, 0.0))
    u.camera_pos[:] = [float(F(v)) for v in eye]
    return u


def render64(g, ubo, oracle):
    """The float64 reference image [H, W, 4] of activated Gaussians g (float64 or float32 arrays) on the oracle's
    frame of their float32 values, and that frame."""
    g32 = {k: np.ascontiguousarray(v, F) for k, v in g.items()}
    frame = oracle.splat_gaussians(g32, ubo, W, H, bg=BG)
    with torch.no_grad():
        img = R.evaluate(g, ubo, W, H, BG, frame, np.zeros((H, W, 4)))["image"]
    return img, frame


def start_leaves(scene, oracle, sh_degree=0):
    """init_params' form on the host: the oracle's gaussians_from_points, then checkpoint_init."""
    g = oracle.gaussians_from_points(scene["xyz"], scene["rgb"])
    ls, lo, sh = checkpoint_init(g["scales"], g["opacities"], g["colors"], sh_degree)
    return {"means": g["means"], "log_scales": ls, "rotations": g["rotations"], "opacity_logits": lo, "sh": sh}


def held_out_mse(img, target):
    return float(np.mean((np.asarray(img, np.float64)[..., :3] - np.asarray(target, np.float64)[..., :3]) ** 2))


class RefTrainer:
    """The reference run: float64 forward and backward per step, the float32 Adam contract between steps (the leaves
    are float32 arrays, as the trainer's are). The views come in the Trainer's order: a permutation per epoch from
    numpy's default_rng(cfg.seed)."""

    def __init__(self, scene, oracle, cfg, sh_degree=0):
        self.oracle, self.cfg, self.scene = oracle, cfg, scene
        self.ubos = [eye_ubo(e) for e in scene["eyes"]]
        self.held_ubo = eye_ubo(scene["held_out"])
        self.targets = [render64(scene["truth"], u, oracle)[0] for u in self.ubos]
        self.held_target = render64(scene["truth"], self.held_ubo, oracle)[0]
        self.p = start_leaves(scene, oracle, sh_degree)
        self.m = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.v = {k: np.zeros_like(v) for k, v in self.p.items()}
        self.iteration = 0
        self._order, self._queue = np.random.default_rng(cfg.seed), []
        self.max_degree = sh_degree

    def activated(self, active):
        """The Gaussians the rasterizer sees, in float64: exp, sigmoid, the SH colour (sh_grad_ref)."""
        p = {k: v.astype(np.float64) for k, v in self.p.items()}
        return p, {"means": p["means"], "scales": np.exp(p["log_scales"]), "rotations": p["rotations"],
                   "opacities": 1.0 / (1.0 + np.exp(-p["opacity_logits"]))}

    def _colors(self, p, eye, active, dcol):
        return S.evaluate(p["means"], p["sh"], eye, active, dcol)

    def render(self, ubo, eye, active=None):
        active = self.max_degree if active is None else active
        p, g = self.activated(active)
        g["colors"] = self._colors(p, eye, active, np.zeros((len(p["means"]), 3)))["colors"]
        return render64(g, ubo, self.oracle)[0]

    def held_out(self):
        return held_out_mse(self.render(self.held_ubo, self.scene["held_out"]), self.held_target)

    def gradients(self, k, active):
        """(loss, {leaf: dL/d leaf float64}, radii) of view k at the current leaves."""
        ubo, eye = self.ubos[k], self.scene["eyes"][k]
        p, g = self.activated(active)
        zero = np.zeros((len(p["means"]), 3))
        g["colors"] = self._colors(p, eye, active, zero)["colors"]
        img, frame = render64(g, ubo, self.oracle)
        loss, _, _, dimg = L.loss_and_grad(img, self.targets[k], lam=self.cfg.lambda_dssim)
        gr = R.evaluate(g, ubo, W, H, BG, frame, dimg)["grads"]
        c = self._colors(p, eye, active, gr["colors"])
        o = g["opacities"]
        grads = {"means": gr["means"] + c["dmeans"], "log_scales": gr["scales"] * g["scales"],
                 "rotations": gr["rotations"], "opacity_logits": gr["opacities"] * o * (1.0 - o), "sh": c["dsh"]}
        return loss, grads, frame["radii"]

    def next_view(self):
        if not self._queue:
            self._queue = [int(k) for k in self._order.permutation(len(self.ubos))]
        return self._queue.pop(0)

    def step(self):
        from pathtracer_gaussiansplatting_amd.train import schedule
        it = self.iteration + 1
        s = schedule(it, self.cfg, 1.0, self.max_degree)
        assert s.densify is None and not s.reset_opacity  # (the reference has neither)
        k = self.next_view()
        loss, grads, radii = self.gradients(k, s.sh_degree)
        c = self.cfg
        lr = {"means": (s.lr_means, 0, 0.0), "log_scales": (c.scaling_lr, 0, 0.0), "rotations": (c.rotation_lr, 0, 0.0),
              "opacity_logits": (c.opacity_lr, 0, 0.0), "sh": (c.sh_lr, 3, c.sh_dc_lr)}
        rows = [A.row(self.p[key], grads[key].astype(F), self.m[key], self.v[key], *lr[key]) for key in KEYS]
        out = A.adam_step(rows, step=it, radii=radii)
        for key, r in zip(KEYS, out):
            shape = self.p[key].shape
            self.p[key], self.m[key], self.v[key] = (r[x].reshape(shape) for x in ("param", "exp_avg", "exp_avg_sq"))
        self.iteration = it
        return loss, k, grads, radii


_RUN = {}


def reference_run(oracle, steps=STEPS, every=20):
    """The reference's convergence run, once per session: {"trajectory": [(iteration, held-out MSE)], "first": the
    first step's (view, gradients, radii, leaves before, leaves after), "scene", "targets", "held_target"}."""
    if "run" not in _RUN:
        scene = make_scene()
        t = RefTrainer(scene, oracle, run_config())
        traj = [(0, t.held_out())]
        first = None
        for _ in range(steps):
            before = {k: v.copy() for k, v in t.p.items()} if first is None else None
            loss, k, grads, radii = t.step()
            if first is None:
                first = {"view": k, "grads": grads, "radii": radii, "before": before,
                         "after": {k2: v.copy() for k2, v in t.p.items()}, "loss": loss}
            if t.iteration % every == 0:
                traj.append((t.iteration, t.held_out()))
        _RUN["run"] = {"trajectory": traj, "first": first, "scene": scene, "targets": t.targets,
                       "held_target": t.held_target, "trainer": t}
    return _RUN["run"]


def first_step_scene(oracle):
    """What the GPU's first-step test needs without the whole run: the scene, the targets and the first step."""
    if "first" not in _RUN:
        if "run" in _RUN:
            r = _RUN["run"]
            _RUN["first"] = {k: r[k] for k in ("first", "scene", "targets", "held_target")}
        else:
            scene = make_scene()
            t = RefTrainer(scene, oracle, run_config())
            before = {k: v.copy() for k, v in t.p.items()}
            loss, k, grads, radii = t.step()
            _RUN["first"] = {"first": {"view": k, "grads": grads, "radii": radii, "before": before,
                                       "after": {k2: v.copy() for k2, v in t.p.items()}, "loss": loss},
                             "scene": scene, "targets": t.targets, "held_target": t.held_target}
    return _RUN["first"]


# The first-step check: an element takes part where |g_ref| >= SIGN_FLOOR max|g_ref| of its leaf. A leaf whose
# reference gradient vanishes analytically takes no part at all: at the start the scales are isotropic, so the
# covariance does not depend on the rotation and every dL/d rotation is rounding noise (1e-17 against 1e-3 for the
# other leaves); a leaf counts as such when its largest |g_ref| is below LEAF_FLOOR x the largest of all leaves.
SIGN_FLOOR, LEAF_FLOOR, SIGN_MAX_LEFT_OUT = 1e-3, 1e-9, 0.20


def sign_tolerance(p0, rate):
    """How far (p1 - p0) / rate may lie from -sign(g) after Adam's first step from zero moments. The step is
    rate x (m' / d) / bc1 with m' / d = ob1 g / (sqrt(ob2 g g) / bc2s + eps): +-1 up to a few float32 roundings
    (eps = 1e-15 is far below every |g| that takes part), 1e-6 in all; storing p - step rounds at the size of p:
    an ulp of the largest |p0| over the rate."""
    return 1e-6 + float(np.spacing(F(np.abs(p0).max()))) / rate


def sign_mask(grads, radii):
    """{leaf: bool mask of the elements whose sign is checked}, the leaves left out as vanishing, and the share of
    the seen elements (of the leaves that take part) that the threshold leaves out."""
    seen = np.asarray(radii) > 0
    top = max(float(np.abs(g).max()) for g in grads.values())
    masks, vanishing, total, kept = {}, [], 0, 0
    for k, g in grads.items():
        a = np.abs(g)
        rows = np.zeros(g.shape, bool)
        rows[seen] = True
        if float(a.max()) < LEAF_FLOOR * top:
            vanishing.append(k)
            masks[k] = np.zeros(g.shape, bool)
            continue
        masks[k] = rows & (a >= SIGN_FLOOR * float(a[rows].max()))
        total += int(rows.sum())
        kept += int(masks[k].sum())
    return masks, vanishing, 1.0 - kept / max(total, 1)
