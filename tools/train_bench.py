"""Time the training loop (pathtracer_gaussiansplatting_amd.train.Trainer) and the share of it that is glue.

    python tools/train_bench.py [--n 100000] [--width 1920] [--height 1080] [--views 8] [--steps 60] [--warmup 10]
                                [--rounds 3] [--out profiles/train_bench.json]

Workload: n Gaussians of degree 3 (synthetic.gaussians_c2, the flagship splat workload's distribution) seen from
`views` eyes on a small circle around the origin, all looking down -Z. The targets are the renderer's own frames of
those Gaussians; the run starts from the same Gaussians with the DC colours pulled half way to grey and the higher SH
bands at zero, as a checkpoint (Renderer.checkpoint_init), so every stage has work to do and the loss is not zero.
The window is iterations warmup + 1 .. warmup + steps of a run with the trainer's default config and the Gaussians' own
extent: before iteration 500, so it holds no densification, reset or degree step (those are timed by
tools/densify_bench.py and tools/adam_bench.py); every iteration gathers the densify statistic, as the first 15 000 of
a real run do.

Figures, per round (the median and the range over the rounds are reported):
  ms_per_iter    host clock around `steps` x Trainer.step() and a final device synchronise, over steps
  in_library_ms  host time spent inside libptgs's C calls (every renderer.lib.ptgs_* call is wrapped by a timer)
  sync_ms        the final synchronise: how far the host ran ahead of the device
  glue_ms        ms_per_iter - in_library_ms - sync_ms: Python, torch.autograd's bookkeeping, the output tensors' allocation
  glue_share     glue_ms / ms_per_iter: the share of wall time spent outside the library's calls
With sync_ms well above zero the device is the bottleneck and the glue overlaps it; with sync_ms near zero the host is,
and the glue is on the critical path. The result is one JSON line, also written to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Camera, Renderer, TrainConfig, Trainer, Ubo, View  # noqa: E402
from pathtracer_gaussiansplatting_amd import synthetic as Y  # noqa: E402


class TimedLib:
    """libptgs behind a timer: every ptgs_* call adds its host time to .seconds and counts in .calls."""

    def __init__(self, lib):
        self._lib, self.seconds, self.calls, self._wrapped = lib, 0.0, 0, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ptgs_"):
            return fn
        if name not in self._wrapped:
            def timed(*a, _fn=fn):
                t0 = time.perf_counter()
                try:
                    return _fn(*a)
                finally:
                    self.seconds += time.perf_counter() - t0
                    self.calls += 1
            self._wrapped[name] = timed
        return self._wrapped[name]


def make_views(renderer, g, n_views, W, H):
    cam = Camera(aspect=W / H)
    views = []
    for k in range(n_views):
        a = 2.0 * np.pi * k / n_views
        eye = [0.3 * np.cos(a), 0.3 * np.sin(a), 0.0]
        pose = cam.look_at(eye, [eye[0], eye[1], -1.0])
        u = Ubo()
        u.view[:] = [float(x) for x in pose.view]
        u.proj[:] = [float(x) for x in pose.proj]
        u.camera_pos[:] = [float(x) for x in pose.position]
        img = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
        renderer.splat_gaussians(g, u, W, H, img)
        views.append(View(u, W, H, tuple(float(x) for x in pose.position), img[..., :3].contiguous(), f"view_{k}"))
    torch.cuda.synchronize()
    return views


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "train_bench needs the GPU"
    assert args.warmup + args.rounds * args.steps < TrainConfig().densify_from, "the window must hold no event"
    W, H, n = args.width, args.height, args.n
    r = Renderer(0)
    g = {k: torch.from_numpy(v).cuda() for k, v in Y.gaussians_c2(n, seed=11).items()}
    views = make_views(r, g, args.views, W, H)
    start_colors = (0.5 * (g["colors"] + 0.5)).contiguous()
    opac = g["opacities"].clamp(1e-3, 0.999).contiguous()
    ls, lo, sh = r.checkpoint_init(g["scales"], opac, start_colors, 3)
    params = {"means": g["means"].clone(), "log_scales": ls, "rotations": g["rotations"].clone(), "opacity_logits": lo,
              "sh": sh}
    lib = TimedLib(r.lib)
    r.lib = lib
    extent = float(1.1 * (g["means"] - g["means"].mean(0)).norm(dim=1).max())  # (the eyes are 0.3 from the origin)
    t = Trainer(r, params, views, TrainConfig(), extent=extent)
    first = float(t.train(args.warmup))
    torch.cuda.synchronize()
    rounds = []
    for _ in range(args.rounds):
        lib.seconds, lib.calls = 0.0, 0
        t0 = time.perf_counter()
        loss = t.train(args.steps)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall, sync, inside = (t2 - t0) / args.steps, (t2 - t1) / args.steps, lib.seconds / args.steps
        rounds.append({"ms_per_iter": 1e3 * wall, "in_library_ms": 1e3 * inside, "sync_ms": 1e3 * sync,
                       "glue_ms": 1e3 * (wall - inside - sync), "glue_share": (wall - inside - sync) / wall,
                       "library_calls_per_iter": lib.calls / args.steps})
    last = float(loss)
    res = {"n": n, "sh_degree": 3, "width": W, "height": H, "views": args.views, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "extent": round(t.extent, 4), "gaussians_after": t.count,
           "loss_first_window": round(first, 6), "loss_last": round(last, 6)}
    for k in rounds[0]:
        v = [x[k] for x in rounds]
        res[k] = {"median": round(float(np.median(v)), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    res["iterations_per_s"] = round(1e3 / res["ms_per_iter"]["median"], 2)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
