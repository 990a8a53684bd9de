"""Time the 3DGS depth supervision against the plain backward pass on the same published frame.

    python tools/gs_depth_bench.py [--n 100000] [--width 1920] [--height 1080] [--rounds 7] [--variant NAME ...]

Legs (C2 by default: synthetic.gaussians_c2(100k, seed 1) at 1920x1080, as tools/gs_backward_bench.py):
  forward_published  splat_gaussians(want_stats=True) of a publishing renderer: the frame the others consume
                     (synchronous: the call waits for the pair count, so the figure includes that wait)
  backward           splat_gaussians_backward of that frame (stream-ordered; the frame stays valid, so the call
                     is repeated on the same frame)
  backward_depth     the same with dL_dinvdepth: ptgs_splat_gaussians_backward_depth
  invdepth           splat_gaussians_invdepth of that frame
  invdepth_l1        invdepth_l1_loss with its gradient, on the rendered inverse depth against a synthetic view
                     depth (one pixel in 16 a miss, +inf)
  backward_depth_NAME / backward_NAME   with --variant NAME: the same two legs of libptgs_NAME.so (an A/B build,
                     build.build(variant=NAME, defines=(...))) on its own renderer and frame
Each figure is a torch.cuda.Event pair around `launches` calls after warm-ups; the legs alternate over the rounds
and the median and the range are printed, with backward_depth / backward. No pass / fail threshold: a
measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Camera, Renderer, Ubo  # noqa: E402
from pathtracer_gaussiansplatting_amd import build as B  # noqa: E402
from pathtracer_gaussiansplatting_amd import synthetic as Y  # noqa: E402


def timed(fn, launches, warmup):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--variant", action="append", default=[])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gs_depth_bench needs the GPU"
    W, H, n = args.width, args.height, args.n
    g = {k: torch.from_numpy(v).cuda() for k, v in Y.gaussians_c2(n, seed=1).items()}
    pose = Camera(aspect=W / H).look_at([0.0, 0.0, 0.0], [0.0, 0.0, -1.0])
    ubo = Ubo()
    ubo.view[:] = [float(x) for x in pose.view]
    ubo.proj[:] = [float(x) for x in pose.proj]
    bg = (0.1, 0.2, 0.3)
    gen = torch.Generator(device="cuda").manual_seed(1)
    dL = torch.randn((H, W, 4), device="cuda", generator=gen)
    dinv = torch.randn((H, W), device="cuda", generator=gen)
    target = torch.rand((H, W), device="cuda", generator=gen) * 8.0 + 2.0
    target.view(-1)[::16] = float("inf")
    pub = Renderer(0, publish_splat_buffers=True)
    out = torch.empty((H, W, 4), device="cuda")
    inv, ginv = torch.empty((H, W), device="cuda"), torch.empty((H, W), device="cuda")
    terms = torch.empty(4, device="cuda")
    stats = {}

    def forward_published():
        stats["K"] = pub.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True).num_rendered

    forward_published()
    pub.splat_gaussians_invdepth(W, H, inv)
    legs = {"forward_published": forward_published,
            "backward": lambda: pub.splat_gaussians_backward(g, ubo, W, H, dL, bg=bg),
            "backward_depth": lambda: pub.splat_gaussians_backward(g, ubo, W, H, dL, bg=bg, dL_dinvdepth=dinv),
            "invdepth": lambda: pub.splat_gaussians_invdepth(W, H, inv),
            "invdepth_l1": lambda: pub.invdepth_l1_loss(inv, target, grad_out=ginv, terms_out=terms)}
    frames = {}
    for name in args.variant:
        rv = Renderer(0, lib_path=os.path.join(B.HERE, f"libptgs_{name}.so"), publish_splat_buffers=True)
        out_v = torch.empty((H, W, 4), device="cuda")
        for leg, kw in ((f"backward_{name}", {}), (f"backward_depth_{name}", {"dL_dinvdepth": dinv})):
            frames[leg] = lambda rv=rv, out_v=out_v: rv.splat_gaussians(g, ubo, W, H, out_v, bg=bg, want_stats=True)
            legs[leg] = lambda rv=rv, kw=kw: rv.splat_gaussians_backward(g, ubo, W, H, dL, bg=bg, **kw)
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            if k in frames:
                frames[k]()  # (the frame a variant's backward consumes is its own renderer's latest)
            ms[k].append(timed(fn, args.launches, 5))
    res = {"n": n, "width": W, "height": H, "pairs": stats["K"], "launches": args.launches, "rounds": args.rounds}
    for k, v in ms.items():
        res[k] = {"ms": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    res["backward_depth_over_backward"] = round(res["backward_depth"]["ms"] / res["backward"]["ms"], 3)
    for name in args.variant:
        res[f"backward_depth_{name}_over_backward"] = round(res[f"backward_depth_{name}"]["ms"] / res["backward"]["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
