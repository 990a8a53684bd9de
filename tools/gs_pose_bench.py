"""Time the camera-pose gradient against the backward passes it rides on, on the same published frame.

    python tools/gs_pose_bench.py [--n 100000] [--width 1920] [--height 1080] [--sh-n 1000000] [--rounds 7]
                                  [--out profiles/gs_pose_bench.json]

Legs (C2 by default: synthetic.gaussians_c2(100k, seed 1) at 1920x1080, as tools/gs_backward_bench.py), all on one
frame of one publishing renderer, interleaved over the rounds:
  backward             splat_gaussians_backward (ptgs_splat_gaussians_backward)
  backward_pose        the same with want_view: ptgs_splat_gaussians_backward_pose, colour only
  backward_depth       with dL_dinvdepth: ptgs_splat_gaussians_backward_depth
  backward_pose_depth  with dL_dinvdepth and want_view: ptgs_splat_gaussians_backward_pose
and, at --sh-n Gaussians of degree 3 (the C calls on buffers allocated once, as tools/sh_bench.py --backward):
  sh_backward          ptgs_gaussians_sh_colors_backward with the means' gradient
  sh_backward_eye      ptgs_gaussians_sh_colors_backward_eye, the same plus dL/d camera_pos
Each figure is a torch.cuda.Event pair around `launches` calls after warm-ups; the median and the range are
printed with each pose form over its plain counterpart of the same run. No pass / fail threshold: a measurement."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Camera, Renderer, Ubo, _abi  # noqa: E402
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


def sh_legs(rend, n, gen):
    K = 16
    means = torch.randn((n, 3), device="cuda", generator=gen) * 3.0
    sh = torch.randn((n, K, 3), device="cuda", generator=gen) * 0.5
    dcol = torch.randn((n, 3), device="cuda", generator=gen)
    dsh, dmeans = torch.empty_like(sh), torch.zeros_like(means)
    deye = torch.empty(3, device="cuda")
    cam = np.asarray((0.3, -1.2, 2.5), np.float32)
    stream = torch.cuda.current_stream().cuda_stream
    a = (rend._h, means.data_ptr(), sh.data_ptr(), n, 3, 3, _abi.fptr(cam), dcol.data_ptr(), dsh.data_ptr(),
         dmeans.data_ptr())

    def plain():
        assert rend.lib.ptgs_gaussians_sh_colors_backward(*a, stream) == 0

    def eye():
        assert rend.lib.ptgs_gaussians_sh_colors_backward_eye(*a, deye.data_ptr(), stream) == 0

    return {"sh_backward": plain, "sh_backward_eye": eye}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--sh-n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gs_pose_bench needs the GPU"
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
    pub = Renderer(0, publish_splat_buffers=True)
    out = torch.empty((H, W, 4), device="cuda")
    K = pub.splat_gaussians(g, ubo, W, H, out, bg=bg, want_stats=True).num_rendered

    def backward(**kw):
        return lambda: pub.splat_gaussians_backward(g, ubo, W, H, dL, bg=bg, **kw)

    legs = {"backward": backward(), "backward_pose": backward(want_view=True),
            "backward_depth": backward(dL_dinvdepth=dinv),
            "backward_pose_depth": backward(dL_dinvdepth=dinv, want_view=True)}
    legs.update(sh_legs(pub, args.sh_n, gen))
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn, args.launches, 5))
    res = {"n": n, "width": W, "height": H, "pairs": K, "sh_n": args.sh_n, "sh_degree": 3, "launches": args.launches,
           "rounds": args.rounds}
    for k, v in ms.items():
        res[k] = {"ms": round(float(np.median(v)), 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    for a, b in (("backward_pose", "backward"), ("backward_pose_depth", "backward_depth"),
                 ("sh_backward_eye", "sh_backward")):
        res[f"{a}_over_{b}"] = round(res[a]["ms"] / res[b]["ms"], 3)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
