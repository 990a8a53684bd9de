"""Time the 3DGS training loss (ptgs_image_loss_l1_dssim: L1 + D-SSIM and its gradient) against a device copy that
moves the call's minimum bytes and against what it replaces, the same loss forward + backward in eager torch.

    python tools/loss_bench.py [--width 1920] [--height 1080] [--gaussians 100000] [--rounds 7]

Workload: a frame of the synthetic Gaussians rendered by the rasterizer (RGBA32F) and a perturbed copy of it as the
target (C = 4), lambda = 0.2. Legs: (1) the call with the gradient; (2) the call with the loss only; (3) copy: one
device-to-device copy of 24 bytes per pixel (the copy reads and writes each byte, so it moves the call's minimum of
48: image 16 + target 16 read, gradient 16 written); (4) torch: the F.conv2d formulation (five grouped 11 x 11
convolutions, the element-wise map, autograd's backward) in float32 on the GPU.
Each figure is a torch.cuda.Event pair around 20 launches after 5 warm-ups; the legs alternate over the rounds and
the median and the range are printed."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Camera, Renderer, cornell_box_scene, make_ubo  # noqa: E402
from pathtracer_gaussiansplatting_amd import synthetic as Y  # noqa: E402

LAMBDA = 0.2


def timed(fn, launches=20, warmup=5):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / launches


def torch_window():
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-((k - 5) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    return (g[:, None] * g[None, :]).float().expand(3, 1, 11, 11).contiguous().cuda()


def torch_loss(image, target, w):
    """(loss, dloss/dimage) of the eager formulation; image is a leaf [H, W, 4]."""
    image.grad = None
    a = image[..., :3].permute(2, 0, 1)[None]
    b = target[..., :3].permute(2, 0, 1)[None]
    cv = lambda x: F.conv2d(x, w, padding=5, groups=3)  # noqa: E731
    mu1, mu2 = cv(a), cv(b)
    s1, s2, s12 = cv(a * a) - mu1 * mu1, cv(b * b) - mu2 * mu2, cv(a * b) - mu1 * mu2
    m = (2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s1 + s2 + 9e-4))
    loss = (1.0 - LAMBDA) * (a - b).abs().mean() + LAMBDA * (1.0 - m.mean())
    loss.backward()
    return loss.detach(), image.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--gaussians", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "loss_bench needs the GPU"
    W, H = args.width, args.height
    r = Renderer(0)
    g = {k: torch.from_numpy(v).cuda() for k, v in Y.gaussians_c2(args.gaussians, seed=11).items()}
    ubo = make_ubo(Camera(aspect=W / H).look_at([0.0, 0.0, 0.0], [0.0, 0.0, -1.0]), cornell_box_scene(), 0)
    image = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    r.splat_gaussians(g, ubo, W, H, image, want_stats=True)
    gen = torch.Generator(device="cuda").manual_seed(1)
    target = (image + 0.05 * torch.randn(image.shape, device="cuda", generator=gen)).clamp_(0.0, 1.0)
    grad = torch.empty_like(image)
    terms = torch.empty(4, dtype=torch.float32, device="cuda")
    w = torch_window()
    leaf = image.clone().requires_grad_(True)
    # both sides compute the same thing
    r.l1_dssim_loss(image, target, LAMBDA, grad_out=grad, terms_out=terms)
    tl, tg = torch_loss(leaf, target, w)
    torch.cuda.synchronize()
    agree = {"loss_rel": abs(float(terms[0]) - float(tl)) / abs(float(tl)),
             "grad_rel_l2": float((grad - tg).norm() / tg.norm())}
    assert agree["loss_rel"] < 1e-4 and agree["grad_rel_l2"] < 1e-3, agree
    px = W * H
    src = torch.empty(24 * px, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    legs = {"loss_grad": lambda: r.l1_dssim_loss(image, target, LAMBDA, grad_out=grad, terms_out=terms),
            "loss_only": lambda: r.l1_dssim_loss(image, target, LAMBDA, terms_out=terms),
            "copy": lambda: dst.copy_(src),
            "torch": lambda: torch_loss(leaf, target, w)}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    res = {"width": W, "height": H, "gaussians": args.gaussians, "lambda": LAMBDA, "loss": round(float(terms[0]), 6),
           "agreement_with_torch": {k: float(f"{v:.2e}") for k, v in agree.items()}, "min_bytes": 48 * px}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    res["copy"]["GB_per_s"] = round(48 * px / res["copy"]["ms"] / 1e6, 1)
    res["loss_grad"]["GB_per_s_of_min_bytes"] = round(48 * px / res["loss_grad"]["ms"] / 1e6, 1)
    res["loss_grad_over_copy"] = round(res["loss_grad"]["ms"] / res["copy"]["ms"], 2)
    res["torch_over_loss_grad"] = round(res["torch"]["ms"] / res["loss_grad"]["ms"], 2)
    print(json.dumps(res))
    r.close()


if __name__ == "__main__":
    main()
