"""Time ptgs_gaussians_sh_colors against a device-to-device copy that moves the same bytes.

    python tools/sh_bench.py [--n 1000000] [--degree 3] [--variant NAME] [--rounds 7]

(a) the kernel of libptgs.so; (b) a copy of half the kernel's bytes (the copy reads and writes each
byte, so it moves the same total); (c) with --variant: the same kernel of libptgs_NAME.so, e.g. the
row-per-work-item form built by
    python -c "from pathtracer_gaussiansplatting_amd import build; build.build(variant='shrow', defines=('PTGS_SH_ROWWISE',))"
whose colours must equal (a)'s bit for bit. Each figure is a torch.cuda.Event pair around 20 launches
after 5 warm-ups; the legs alternate over the rounds and the median and the range are printed.
Bytes per Gaussian: 12 (mean) + 12 (degree + 1)^2 (coefficients) + 12 (colour).

--backward times ptgs_gaussians_sh_colors_backward (with the means' gradient) the same way: (a) the kernel,
(b) a copy moving its bytes, N (24 + 24 (degree + 1)^2 + 24): mean, dL/d colour and the coefficient row in,
the dL/d sh row out, the dL/d mean read and written; (c) the variant, whose outputs must equal (a)'s bit for
bit; (d) what the kernel replaces: the backward of a torch restatement of the colour in eager mode
(torch.autograd.grad over a retained graph; "torch_fwd_bwd" includes building that graph)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Renderer  # noqa: E402
from pathtracer_gaussiansplatting_amd import build as B  # noqa: E402


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


def torch_colors(means, sh, cam, degree):
    """The colour of ptgs_gaussians_sh_colors in eager torch (the same expressions; torch's own rounding)."""
    C0, C1 = 0.28209479177387814, 0.4886025119029199
    C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
    C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
          1.445305721320277, -0.5900435899266435)
    d = means - cam[None, :]
    d = d / d.norm(dim=1, keepdim=True)
    x, y, z = d[:, 0:1], d[:, 1:2], d[:, 2:3]
    s = lambda k: sh[:, k, :]  # noqa: E731
    res = C0 * s(0)
    if degree >= 1:
        res = res - C1 * y * s(1) + C1 * z * s(2) - C1 * x * s(3)
    if degree >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + C2[0] * xy * s(4) + C2[1] * yz * s(5) + C2[2] * (2 * zz - xx - yy) * s(6) + C2[3] * xz * s(7)
               + C2[4] * (xx - yy) * s(8))
    if degree >= 3:
        res = (res + C3[0] * y * (3 * xx - yy) * s(9) + C3[1] * xy * z * s(10) + C3[2] * y * (4 * zz - xx - yy) * s(11)
               + C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * s(12) + C3[4] * x * (4 * zz - xx - yy) * s(13)
               + C3[5] * z * (xx - yy) * s(14) + C3[6] * x * (3 * xx - yy) * s(15))
    return torch.clamp_min(res + 0.5, 0.0)


def backward_legs(args, n, K, means, sh, cam, gen):
    """(legs, bytes) of --backward; every leg writes into buffers allocated once."""
    nbytes = n * (24 + 24 * K + 24)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dcol = torch.randn((n, 3), device="cuda", generator=gen)
    camf = np.asarray(cam, np.float32)
    from pathtracer_gaussiansplatting_amd import _abi

    def leg(rend):
        dsh, dmeans = torch.empty_like(sh), torch.zeros_like(means)
        stream = torch.cuda.current_stream().cuda_stream
        a = (rend._h, means.data_ptr(), sh.data_ptr(), n, args.degree, args.degree, _abi.fptr(camf), dcol.data_ptr(),
             dsh.data_ptr(), dmeans.data_ptr(), stream)

        def run():
            assert rend.lib.ptgs_gaussians_sh_colors_backward(*a) == 0
        return run, dsh, dmeans

    legs = {}
    legs["sh_colors_backward"], dsh, dmeans = leg(Renderer(0))
    legs["copy"] = lambda: dst.copy_(src)
    if args.variant:
        rv = Renderer(0, lib_path=os.path.join(B.HERE, f"libptgs_{args.variant}.so"))
        legs[args.variant], dshv, dmeansv = leg(rv)
        legs["sh_colors_backward"]()
        legs[args.variant]()
        torch.cuda.synchronize()
        assert torch.equal(dsh, dshv) and torch.equal(dmeans, dmeansv), "the variant's gradients differ"
    tm, ts, tc = means.clone().requires_grad_(True), sh.clone().requires_grad_(True), torch.tensor(camf, device="cuda")
    graph = torch_colors(tm, ts, tc, args.degree)
    legs["torch_bwd"] = lambda: torch.autograd.grad(graph, (tm, ts), dcol, retain_graph=True)
    legs["torch_fwd_bwd"] = lambda: torch.autograd.grad(torch_colors(tm, ts, tc, args.degree), (tm, ts), dcol)
    return legs, nbytes


def report(args, n, nbytes, legs, first):
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    res = {"n": n, "degree": args.degree, "bytes": nbytes}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "GB_per_s": round(nbytes / med / 1e6, 1)}
    for k in legs:
        if k != first:
            res[f"{first}_over_{k}"] = round(res[first]["ms"] / res[k]["ms"], 3)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backward", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--degree", type=int, default=3)
    ap.add_argument("--variant", default="")
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sh_bench needs the GPU"
    n, K = args.n, (args.degree + 1) ** 2
    gen = torch.Generator(device="cuda").manual_seed(1)
    means = torch.randn((n, 3), device="cuda", generator=gen) * 3.0
    sh = torch.randn((n, K, 3), device="cuda", generator=gen) * 0.5
    cam = (0.3, -1.2, 2.5)
    if args.backward:
        legs, nbytes = backward_legs(args, n, K, means, sh, cam, gen)
        report(args, n, nbytes, legs, "sh_colors_backward")
        return
    nbytes = n * (12 + 12 * K + 12)
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    legs = {}
    r = Renderer(0)
    out = torch.empty((n, 3), device="cuda")
    legs["sh_colors"] = lambda: r.sh_colors(means, sh, cam, out=out)
    legs["copy"] = lambda: dst.copy_(src)
    if args.variant:
        lib = os.path.join(B.HERE, f"libptgs_{args.variant}.so")
        rv = Renderer(0, lib_path=lib)
        outv = torch.empty_like(out)
        legs[args.variant] = lambda: rv.sh_colors(means, sh, cam, out=outv)
        legs["sh_colors"]()
        legs[args.variant]()
        torch.cuda.synchronize()
        assert torch.equal(out, outv), "the variant's colours differ"
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    res = {"n": n, "degree": args.degree, "bytes": nbytes}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                  "GB_per_s": round(nbytes / med / 1e6, 1)}
    res["sh_colors_over_copy"] = round(res["sh_colors"]["ms"] / res["copy"]["ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
