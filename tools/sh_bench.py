"""Time ptgs_gaussians_sh_colors against a device-to-device copy that moves the same bytes.

    python tools/sh_bench.py [--n 1000000] [--degree 3] [--variant NAME] [--rounds 7]

(a) the kernel of libptgs.so; (b) a copy of half the kernel's bytes (the copy reads and writes each
byte, so it moves the same total); (c) with --variant: the same kernel of libptgs_NAME.so, e.g. the
row-per-work-item form built by
    python -c "from pathtracer_gaussiansplatting_amd import build; build.build(variant='shrow', defines=('PTGS_SH_ROWWISE',))"
whose colours must equal (a)'s bit for bit. Each figure is a torch.cuda.Event pair around 20 launches
after 5 warm-ups; the legs alternate over the rounds and the median and the range are printed.
Bytes per Gaussian: 12 (mean) + 12 (degree + 1)^2 (coefficients) + 12 (colour)."""
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


def main():
    ap = argparse.ArgumentParser()
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
