"""Time the optimizer step (ptgs_gaussians_adam_step) against a device copy that moves the dense step's bytes and
against what it replaces, torch.optim.Adam.

    python tools/adam_bench.py [--n 1000000] [--rounds 7] [--visible 0.3] [--run 64]

Workload: n Gaussians of degree 3, all five parameters (59 floats: mean 3, log-scale 3, rotation 4, logit 1, SH 48)
with their moments; gradients N(0, 1e-3) with 30 % exact zeros; the SH row steps with head 3 (the DC term's rate).
Legs: (1) dense: the call with radii NULL; (2) masked: the call with radii that make `--visible` of the Gaussians
visible, in clustered runs: visible and invisible runs alternate, each length a geometric draw (>= 1), mean `--run`
for the visible runs and run * (1 - visible) / visible for the invisible ones (a spatially sorted set seen by one
camera: neighbours in memory share their fate; the saving on the narrow rows depends on this, a masked-out row of
width 1 or 3 only saves traffic where its cache line's other rows are masked out too); (3) copy: one
device-to-device copy of half the dense step's bytes (the copy reads and writes each byte, so it moves the same
total); (4) torch: torch.optim.Adam on the same five tensors, default (foreach); (5) torch_fused:
torch.optim.Adam(fused=True), when it constructs on this build. Each figure is a torch.cuda.Event pair around 20 calls
after 5 warm-ups; the legs alternate over the rounds and the median and the range are printed.

Bytes: a float that steps moves 28 (g, p, m, v read; p, m, v written), so the dense step moves n * 59 * 28; the
masked step V * 59 * 28 + n * 4 * 5 (V visible; each of the five segments reads the radii)."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Renderer, _abi  # noqa: E402

SHAPES = {"means": (3,), "log_scales": (3,), "rotations": (4,), "opacity_logits": (), "sh": (16, 3)}
LR = {"means": 0.00016, "log_scales": 0.005, "rotations": 0.001, "opacity_logits": 0.025, "sh": 0.0025 / 20}
FLOATS = 59


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


def clustered_radii(n, visible, run, rng):
    """int32 [n]: alternating visible (radius 1..49) and invisible (0) runs of random length."""
    mean = {True: run, False: run * (1.0 - visible) / visible}
    radii = np.zeros(n, np.int32)
    at, vis, lengths = 0, bool(rng.random() < visible), {True: [], False: []}
    while at < n:
        length = min(int(rng.geometric(1.0 / max(mean[vis], 1.0))), n - at)
        if vis:
            radii[at:at + length] = rng.integers(1, 50, length)
        lengths[vis].append(length)
        at += length
        vis = not vis
    return radii, lengths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--visible", type=float, default=0.3)
    ap.add_argument("--run", type=float, default=64.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "adam_bench needs the GPU"
    n = args.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    P = {k: torch.randn((n,) + s, device="cuda", generator=gen) for k, s in SHAPES.items()}
    G = {}
    for k, p in P.items():
        g = torch.randn(p.shape, device="cuda", generator=gen) * 1e-3
        g[torch.rand(p.shape, device="cuda", generator=gen) < 0.3] = 0
        G[k] = g
    rng = np.random.default_rng(2)
    radii_h, lengths = clustered_radii(n, args.visible, args.run, rng)
    radii = torch.from_numpy(radii_h).cuda()
    V = int((radii_h > 0).sum())
    r = Renderer(0)
    stream = torch.cuda.current_stream().cuda_stream

    def table():
        """(the C table over fresh copies of the parameters with zero moments, the tensors it points at)"""
        keep = {k: (P[k].clone(), torch.zeros_like(P[k]), torch.zeros_like(P[k])) for k in P}
        arr = (_abi.AdamRows * len(P))()
        for i, (k, (p, m, v)) in enumerate(keep.items()):
            arr[i].param, arr[i].grad, arr[i].exp_avg, arr[i].exp_avg_sq = p.data_ptr(), G[k].data_ptr(), m.data_ptr(), v.data_ptr()
            arr[i].width, arr[i].lr = p.numel() // n, LR[k]
            if k == "sh":
                arr[i].head, arr[i].lr_head = 3, 0.0025
        return arr, keep

    step = [0]

    def call(arr, rp):
        step[0] += 1
        prm = _abi.AdamParams(0.9, 0.999, 1e-15, step[0])
        assert r.lib.ptgs_gaussians_adam_step(r._h, n, arr, len(P), C.byref(prm), rp, stream) == 0

    dense_arr, dense_keep = table()
    masked_arr, masked_keep = table()
    # the masked call leaves what it does not see as it was, and moves what it sees
    call(masked_arr, radii.data_ptr())
    torch.cuda.synchronize()
    hidden = radii <= 0
    for k in P:
        assert torch.equal(masked_keep[k][0][hidden], P[k][hidden]) and not bool(masked_keep[k][2][hidden].any())
    assert not torch.equal(masked_keep["sh"][0][~hidden], P["sh"][~hidden])

    def torch_adam(**kw):
        leaves = [P[k].clone().requires_grad_(True) for k in P]
        for t, k in zip(leaves, P):
            t.grad = G[k]
        return torch.optim.Adam([{"params": [t], "lr": LR[k]} for t, k in zip(leaves, P)], eps=1e-15, **kw)

    nbytes = n * FLOATS * 28
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    legs = {"dense": lambda: call(dense_arr, None), "masked": lambda: call(masked_arr, radii.data_ptr()),
            "copy": lambda: dst.copy_(src), "torch": torch_adam().step}
    fused_error = None
    try:
        fused = torch_adam(fused=True)
        fused.step()
        torch.cuda.synchronize()
        legs["torch_fused"] = fused.step
    except Exception as e:  # this build of torch has no fused Adam for the device
        fused_error = f"{type(e).__name__}: {e}"
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    mean = lambda v: round(float(np.mean(v)), 1) if v else 0.0  # noqa: E731
    res = {"n": n, "visible": V, "visible_fraction": round(V / n, 4),
           "visible_run_mean": mean(lengths[True]), "invisible_run_mean": mean(lengths[False]),
           "dense_bytes": nbytes, "masked_bytes": V * FLOATS * 28 + n * 4 * len(P)}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
    res["dense"]["GB_per_s"] = round(nbytes / res["dense"]["ms"] / 1e6, 1)
    res["copy"]["GB_per_s"] = round(nbytes / res["copy"]["ms"] / 1e6, 1)
    res["masked"]["GB_per_s"] = round(res["masked_bytes"] / res["masked"]["ms"] / 1e6, 1)
    best = min((k for k in ("torch", "torch_fused") if k in res), key=lambda k: res[k]["ms"])
    res["torch_fused_error"] = fused_error
    res["dense_over_copy"] = round(res["dense"]["ms"] / res["copy"]["ms"], 3)
    res["masked_over_dense"] = round(res["masked"]["ms"] / res["dense"]["ms"], 3)
    res["best_torch"] = best
    res["best_torch_over_dense"] = round(res[best]["ms"] / res["dense"]["ms"], 2)
    res["best_torch_over_masked"] = round(res[best]["ms"] / res["masked"]["ms"], 2)
    res["torch_foreach_over_dense"] = round(res["torch"]["ms"] / res["dense"]["ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
