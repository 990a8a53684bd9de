"""Time densification and pruning (ptgs_gaussians_densify_plan / _apply) against a device copy that moves the
apply's bytes and against what the two replace, the trainer's eager-torch sequence.

    python tools/densify_bench.py [--n 1000000] [--rounds 7]

Workload: n Gaussians of degree 3 (59 floats of parameters: mean 3, log-scale 3, rotation 4, logit 1, SH 48)
with both Adam moments of all five parameters (118 floats); about 10 % are cloned, 5 % split and 10 % pruned.
Legs: (1) plan: decision, two-level scan, source map, with its host wait; (2) apply: the gather of the 15
arrays into buffers allocated once; (3) copy: one device-to-device copy of half the apply's bytes (the copy reads
and writes each byte, so it moves the same total); (4) torch: densify_and_clone, densify_and_split and the prune
of the reference trainer in eager torch: boolean-mask indexing and cat of every parameter and moment.
Each figure is a torch.cuda.Event pair around 20 launches after 5 warm-ups; the legs alternate over the rounds
and the median and the range are printed.

Bytes of the apply, N' = A + B + 2 C outputs (A survivors, B clones, C split sources):
    N' (4 + 59 * 8 + 118 * 4) + A 118 * 4 + 2 C 52
the source map; every parameter float read and written; every moment float written, and read for survivors only
(new Gaussians get zeros); a child's mean also reads its parent's rotation, scales and noise (52 bytes)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pathtracer_gaussiansplatting_amd import Renderer, _abi  # noqa: E402

KEYS = ("means", "log_scales", "rotations", "opacity_logits", "sh")
TH = dict(grad_threshold=0.0002, scale_split=0.05, min_opacity=0.005, max_scale=0.5, max_screen_radius=40.0)


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


def workload(n, gen):
    u = lambda lo, hi, *shape: torch.rand(shape, device="cuda", generator=gen) * (hi - lo) + lo  # noqa: E731
    pick = torch.rand(n, device="cuda", generator=gen)
    pruned, cloned, split = pick < 0.10, (pick >= 0.10) & (pick < 0.20), (pick >= 0.20) & (pick < 0.25)
    smax = torch.where(split, u(0.06, 0.45, n), u(0.005, 0.045, n))
    scales = smax[:, None] * u(0.3, 1.0, n, 3)
    scales[:, 0] = smax
    opac = torch.where(pruned, u(0.0005, 0.004, n), u(0.01, 0.99, n))
    P = {"means": torch.randn((n, 3), device="cuda", generator=gen),
         "log_scales": scales.log(),
         "rotations": torch.randn((n, 4), device="cuda", generator=gen),
         "opacity_logits": (opac / (1 - opac)).log(),
         "sh": torch.randn((n, 16, 3), device="cuda", generator=gen) * 0.5}
    M = {k: (torch.randn(v.shape, device="cuda", generator=gen), torch.rand(v.shape, device="cuda", generator=gen))
         for k, v in P.items()}
    denom = torch.full((n,), 4.0, device="cuda")
    accum = torch.where(cloned | split, u(3e-4, 1e-3, n), u(0.0, 1e-4, n)) * denom
    stats = {"accum": accum, "denom": denom, "max_radii": torch.floor(u(0.0, 39.0, n))}
    noise = torch.randn((2, n, 3), device="cuda", generator=gen)
    return P, M, stats, noise


def build_rotation(q):
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.empty((q.shape[0], 3, 3), device=q.device)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)
    return R


def torch_densify(P, M, stats, noise):
    """densify_and_prune of the reference trainer (cat_tensors_to_optimizer / _prune_optimizer on every
    parameter and both moments), new Gaussians inheriting the parent's screen radius."""
    n = P["means"].shape[0]
    grads = torch.where(stats["denom"] > 0, stats["accum"] / stats["denom"], torch.zeros_like(stats["accum"]))
    radii = stats["max_radii"]

    def extend(P, M, new):
        P2 = {k: torch.cat((P[k], new[k])) for k in KEYS}
        M2 = {k: tuple(torch.cat((m, torch.zeros_like(new[k]))) for m in M[k]) for k in KEYS}
        return P2, M2

    def keep(P, M, valid):
        return {k: P[k][valid] for k in KEYS}, {k: tuple(m[valid] for m in M[k]) for k in KEYS}

    # densify_and_clone
    mask = (grads >= TH["grad_threshold"]) & (P["log_scales"].exp().max(dim=1).values <= TH["scale_split"])
    P, M = extend(P, M, {k: P[k][mask] for k in KEYS})
    radii = torch.cat((radii, radii[mask]))
    # densify_and_split
    padded = torch.zeros(P["means"].shape[0], device="cuda")
    padded[:n] = grads
    scales = P["log_scales"].exp()
    mask = (padded >= TH["grad_threshold"]) & (scales.max(dim=1).values > TH["scale_split"])
    stds = scales[mask].repeat(2, 1)
    samples = stds * torch.cat((noise[0][mask[:n]], noise[1][mask[:n]]))
    rots = build_rotation(P["rotations"][mask]).repeat(2, 1, 1)
    new = {"means": torch.bmm(rots, samples.unsqueeze(-1)).squeeze(-1) + P["means"][mask].repeat(2, 1),
           "log_scales": (stds / 1.6).log(), "rotations": P["rotations"][mask].repeat(2, 1),
           "opacity_logits": P["opacity_logits"][mask].repeat(2), "sh": P["sh"][mask].repeat(2, 1, 1)}
    P, M = extend(P, M, new)
    radii = torch.cat((radii, radii[mask].repeat(2)))
    valid = ~torch.cat((mask, torch.zeros(2 * int(mask.sum()), dtype=torch.bool, device="cuda")))
    P, M = keep(P, M, valid)
    radii = radii[valid]
    # prune
    prune = torch.sigmoid(P["opacity_logits"]) < TH["min_opacity"]
    prune |= radii > TH["max_screen_radius"]
    prune |= P["log_scales"].exp().max(dim=1).values > TH["max_scale"]
    return keep(P, M, ~prune)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "densify_bench needs the GPU"
    n = args.n
    gen = torch.Generator(device="cuda").manual_seed(1)
    P, M, stats, noise = workload(n, gen)
    r = Renderer(0)
    scales, opac = r.activate_gaussians(P["log_scales"], P["opacity_logits"])
    plan = lambda: r.densify_plan(scales, opac, stats["accum"], stats["denom"], stats["max_radii"], **TH)  # noqa: E731
    counts = plan()
    A, B, Cs, total = counts.survivors, counts.clones, counts.split_sources, counts.total
    # the apply's arrays, allocated once
    srcs = [(P["rotations"], 0), (P["opacity_logits"], 0), (P["sh"], 0)]
    srcs += [(m, 1) for k in KEYS for m in M[k]]
    new = lambda t: torch.empty((total,) + tuple(t.shape[1:]), device="cuda")  # noqa: E731
    means_out, ls_out = new(P["means"]), new(P["log_scales"])
    dsts = [new(t) for t, _ in srcs]
    rows = (_abi.DensifyRows * len(srcs))()
    for k, ((t, z), o) in enumerate(zip(srcs, dsts)):
        rows[k].src, rows[k].dst, rows[k].width, rows[k].zero_new = t.data_ptr(), o.data_ptr(), t.numel() // n, z
    stream = torch.cuda.current_stream().cuda_stream
    a = (r._h, n, total, P["means"].data_ptr(), P["log_scales"].data_ptr(), P["rotations"].data_ptr(),
         scales.data_ptr(), noise.data_ptr(), means_out.data_ptr(), ls_out.data_ptr(), rows, len(srcs), None, stream)

    def apply():
        assert r.lib.ptgs_gaussians_densify_apply(*a) == 0

    nbytes = total * (4 + 59 * 8 + 118 * 4) + A * 118 * 4 + 2 * Cs * 52
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    # the torch sequence reaches the same set (its own rounding in exp / log: compare sizes and the copied rows)
    apply()
    Pt, Mt = torch_densify(P, M, stats, noise)
    torch.cuda.synchronize()
    assert Pt["means"].shape[0] == total, (Pt["means"].shape[0], total)
    assert torch.equal(Pt["sh"], dsts[2]) and torch.equal(Mt["sh"][0], dsts[3 + 2 * KEYS.index("sh")])
    del Pt, Mt
    legs = {"plan": plan, "apply": apply, "copy": lambda: dst.copy_(src),
            "torch": lambda: torch_densify(P, M, stats, noise)}
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, fn in legs.items():
            ms[k].append(timed(fn))
    res = {"n": n, "total": total, "survivors": A, "clones": B, "split_sources": Cs,
           "pruned_originals": counts.pruned_originals, "pruned_children": counts.pruned_children, "apply_bytes": nbytes,
           "apply_bytes_per_output": round(nbytes / total, 1)}
    for k, v in ms.items():
        med = float(np.median(v))
        res[k] = {"ms": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
        if k in ("apply", "copy"):
            res[k]["GB_per_s"] = round(nbytes / med / 1e6, 1)
    res["apply_over_copy"] = round(res["apply"]["ms"] / res["copy"]["ms"], 3)
    res["plan_plus_apply_ms"] = round(res["plan"]["ms"] + res["apply"]["ms"], 4)
    res["torch_over_plan_plus_apply"] = round(res["torch"]["ms"] / res["plan_plus_apply_ms"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
