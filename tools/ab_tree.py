#!/usr/bin/env python3
"""A/B of BVH shapes (leaf size : fan-out : SAH depth budget, api.cpp PTGS_BVH_TRIES) on C5's mesh and
camera: each arm uploads the same scene under its own tree list, then interleaved rounds trace the 4K
frame at AB_SPP samples in ONE process (cdna_hip_programming.md §5.4 rule 24).

  PTGS_BVH_LOG=1 python tools/ab_tree.py default 4:4:38 3:4:34 ...

The arms `opt` and `noopt` upload the default tree with the reinsertion-optimised traversal copy forced on and off
(PTGS_PT_TREE_OPT=1 / 0, csrc/bvh_opt.h): both uploads live in this one process, the images are compared bit for bit
and the copy's report (ptgs_scene_get_tree_opt) is printed:

  python tools/ab_tree.py noopt opt                        (C5's mesh, 3840x2160, 16 spp)
  AB_SCENE=c3 AB_SPP=64 python tools/ab_tree.py noopt opt  (the C3 frame of bench.py)
  AB_SCENE=c3 AB_SPP=1 AB_CALLS=64 python tools/ab_tree.py noopt opt   (the viewer: 64 calls of 1 spp)
"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import numpy as np
    import torch
    from pathtracer_gaussiansplatting_amd import ACCUM_SUM, FLAG_COUNT_TRAVERSAL, Camera, Renderer, make_ubo
    from pathtracer_gaussiansplatting_amd import synthetic as Y
    arms = sys.argv[1:] or ["default"]
    spp = int(os.environ.get("AB_SPP", "16"))
    rounds = int(os.environ.get("AB_ROUNDS", "3"))
    calls = int(os.environ.get("AB_CALLS", "1"))  # consecutive calls per measurement (the viewer: AB_SPP=1 AB_CALLS=64)
    c3 = os.environ.get("AB_SCENE", "c5") == "c3"
    W, H = int(os.environ.get("AB_W", "1920" if c3 else "3840")), int(os.environ.get("AB_H", "1080" if c3 else "2160"))
    scene = Y.atrium_scene(target_tris=int(os.environ.get("AB_TRIS", "250000" if c3 else "1000000")), seed=2)
    scene.blue_noise = Y.blue_noise(1024)
    pose = Camera(aspect=W / H).look_at([-15.0, 4.0, 5.0], [10.0, 3.0, -3.0])
    rs = {}
    for a in arms:
        env = {}
        if a.startswith("env:"):  # env:KEY=VAL+KEY=VAL (e.g. the collapse: env:PTGS_BVH_COLLAPSE=sah+PTGS_BVH_CTRI=0.4)
            env = dict(kv.split("=", 1) for kv in a[4:].split("+"))
        elif a in ("opt", "noopt"):
            env = {"PTGS_PT_TREE_OPT": "1" if a == "opt" else "0"}
        elif a != "default":
            env = {"PTGS_BVH_TRIES": a}
        for k in ("PTGS_BVH_TRIES", "PTGS_PT_TREE_OPT", "PTGS_BVH_COLLAPSE", "PTGS_BVH_CNODE", "PTGS_BVH_CTRI"):
            os.environ.pop(k, None)
        os.environ.update(env)
        r = Renderer(0)
        t_up = time.perf_counter()
        info = r.upload_scene(scene)
        t_up = time.perf_counter() - t_up
        for k in env:
            os.environ.pop(k, None)
        to = r.scene_tree_opt()
        print(f"{a:12s} nodes {info.num_bvh_nodes} depth {info.bvh_depth} leaf {info.max_leaf_size} "
              f"build {info.build_ms:.0f} ms, upload {t_up * 1e3:.0f} ms; traversal copy: "
              + (f"optimised in {to.ms:.0f} ms, nodes {to.num_nodes} need {to.stack_need} depth {to.depth}, area sum "
                 f"{to.area_before:.3f} -> {to.area_after:.3f}" if to.applied else "the canonical tree's"), flush=True)
        rs[a] = r
    os.environ.pop("PTGS_BVH_TRIES", None)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    res = {a: [] for a in arms}
    ref = None
    same = {}
    for rd in range(rounds + 1):
        for a in arms:
            r = rs[a]
            ubo = make_ubo(pose, scene, 0, ambient=(0.3, 0.4, 0.5, 1.0), height=H)
            r.stats_reset()
            acc.zero_()
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(calls):
                r.trace_camera(ubo, W, H, acc, spp=spp, mode=ACCUM_SUM)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            st = r.stats()
            img = acc.cpu().numpy()
            if ref is None:
                ref = img.copy()
            err = float(np.linalg.norm(img - ref) / max(np.linalg.norm(ref), 1e-30))
            same[a] = same.get(a, True) and bool(np.array_equal(img, ref))
            if rd > 0:
                res[a].append(((st.extension_rays + st.shadow_rays) / dt / 1e6, dt * 1e3 / calls, err))
    cnt = {}
    for a in arms:  # traversal work per ray (an untimed pass with the counting kernels)
        r = rs[a]
        r.set_flags(FLAG_COUNT_TRAVERSAL)
        r.stats_reset()
        r.trace_camera(make_ubo(pose, scene, 0, ambient=(0.3, 0.4, 0.5, 1.0), height=H), W, H, acc, spp=spp, mode=ACCUM_SUM)
        torch.cuda.synchronize()
        st = r.stats()
        r.set_flags(0)
        nr = max(st.extension_rays + st.shadow_rays, 1)
        cnt[a] = (st.node_visits / nr, st.tri_tests / nr)
    for a in arms:
        m = [x[0] for x in res[a]]
        ms = np.median([x[1] for x in res[a]])
        print(f"{a:12s} Mrays/s median {np.median(m):9.1f} min {min(m):9.1f} max {max(m):9.1f} ms {ms:8.2f} "
              f"(x{256 // spp} = {ms * 256 / spp:8.1f} ms for 256 spp) rel L2 vs first {max(x[2] for x in res[a]):.1e} ({'bit-equal' if same[a] else 'NOT bit-equal'}) "
              f"child-box tests/ray {cnt[a][0]:.2f} tri tests/ray {cnt[a][1]:.2f}",
              flush=True)


if __name__ == "__main__":
    main()
