"""The megakernel's own LDS stack depth (pt_device.h PTGS_PT_STACK) and the stack-budgeted collapse that lets the
tree it walks meet it (csrc/bvh_opt.h collapse_bvh4_budget; the scene upload's upload_traversal_nodes;
ptgs_scene_get_pt_stack).

CPU part, two stand-alone programs (their own main, host code only: bvh.cpp, bvh_opt.cpp), built here with
g++ -fsanitize=address,undefined and run directly:
  tests/native/tree_opt_check.cpp at the new limits: PTGS_PT_STACK, and limits tight enough to bind on the small
    meshes (the reinserted BVH2's height + 1, the tightest feasible one) or to be infeasible (that height);
  tests/native/tree_budget_check.cpp for what that program cannot see: a budget that does not bind gives the greedy
    collapse's bytes; every limit from the greedy need down to the BVH2's height + 1 gives need < limit with the
    greedy tree's leaves; the height itself is refused; the optimiser applies, falls back and orders two limits
    accordingly.

GPU part: the megakernel against the CPU oracle and against the same render with PTGS_PT_TREE_OPT=0, images bit
for bit and ray counts equal, and the launch rule at its boundary: ptgs_scene_get_pt_stack must say DEEP exactly when
the walked copy's need reaches PTGS_PT_STACK (a write past the LDS stack would be silent corruption, not a fault;
no test provokes one)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bvh_soups as B
import scenes_util as U
from bvh_soups import geometric_slivers as _geometric_slivers, strip as _strip
from pathtracer_gaussiansplatting_amd import make_ubo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(HERE, "native")

PT_STACK = 30     # pt_device.h PTGS_PT_STACK: the plain instantiations' LDS entries, and the launch rule's bound
DEEP_STACK = 39   # pt_device.h PTGS_STACK: the DEEP instantiations' LDS entries
STACK_TOTAL = 48  # pt_device.h PTGS_STACK_TOTAL


def _build(name):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out_dir = os.path.join(NATIVE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name + "_budget")  # (its own binary: tests/test_pt_tree_opt.py builds tree_opt_check too)
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(CSRC, "bvh_opt.cpp"), os.path.join(NATIVE, name + ".cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("bvh.h", "bvh_opt.h", "stack_key.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.fixture(scope="module")
def opt_check():
    return _build("tree_opt_check")


@pytest.fixture(scope="module")
def budget_check():
    return _build("tree_budget_check")


def _run(binary, tmp_path, tri, tries, *more):
    path = os.path.join(str(tmp_path), "tris.bin")
    np.ascontiguousarray(tri, np.float32).tofile(path)
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([binary, path, leaf, fan, depth] + [str(m) for m in more], capture_output=True, text=True,
                       timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                                         "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    return {k: (float(v) if "." in v else int(v)) for k, v in zip(w[1::2], w[2::2])}


_CACHE = {}


def _scene(name):
    """The test scenes, built once per module (no test changes them)."""
    if name not in _CACHE:
        _CACHE[name] = {"features": U.features, "atrium": U.atrium}[name]()
    return _CACHE[name]


def _triangles(sc):
    return B.triangles(sc).reshape(-1, 9)


def _slivers(n=257):
    """A strip of thin triangles sorted along x (each 1e-3 wide, 1 long, slightly tilted)."""
    x = np.arange(n + 1, dtype=np.float32) * np.float32(1e-3)
    return _strip(x)


# what tree_budget_check reports for the reinserted BVH2 of each mesh (opt_height2; test_budget_check pins them)
_HEIGHT = {("slivers", "1:4:38"): 9, ("features", "1:4:38"): 22, ("features", "3:4:38"): 20}


@pytest.mark.parametrize("mesh,tries,limit,applied", [
    ("slivers", "1:4:38", PT_STACK, 1), ("slivers", "1:4:38", 10, 1), ("slivers", "1:4:38", 9, 0),
    ("features", "1:4:38", PT_STACK, 1), ("features", "1:4:38", 23, 1), ("features", "1:4:38", 22, 0),
    ("features", "3:4:38", PT_STACK, 1), ("features", "3:4:38", 21, 1),
    ("atrium", "3:4:38", PT_STACK, 1)])
def test_opt_check_at_the_new_limits(opt_check, tmp_path, mesh, tries, limit, applied):
    """tree_opt_check's structure, byte-identical reruns and both lockstep walks against brute force (no stack write
    at or above the need) under PTGS_PT_STACK, under the tightest feasible limit (the reinserted BVH2's height + 1),
    and under that height, where no collapse fits and the canonical nodes are converted."""
    tri = _slivers() if mesh == "slivers" else _triangles(_scene(mesh))
    st = _run(opt_check, tmp_path, tri, tries, 16, limit)
    assert st["violations"] == 0 and st["limit"] == limit and st["applied"] == applied
    assert st["hits"] > 0
    if applied:
        assert st["need_opt"] < limit and st["fan_opt"] == 4
        assert 0 < st["c_high_water_opt"] <= st["need_opt"]
        if (mesh, tries) in _HEIGHT and limit == _HEIGHT[(mesh, tries)] + 1:
            assert st["need_opt"] == limit - 1  # (no collapse needs less than the BVH2's height)
    else:
        assert (st["nodes_opt"], st["need_opt"]) == (st["nodes_can"], st["need_can"])
    if mesh == "atrium":
        # the C3 mesh under the megakernel's budget: what the budget costs in node steps on the seeded waves
        print(f"atrium under limit {limit}: nodes {st['nodes_opt']}, need {st['need_opt']}, depth {st['depth_opt']}, "
              f"area sum {st['area_opt']:.3f}, closest-hit wave node steps {st['c_node_steps_opt']} "
              f"(canonical {st['c_node_steps_can']}), any-hit {st['a_node_steps_opt']} ({st['a_node_steps_can']})")
        assert st["need_can"] == 38 and st["c_node_steps_opt"] < st["c_node_steps_can"]


@pytest.mark.parametrize("mesh,tries", [("slivers", "1:4:38"), ("slivers", "3:4:38"), ("slivers", "1:3:38"),
                                        ("slivers", "1:2:38"), ("geometric", "1:4:38"), ("features", "1:4:38"),
                                        ("features", "3:4:38")])
def test_budget_check(budget_check, tmp_path, mesh, tries):
    """tree_budget_check: the non-binding budget's bytes, every feasible limit, the infeasible one, and the optimiser's
    use of them. Fan-out 2 has nothing to narrow (its need is the height): only the refusals run there."""
    tri = {"slivers": _slivers, "geometric": lambda: _geometric_slivers(41, 1.5)}.get(mesh, lambda: _triangles(_scene(mesh)))()
    st = _run(budget_check, tmp_path, tri, tries)
    assert st["violations"] == 0
    assert st["height2"] <= st["need_greedy"] and st["limits_run"] == st["need_greedy"] - st["height2"]
    if st["limits_run"]:
        assert st["need_tight"] == st["height2"]
    assert st["opt_applied"] == 1 and st["opt_applied_tight"] == 1 and st["opt_applied_below"] == 0
    assert st["opt_need_tight"] == st["opt_height2"] and st["opt_limit_two"] == st["opt_need_greedy"] + 1
    if (mesh, tries) in _HEIGHT:
        assert st["opt_height2"] == _HEIGHT[(mesh, tries)]


# ---------------------------------------------------------------------------------------------------
# GPU: the megakernel under its own stack depth, against the oracle and against the canonical copy
# ---------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(oracle_lib, key, sc, ubo, W, H, spp):
    """The oracle's image and ray counts, once per (scene, size, spp)."""
    if key not in _ORACLE:
        o = np.zeros((H, W, 4), np.float32)
        so = oracle_lib.trace_camera(sc.desc(), ubo, W, H, o, spp=spp)
        o.setflags(write=False)
        _ORACLE[key] = (o, so.extension_rays, so.shadow_rays)
    return _ORACLE[key]


def _render(renderer, monkeypatch, sc, ubo, W, H, spp, opt):
    """An upload with PTGS_PT_TREE_OPT unset (opt None: the upload's own policy) or set, and one render: image, ray
    counts, the copy's report, the canonical build's, and the megakernel's (LDS depth, walked need, deep)."""
    import torch
    if opt is None:
        monkeypatch.delenv("PTGS_PT_TREE_OPT", raising=False)
    else:
        monkeypatch.setenv("PTGS_PT_TREE_OPT", str(opt))
    renderer.set_wavefront(False)
    renderer.upload_scene(sc)  # (reads PTGS_PT_TREE_OPT and PTGS_BVH_TRIES)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.stats_reset()
    renderer.trace_camera(ubo, W, H, acc, spp=spp)
    torch.cuda.synchronize()
    st = renderer.stats()
    return {"img": acc.cpu().numpy(), "rays": (st.extension_rays, st.shadow_rays), "opt": renderer.scene_tree_opt(),
            "build": renderer.scene_build(), "stack": renderer.scene_pt_stack()}


def _check_rule(r):
    """The launch rule, whatever copy is walked: its need is the optimised copy's when that is applied, else the
    canonical tree's; DEEP exactly when it reaches the LDS depth; and it fits LDS + overflow."""
    lds, need, deep = r["stack"]
    assert lds == (DEEP_STACK if deep else PT_STACK)
    assert need == (r["opt"].stack_need if r["opt"].applied else r["build"].stack_need)
    assert deep == (need >= PT_STACK) and need < STACK_TOTAL


def _on_off_oracle(renderer, oracle_lib, monkeypatch, key, sc, ubo, W, H, spp, on_opt=None):
    on = _render(renderer, monkeypatch, sc, ubo, W, H, spp, on_opt)
    off = _render(renderer, monkeypatch, sc, ubo, W, H, spp, 0)
    o, ext, shd = _oracle(oracle_lib, key, sc, ubo, W, H, spp)
    print(f"{key}: applied {on['opt'].applied}/{off['opt'].applied}, canonical need {on['build'].stack_need}, megakernel "
          f"(LDS depth, walked need, deep) {on['stack']} / {off['stack']}")
    assert off["opt"].applied == 0 and ext > 0
    for r in (on, off):
        _check_rule(r)
        assert np.array_equal(r["img"], o)
        assert r["rays"] == (ext, shd)
    return on, off


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["features", "atrium"])
def test_budgeted_copy_runs_the_plain_instantiation(renderer, oracle_lib, monkeypatch, name):
    """160x120 at 2 spp: the optimised copy meets the megakernel's budget and is not DEEP. The atrium's canonical tree
    needs 38: converted as it is (PTGS_PT_TREE_OPT=0) it is DEEP under the shorter stack, with the same image."""
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene(name)
    if name == "features":
        ubo = make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    else:
        ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    on, off = _on_off_oracle(renderer, oracle_lib, monkeypatch, f"{name} 160x120 2spp", sc, ubo, 160, 120, 2)
    assert on["opt"].applied == 1 and on["rays"][1] > 0
    assert on["stack"] == (PT_STACK, on["opt"].stack_need, False)
    assert on["build"].deep_stack == off["build"].deep_stack == 0  # (the canonical tree's kernels: PTGS_STACK)
    if name == "atrium":
        assert off["stack"] == (DEEP_STACK, 38, True)


@pytest.mark.gpu
def test_atrium_with_one_triangle_leaves(renderer, oracle_lib, monkeypatch):
    """Canonical need 40: DEEP for every kernel that walks the canonical nodes, and for the megakernel when the copy
    is that tree's conversion. The optimised copy is DEEP only if the budget was infeasible."""
    monkeypatch.setenv("PTGS_BVH_TRIES", "1:4:38")
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    on, off = _on_off_oracle(renderer, oracle_lib, monkeypatch, "atrium 160x120 2spp", sc, ubo, 160, 120, 2)
    assert on["opt"].applied == 1 and on["build"].stack_need == 40 and on["build"].deep_stack == 1
    assert off["stack"] == (DEEP_STACK, 40, True)


@pytest.mark.gpu
def test_lbvh_upload(renderer, oracle_lib, monkeypatch):
    """PTGS_FLAG_GPU_LBVH: converted as it is, so the megakernel's rule reads the canonical need; PTGS_PT_TREE_OPT=1
    asks for the optimised copy of it."""
    from pathtracer_gaussiansplatting_amd import FLAG_GPU_BVH, FLAG_GPU_LBVH
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    renderer.set_flags(FLAG_GPU_BVH | FLAG_GPU_LBVH)
    try:
        plain, off = _on_off_oracle(renderer, oracle_lib, monkeypatch, "atrium 160x120 2spp", sc, ubo, 160, 120, 2)
        asked = _render(renderer, monkeypatch, sc, ubo, 160, 120, 2, 1)
    finally:
        renderer.set_flags(0)
    assert plain["build"].builder == 2 and plain["opt"].applied == 0
    lbvh_deep = plain["build"].stack_need >= PT_STACK
    assert plain["stack"] == off["stack"] == (DEEP_STACK if lbvh_deep else PT_STACK, plain["build"].stack_need, lbvh_deep)
    _check_rule(asked)
    assert asked["opt"].applied == 1
    assert np.array_equal(asked["img"], plain["img"]) and asked["rays"] == plain["rays"]


# geometric sliver strips whose canonical tree (1-triangle leaves, 4-wide) needs exactly PTGS_PT_STACK - 1 and
# PTGS_PT_STACK entries (lengths found with tests/native/tree_budget_check.cpp: need_greedy)
_BOUNDARY = {PT_STACK - 1: (41, 1.5), PT_STACK: (47, 1.4)}  # need: (triangles, ratio)


@pytest.mark.gpu
@pytest.mark.parametrize("need", sorted(_BOUNDARY))
def test_launch_rule_at_its_boundary(renderer, oracle_lib, monkeypatch, need):
    """64x64 at 2 spp, seen along the strip from its narrow end, where the chain is deepest. Converted as it is
    (PTGS_PT_TREE_OPT=0), the strip whose need is PTGS_PT_STACK - 1 may fill the LDS stack to its last entry and
    runs the plain instantiation; one more entry and it runs DEEP. The optimised copy follows the same rule on
    its own need."""
    from pathtracer_gaussiansplatting_amd import scene as S
    monkeypatch.setenv("PTGS_BVH_TRIES", "1:4:38")
    tri = _geometric_slivers(*_BOUNDARY[need])
    sc = B.scene(tri.reshape(-1, 3, 3))
    pose = S.Camera(aspect=1.0).look_at([-0.5, 0.5, 0.4], [float(tri[:, 3].max()) * 0.05, 0.5, 0.0])
    ubo = make_ubo(pose, sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    on, off = _on_off_oracle(renderer, oracle_lib, monkeypatch, f"geometric slivers {len(tri)}", sc, ubo, 64, 64, 2)
    assert off["build"].stack_need == need
    assert off["stack"] == (DEEP_STACK if need >= PT_STACK else PT_STACK, need, need >= PT_STACK)
    assert on["rays"][0] > 64 * 64 * 2  # (some paths hit the strip and go on)
