"""The reinsertion-optimised topology of the megakernel's compact traversal nodes (csrc/bvh_opt.h; the scene
upload's upload_traversal_nodes; ptgs_scene_get_tree_opt).

CPU part: tests/native/tree_opt_check.cpp, a stand-alone program (its own main, host code only: bvh.cpp,
bvh_opt.cpp), built here with g++ -fsanitize=address,undefined and run directly. It builds the canonical tree as the
upload does, calls what the upload calls, and counts violations: the optimised nodes' leaf links are the canonical
ones, each as often; links in range, every node linked once; every interior child box contains its subtree's leaf
boxes; the reported need and depth are what a fresh pass computes and stay below the limit; two runs give identical
bytes; with the limit below any need the optimiser reports "not applied" and the compact nodes are the plain
conversion's bytes; and the lockstep models of the closest-hit and any-hit walks, on the canonical and on the
optimised compact nodes, return the brute-force (t, gid) and occlusion on every seeded ray with no stack write at or
above the walked tree's need. It prints the walks' wave and lane node steps on both trees (pytest -s).

GPU part: the megakernel on the optimised copy against the CPU oracle (which walks its own tree) and against the
same render with PTGS_PT_TREE_OPT=0: images bit for bit, ray counts equal; the query says which copy is walked; the
canonical arrays (ptgs_scene_get_bvh, scene_info, scene_build) do not move."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import scenes_util as U
from pathtracer_gaussiansplatting_amd import make_ubo

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(HERE, "native")


@pytest.fixture(scope="module")
def check_bin():
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out_dir = os.path.join(NATIVE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "tree_opt_check")
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(CSRC, "bvh_opt.cpp"), os.path.join(NATIVE, "tree_opt_check.cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("bvh.h", "bvh_opt.h", "stack_key.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


def _triangles(sc):
    """The scene's triangles in flattening order (api.cpp ptgs_scene_upload), float32 [n, 9]."""
    pos = np.asarray(sc.vertices["pos"], np.float32)
    out = []
    for m, cnt in zip(sc.meshes, sc.mesh_index_count):
        cnt = int(cnt)
        if cnt < 3:
            continue
        idx = np.asarray(sc.indices[int(m["index_offset"]):int(m["index_offset"]) + cnt // 3 * 3], np.int64)
        out.append(pos[idx + int(m["vertex_offset"])].reshape(-1, 9))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


_CACHE = {}


def _scene(name):
    """The test scenes, built once per module (no test changes them)."""
    if name not in _CACHE:
        _CACHE[name] = {"features": U.features, "atrium": U.atrium}[name]()
    return _CACHE[name]


def _one_triangle():
    return np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.5]], np.float32)


def _two_triangles():
    return np.array([[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.5],
                     [2.0, 0.0, 1.0, 3.0, 0.5, 1.0, 2.0, 1.0, 0.0]], np.float32)


def _coincident():
    """Five times the same triangle: every area and every cost ties."""
    return np.repeat(_one_triangle(), 5, axis=0)


def _slivers(n=257):
    """A strip of thin triangles sorted along x (each 1e-3 wide, 1 long, slightly tilted)."""
    x = np.arange(n, dtype=np.float32) * np.float32(1e-3)
    t = np.zeros((n, 9), np.float32)
    t[:, 0], t[:, 3], t[:, 6] = x, x + np.float32(1e-3), x
    t[:, 4] = 1.0
    t[:, 7], t[:, 8] = 1.0, x * np.float32(0.25)
    return t


def _run_check(check_bin, tmp_path, tri, tries, waves, limit=0):
    path = os.path.join(str(tmp_path), "tris.bin")
    np.ascontiguousarray(tri, np.float32).tofile(path)
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([check_bin, path, leaf, fan, depth, str(waves), str(limit)], capture_output=True, text=True,
                       timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                                         "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    return {k: (float(v) if "." in v else int(v)) for k, v in zip(w[1::2], w[2::2])}


def _report(name, st):
    for walk, what in (("c", "closest-hit"), ("a", "any-hit")):
        if st[f"{walk}_node_steps_can"]:
            print(f"{name} {what}: wave node steps {st[f'{walk}_node_steps_opt'] / st[f'{walk}_node_steps_can'] - 1:+.1%}, "
                  f"lane node steps {st[f'{walk}_lane_nodes_opt'] / st[f'{walk}_lane_nodes_can'] - 1:+.1%}, "
                  f"lane triangle tests {st[f'{walk}_lane_tris_opt'] / max(st[f'{walk}_lane_tris_can'], 1) - 1:+.1%}")


def test_empty_tree(check_bin, tmp_path):
    """No triangles: the root no ray reaches is left alone, and every walk misses."""
    st = _run_check(check_bin, tmp_path, np.zeros((0, 9), np.float32), "3:4:38", 4)
    assert st["violations"] == 0 and st["applied"] == 0
    assert st["nodes_opt"] == st["nodes_can"] == 1 and st["hits"] == 0 and st["occluded"] == 0


@pytest.mark.parametrize("name,tri,tries", [("one triangle", _one_triangle, "3:4:38"),
                                            ("two triangles", _two_triangles, "1:4:38"),
                                            ("five coincident triangles", _coincident, "1:4:38"),
                                            ("five coincident triangles, 3 per leaf", _coincident, "3:4:38")])
def test_trees_with_nothing_to_move(check_bin, tmp_path, name, tri, tries):
    """A root of two leaves (nothing to move), and costs that all tie: it ends, is deterministic, and keeps the
    canonical shape (a move needs a strictly lower cost)."""
    st = _run_check(check_bin, tmp_path, tri(), tries, 8)
    assert st["violations"] == 0
    assert st["hits"] > 0
    assert (st["nodes_opt"], st["need_opt"], st["depth_opt"]) == (st["nodes_can"], st["need_can"], st["depth_can"])


@pytest.mark.parametrize("tries", ["1:4:38", "1:2:38"])
def test_sliver_strip_with_the_canonical_need_at_the_limit(check_bin, tmp_path, tries):
    """limit = canonical need + 1: the optimised need may not exceed the canonical one, at this fan-out or a lower
    one, or the canonical nodes are converted (the program checks which, and that the need stays below the limit)."""
    st = _run_check(check_bin, tmp_path, _slivers(), tries, 16, limit=-1)
    assert st["violations"] == 0
    assert st["limit"] == st["need_can"] + 1
    assert st["need_opt"] <= st["need_can"]
    assert st["hits"] > 0
    _report("slivers " + tries, st)


@pytest.mark.parametrize("tries", ["3:4:38", "1:4:38"])
def test_features(check_bin, tmp_path, tries):
    """3- and 1-triangle leaves."""
    st = _run_check(check_bin, tmp_path, _triangles(_scene("features")), tries, 32)
    assert st["violations"] == 0 and st["applied"] == 1
    assert 0 < st["hits"] <= st["rays"] and 0 < st["occluded"] < st["rays"]
    assert 0 < st["c_high_water_opt"] <= st["need_opt"] < st["limit"]
    _report("features " + tries, st)


def test_atrium(check_bin, tmp_path):
    """The C3 mesh: the area sum of the 4-wide nodes falls to at most 0.92 x the canonical sum (a full reinsertion
    pass from the SAH build's own BVH2 reached 0.900; 2% for the binarised start), and the closest-hit walk's wave
    node steps fall on the seeded waves (the gate for taking the tree to the GPU: node steps on rays, not area)."""
    st = _run_check(check_bin, tmp_path, _triangles(_scene("atrium")), "3:4:38", 16)
    assert st["violations"] == 0 and st["applied"] == 1
    assert (st["nodes_can"], st["need_can"], st["depth_can"]) == (58627, 38, 13)
    assert st["need_opt"] < st["limit"] == 39
    print(f"atrium: area sum {st['area_can']:.3f} -> {st['area_opt']:.3f} ({st['area_opt'] / st['area_can']:.4f}), "
          f"{st['ms']:.0f} ms under the sanitizers")
    _report("atrium", st)
    assert st["area_opt"] <= 0.92 * st["area_can"]
    assert st["c_node_steps_opt"] < st["c_node_steps_can"]


def test_query_struct_layout():
    """ptgs_scene_tree_opt (ptgs.h): six uint32, then three doubles at 24, 32 and 40; 48 bytes."""
    import ctypes as C
    from pathtracer_gaussiansplatting_amd._abi import SYMBOLS, SceneTreeOpt
    assert C.sizeof(SceneTreeOpt) == 48
    assert [n for n, _ in SceneTreeOpt._fields_] == ["applied", "num_nodes", "stack_need", "depth", "fan", "passes",
                                                     "area_before", "area_after", "ms"]
    assert (SceneTreeOpt.passes.offset, SceneTreeOpt.area_before.offset, SceneTreeOpt.ms.offset) == (20, 24, 40)
    assert "ptgs_scene_get_tree_opt" in SYMBOLS


# ---------------------------------------------------------------------------------------------------
# GPU: the megakernel on the optimised copy against the oracle and against the canonical copy
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


def _upload_and_render(renderer, monkeypatch, sc, ubo, W, H, spp, opt):
    """(image, extension rays, shadow rays, tree_opt, scene_info, scene_build) of an upload with PTGS_PT_TREE_OPT
    unset (opt None: the upload's own policy), 1 or 0."""
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
    return acc.cpu().numpy(), st.extension_rays, st.shadow_rays, renderer.scene_tree_opt(), renderer.scene_info(), \
        renderer.scene_build()


def _on_off_oracle(renderer, oracle_lib, monkeypatch, key, sc, ubo, W, H, spp, deep=False):
    on = _upload_and_render(renderer, monkeypatch, sc, ubo, W, H, spp, None)
    off = _upload_and_render(renderer, monkeypatch, sc, ubo, W, H, spp, 0)
    o, ext, shd = _oracle(oracle_lib, key, sc, ubo, W, H, spp)
    t_on, t_off = on[3], off[3]
    print(f"{key}: applied {t_on.applied}/{t_off.applied}, nodes {on[4].num_bvh_nodes} -> {t_on.num_nodes}, need "
          f"{on[5].stack_need} -> {t_on.stack_need}, depth {on[4].bvh_depth} -> {t_on.depth}, area sum "
          f"{t_on.area_before:.3f} -> {t_on.area_after:.3f}, {t_on.ms:.1f} ms; "
          f"{int(np.count_nonzero(np.any(on[0] != o, axis=-1)))} pixels differ from the oracle")
    assert t_on.applied == 1 and t_off.applied == 0
    assert t_on.num_nodes > 0 and t_on.passes > 0 and 0 < t_on.area_after and t_on.area_before == t_off.area_before
    # the copy is held to the bound of the canonical tree's kernel instantiation
    assert on[5].deep_stack == off[5].deep_stack == (1 if deep else 0)
    assert t_on.stack_need < (48 if deep else 39)
    # scene_info and scene_build describe the canonical tree either way
    assert (on[4].num_bvh_nodes, on[4].bvh_depth, on[4].max_leaf_size) == \
        (off[4].num_bvh_nodes, off[4].bvh_depth, off[4].max_leaf_size)
    assert (on[5].builder, on[5].leaf, on[5].fan, on[5].stack_need) == (off[5].builder, off[5].leaf, off[5].fan,
                                                                        off[5].stack_need)
    assert ext > 0 and shd > 0
    assert np.array_equal(on[0], o)
    assert (on[1], on[2]) == (ext, shd)
    assert np.array_equal(on[0], off[0])
    assert (on[1], on[2]) == (off[1], off[2])
    return on, off


@pytest.mark.gpu
def test_features_image_and_ray_counts(renderer, oracle_lib, monkeypatch):
    """MASK and BLEND triangles, punctual lights, 3- and 1-triangle leaves."""
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("features")
    ubo = make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    _on_off_oracle(renderer, oracle_lib, monkeypatch, "features 160x120 2spp", sc, ubo, 160, 120, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,spp", [(160, 120, 2), (150, 70, 3)])
def test_atrium_image_and_ray_counts(renderer, oracle_lib, monkeypatch, W, H, spp):
    """The C3 mesh; 150x70 at 3 spp: partial tiles, and an odd sample left over in the lane pair."""
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    on, _ = _on_off_oracle(renderer, oracle_lib, monkeypatch, f"atrium {W}x{H} {spp}spp", sc, ubo, W, H, spp)
    assert on[3].area_after <= 0.92 * on[3].area_before


@pytest.mark.gpu
def test_atrium_deep_instantiation(renderer, oracle_lib, monkeypatch):
    """1-triangle leaves: the canonical tree needs 40 stack entries, so the DEEP instantiation (entries beyond 39 in
    the private overflow) walks the copy, which is held to PTGS_STACK + PTGS_STACK_OVF."""
    monkeypatch.setenv("PTGS_BVH_TRIES", "1:4:38")
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    on, _ = _on_off_oracle(renderer, oracle_lib, monkeypatch, "atrium 160x120 2spp", sc, ubo, 160, 120, 2, deep=True)
    assert on[5].stack_need >= 39


def _bvh_arrays(renderer):
    bb = renderer.bvh_buffers()
    nodes = np.zeros((bb.num_nodes, 32), np.uint32)
    tris = np.zeros((bb.num_triangles, 12), np.uint32)
    renderer.copy_d2h(nodes, bb.nodes, nodes.nbytes)
    renderer.copy_d2h(tris, bb.triangles, tris.nbytes)
    return nodes, tris


@pytest.mark.gpu
def test_gpu_sah_upload_keeps_the_canonical_arrays(renderer, oracle_lib, monkeypatch):
    """PTGS_FLAG_GPU_BVH: the GPU SAH builder's canonical nodes and triangle records are the same words with the
    optimiser on and off (the copy alone is rebuilt, from the nodes read back), and the image is the oracle's. The
    LBVH, whose point is rebuild time, is converted as it is unless PTGS_PT_TREE_OPT=1 asks."""
    from pathtracer_gaussiansplatting_amd import FLAG_GPU_BVH, FLAG_GPU_LBVH
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    renderer.set_flags(FLAG_GPU_BVH)
    try:
        on = _upload_and_render(renderer, monkeypatch, sc, ubo, 160, 120, 2, None)
        nodes_on, tris_on = _bvh_arrays(renderer)
        off = _upload_and_render(renderer, monkeypatch, sc, ubo, 160, 120, 2, 0)
        nodes_off, tris_off = _bvh_arrays(renderer)
        renderer.set_flags(FLAG_GPU_BVH | FLAG_GPU_LBVH)
        lbvh = _upload_and_render(renderer, monkeypatch, sc, ubo, 160, 120, 2, None)
    finally:
        renderer.set_flags(0)
    assert on[5].builder == off[5].builder == 1 and lbvh[5].builder == 2
    assert on[3].applied == 1 and off[3].applied == 0 and lbvh[3].applied == 0
    assert np.array_equal(nodes_on, nodes_off) and np.array_equal(tris_on, tris_off)
    assert nodes_on.shape[0] == on[4].num_bvh_nodes == 58627
    assert on[3].num_nodes != on[4].num_bvh_nodes and on[3].area_after <= 0.92 * on[3].area_before
    o, ext, shd = _oracle(oracle_lib, "atrium 160x120 2spp", sc, ubo, 160, 120, 2)
    for img, e, s in (on[:3], off[:3], lbvh[:3]):
        assert np.array_equal(img, o) and (e, s) == (ext, shd)
