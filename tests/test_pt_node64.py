"""The compact 64-B traversal nodes of the path-tracer megakernel (bvh.h quantize_bvh4, pt_device.h box4_q).

CPU part: tests/native/node64_check.cpp, a stand-alone program (its own main, host code only: bvh.cpp),
built here with g++ -fsanitize=address,undefined. It builds the host tree of a test scene, converts it and
restates the kernel's decode with the same float expressions: every decoded child box contains its
canonical box (unit ray and seeded rays, per axis: near distance not later, far distance not earlier),
empty slots are unhittable, links equal the canonical links. The condition is zero violations.

GPU part: the megakernel (which reads the compact nodes) against the CPU oracle (which walks its own tree):
images bit for bit (np.array_equal), ray counts equal. The DEEP instantiation (stack need >= 39) needs a
tree of C5's size; no test scene builds one in under a second, so it is covered by the existing C5 config
test only."""
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
    out = os.path.join(out_dir, "node64_check")
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(NATIVE, "node64_check.cpp")]
    deps = srcs + [os.path.join(CSRC, "bvh.h")]
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


@pytest.mark.parametrize("name,tries,rays", [("features", "3:4:38", 64), ("atrium", "3:4:38", 8),
                                             ("atrium", "2:4:38", 8)])
def test_decoded_boxes_contain_the_canonical_boxes(check_bin, tmp_path, name, tries, rays):
    """Zero violations, under AddressSanitizer + UndefinedBehaviorSanitizer; the 2:4:38 tree (and any
    tree with two-leaf nodes) has empty slots."""
    tri = _triangles(_scene(name))
    path = os.path.join(str(tmp_path), "tris.bin")
    tri.tofile(path)
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([check_bin, path, leaf, fan, depth, str(rays)], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    stats = dict(zip(w[1::2], map(int, w[2::2])))
    assert stats["violations"] == 0
    assert stats["children"] > 0 and stats["rays"] == stats["nodes"] * rays
    if tries == "2:4:38":
        assert stats["empty"] > 0


# ---------------------------------------------------------------------------------------------------
# GPU: the megakernel on the compact nodes against the oracle
# ---------------------------------------------------------------------------------------------------
def _render_both(renderer, oracle_lib, sc, ubo, W, H, spp):
    import torch
    renderer.set_wavefront(False)
    renderer.upload_scene(sc)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.stats_reset()
    renderer.trace_camera(ubo, W, H, acc, spp=spp)
    torch.cuda.synchronize()
    st = renderer.stats()
    g = acc.cpu().numpy()
    o = np.zeros((H, W, 4), np.float32)
    so = oracle_lib.trace_camera(sc.desc(), ubo, W, H, o, spp=spp)
    ndiff = int(np.count_nonzero(np.any(g != o, axis=-1)))
    print(f"{W}x{H} {spp} spp: {ndiff} pixels differ, ext {st.extension_rays}/{so.extension_rays} "
          f"shadow {st.shadow_rays}/{so.shadow_rays}")
    assert np.array_equal(g, o), f"{ndiff} pixels differ"
    assert (st.extension_rays, st.shadow_rays) == (so.extension_rays, so.shadow_rays)


@pytest.mark.gpu
def test_features_blend_mask_anyhit(renderer, oracle_lib):
    sc = _scene("features")
    ubo = make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    _render_both(renderer, oracle_lib, sc, ubo, 160, 120, 3)


@pytest.mark.gpu
def test_features_textured(renderer, oracle_lib):
    sc = U.features(textured=True)
    ubo = make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    ubo.use_lod = 1.0
    ubo.lod_factor = 0.8
    _render_both(renderer, oracle_lib, sc, ubo, 160, 120, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("tries", [None, "2:4:38"])
def test_atrium(renderer, oracle_lib, tries, monkeypatch):
    """The default tree, and 2-triangle leaves (PTGS_BVH_TRIES=2:4:38: nodes with empty slots)."""
    if tries:
        monkeypatch.setenv("PTGS_BVH_TRIES", tries)
    else:
        monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    _render_both(renderer, oracle_lib, sc, ubo, 160, 90, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("W,H,spp", [(64, 64, 1), (60, 45, 3)])
def test_cornell_tiles(renderer, oracle_lib, W, H, spp):
    """64x64 at 1 spp: 8x8 tiles, no lane pairs; 60x45 at 3 spp: partial tiles, odd spp."""
    sc = U.cornell()
    ubo = make_ubo(U.cornell_pose(W / H), sc, 0)
    _render_both(renderer, oracle_lib, sc, ubo, W, H, spp)
