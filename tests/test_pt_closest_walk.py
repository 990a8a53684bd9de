"""The node step of the path tracer's closest-hit walk (pt_device.h trace_closest: the two-site walk that ships, with
the node loop's test as one unsigned compare; forms b1 and b2 with one pop site instead of two:
tools/patches/pt_one_pop_rejected.patch; the slab distances as two-element FMAs in box4_q:
tools/patches/pt_pk_slab_rejected.patch).

CPU part: tests/native/closest_walk_check.cpp, a stand-alone program (its own main, host code only: bvh.cpp, bvh.h
and stack_key.h), built here with g++ -fsanitize=address,undefined and run directly. It models a wave of 64 lanes
in lockstep, with the packed stack words and the cull at pop, for the walk with two pop sites, for the one-site walk
that parks a popped leaf and pops again (form b1) and for the one-site walk that pops once (form b2), on seeded
rays (general directions, one axis-parallel component, origins outside the bounds) in waves of 1 to 64 active
lanes. The condition is zero violations: every walk returns the brute-force closest (t, gid) on every ray, no stack
write at or above the tree's stack need, no write by a lane outside the node loop, and form b1's per-lane
sequence of visited nodes and leaves equals the two-site walk's. The program prints the modelled wave and lane node
steps of the three walks (run pytest -s to see them).

GPU part: the megakernel against the CPU oracle (which walks its own tree): images bit for bit (np.array_equal),
extension and shadow ray counts equal. It runs the library as built (the unsigned loop test in both walks; a
library built with one of the two patches runs that form: the one-site forms and the packed FMAs measured no
gain, profiles/r10_summary.md, where their images on the C3 frame are compared bit for bit with the
two-site walk's). A slab distance that rounded differently, or a lane that left the node loop on the wrong word,
would move the visited boxes or lose a leaf; the image must not notice, the ray counts neither. The DEEP
instantiation (stack need >= 39, entries in the private overflow) needs a tree of C5's size; no test scene builds
one in under a second, so it stays covered by the existing C5 config test and by the C5 row of the A/B table
(profiles/r10_summary.md: image identical)."""
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
    out = os.path.join(out_dir, "closest_walk_check")
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(NATIVE, "closest_walk_check.cpp")]
    deps = srcs + [os.path.join(CSRC, "bvh.h"), os.path.join(CSRC, "stack_key.h")]
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


def _run_check(check_bin, path, tries, waves):
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([check_bin, path, leaf, fan, depth, str(waves)], capture_output=True, text=True,
                       timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                                         "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    return dict(zip(w[1::2], map(int, w[2::2])))


@pytest.mark.parametrize("name,tries,waves", [("features", "3:4:38", 64), ("features", "1:4:38", 64),
                                              ("atrium", "3:4:38", 16), ("atrium", "2:4:38", 16)])
def test_walks_find_the_closest_hit_and_stay_in_the_stack(check_bin, tmp_path, name, tries, waves):
    """Zero violations, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    tri = _triangles(_scene(name))
    path = os.path.join(str(tmp_path), "tris.bin")
    tri.tofile(path)
    st = _run_check(check_bin, path, tries, waves)
    assert st["violations"] == 0
    assert st["waves"] == waves and waves <= st["rays"] <= 64 * waves
    assert 0 < st["hits"] <= st["rays"]
    assert 0 < st["high_water"] <= st["need"]
    assert st["key_bits"] > 0 and st["culled_old"] > 0  # the cull at pop is part of what is modelled
    # ONE_POP=1 is the two-site walk, lane by lane: the same visits in the same order, so the same counts
    assert st["seq_diff_b1"] == 0
    for k in ("node_steps", "lane_nodes", "leaf_phases", "lane_leaves", "pops", "culled"):
        assert st[k + "_b1"] == st[k + "_old"], k
    for v in ("b1", "b2"):
        print(f"{name} {tries} {v}: wave node steps {st['node_steps_' + v] / st['node_steps_old'] - 1:+.1%}, "
              f"lane node steps {st['lane_nodes_' + v] / st['lane_nodes_old'] - 1:+.1%}, "
              f"leaf phases {st['leaf_phases_' + v] / st['leaf_phases_old'] - 1:+.1%}")


def test_empty_tree(check_bin, tmp_path):
    """No triangles: no nodes, and every walk misses."""
    path = os.path.join(str(tmp_path), "empty.bin")
    open(path, "wb").close()
    st = _run_check(check_bin, path, "3:4:38", 4)
    assert st["violations"] == 0 and st["nodes"] == 0 and st["hits"] == 0 and st["high_water"] == 0
    assert st["node_steps_old"] == st["node_steps_b1"] == st["node_steps_b2"] == 0


# ---------------------------------------------------------------------------------------------------
# GPU: the megakernel against the oracle
# ---------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(oracle_lib, key, sc, ubo, W, H, spp):
    """The oracle's image and ray counts, once per (scene, size, spp): shared by the tree variants."""
    if key not in _ORACLE:
        o = np.zeros((H, W, 4), np.float32)
        so = oracle_lib.trace_camera(sc.desc(), ubo, W, H, o, spp=spp)
        o.setflags(write=False)
        _ORACLE[key] = (o, so.extension_rays, so.shadow_rays)
    return _ORACLE[key]


def _render_against_oracle(renderer, oracle_lib, key, sc, ubo, W, H, spp):
    import torch
    renderer.set_wavefront(False)
    renderer.upload_scene(sc)  # (reads PTGS_BVH_TRIES)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.stats_reset()
    renderer.trace_camera(ubo, W, H, acc, spp=spp)
    torch.cuda.synchronize()
    st = renderer.stats()
    g = acc.cpu().numpy()
    o, ext, shd = _oracle(oracle_lib, key, sc, ubo, W, H, spp)
    ndiff = int(np.count_nonzero(np.any(g != o, axis=-1)))
    print(f"{key}: {ndiff} pixels differ, ext {st.extension_rays}/{ext} shadow {st.shadow_rays}/{shd}")
    assert ext > 0 and shd > 0
    assert np.array_equal(g, o), f"{ndiff} pixels differ"
    assert (st.extension_rays, st.shadow_rays) == (ext, shd)


def _atrium(renderer, oracle_lib, monkeypatch, W, H, spp, tries=None):
    if tries:
        monkeypatch.setenv("PTGS_BVH_TRIES", tries)
    else:
        monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    _render_against_oracle(renderer, oracle_lib, f"atrium {W}x{H} {spp}spp", sc, ubo, W, H, spp)


@pytest.mark.gpu
def test_features_image_and_ray_counts(renderer, oracle_lib, monkeypatch):
    """MASK and BLEND triangles (the any-hit decision inside the closest-hit leaf), punctual lights."""
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    sc = _scene("features")
    ubo = make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    _render_against_oracle(renderer, oracle_lib, "features 160x120 2spp", sc, ubo, 160, 120, 2)


@pytest.mark.gpu
def test_atrium_two_samples(renderer, oracle_lib, monkeypatch):
    _atrium(renderer, oracle_lib, monkeypatch, 160, 120, 2)


@pytest.mark.gpu
def test_atrium_one_sample_per_pixel(renderer, oracle_lib, monkeypatch):
    """spp = 1: the unpaired lane layout (8x8 tiles, one lane per pixel)."""
    _atrium(renderer, oracle_lib, monkeypatch, 160, 120, 1)


@pytest.mark.gpu
def test_atrium_partial_tiles_odd_samples(renderer, oracle_lib, monkeypatch):
    """150x70 at 3 spp: partial tiles, and an odd sample left over in the lane pair."""
    _atrium(renderer, oracle_lib, monkeypatch, 150, 70, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("tries", ["2:4:38", "1:4:38"])
def test_atrium_other_trees(renderer, oracle_lib, tries, monkeypatch):
    """2-triangle leaves (nodes with empty child slots) and 1-triangle leaves (many leaves: a lane parks one at
    nearly every step, and the popped word is often a leaf too)."""
    _atrium(renderer, oracle_lib, monkeypatch, 160, 120, 2, tries)
