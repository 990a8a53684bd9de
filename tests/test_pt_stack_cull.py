"""The path-tracer megakernel's packed stack word and its cull at pop (stack_key.h, bvh.h stack_layout /
pack_links64, pt_device.h trace_closest<.., CULL>).

CPU part: tests/native/stack_cull_check.cpp, a stand-alone program (its own main, host code only: bvh.cpp and
stack_key.h, the header the kernel itself packs and unpacks with), built here with
g++ -fsanitize=address,undefined and run directly. For every key width 0 .. 31 it checks
decode(encode(x)) <= x at every binade boundary in [0, 2^15], its neighbours and a few million seeded floats;
every link of the test trees round-trips through the packed form (leaves of 1 to 3 triangles, the empty
tree); one lane of the kernel's walk, restated, gives the same (t, gid) with and without the cull for the
tree's own key width and forced widths 0, 3 and 8, and no culled entry holds a triangle the walk would
still accept. The condition is zero violations. The program prints the share of culled pops and the node
steps with and without the cull (run pytest -s to see them).

GPU part: the megakernel against the CPU oracle (which walks its own tree and never culls): images bit for
bit (np.array_equal), extension and shadow ray counts equal, as built and with the key width forced to 0
(never culls) and to 3 through PTGS_PT_STACK_KEY_BITS, read at upload. The DEEP instantiation (stack need
>= 39, packed words in the private overflow) needs a tree of C5's size; no test scene builds one in under a
second, so it remains covered by the existing C5 config test only."""
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
    out = os.path.join(out_dir, "stack_cull_check")
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(NATIVE, "stack_cull_check.cpp")]
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


def _run_check(check_bin, path, tries, rays, floats):
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([check_bin, path, leaf, fan, depth, str(rays), str(floats)], capture_output=True, text=True,
                       timeout=600, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                                         "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    return dict(zip(w[1::2], map(int, w[2::2])))


# (the float sample runs once, in the first case: 3 million floats x 32 widths)
@pytest.mark.parametrize("name,tries,rays,floats", [("features", "3:4:38", 3000, 3_000_000), ("features", "1:4:38", 1500, 0),
                                                    ("atrium", "3:4:38", 1500, 0), ("atrium", "2:4:38", 1000, 0)])
def test_key_floor_link_round_trip_and_walk(check_bin, tmp_path, name, tries, rays, floats):
    """Zero violations, under AddressSanitizer + UndefinedBehaviorSanitizer."""
    tri = _triangles(_scene(name))
    path = os.path.join(str(tmp_path), "tris.bin")
    tri.tofile(path)
    st = _run_check(check_bin, path, tries, rays, floats)
    assert st["violations"] == 0
    assert st["rays"] == rays and st["links"] == 4 * st["nodes"] and st["floats"] >= floats + 3 * 165
    assert st["link_bits"] + st["key_bits"] == 32  # these trees leave more than the minimum
    assert st["pops"] > 0
    print(f"{name} {tries}: {st['culled'] / st['pops']:.1%} of pops culled, node steps "
          f"{st['steps_cull'] / st['steps_plain'] - 1:+.1%}, triangle tests {st['tris_cull'] / max(st['tris_plain'], 1) - 1:+.1%}")
    # the cull only removes work
    assert st["steps_cull"] <= st["steps_plain"] and st["tris_cull"] <= st["tris_plain"]


def test_empty_tree(check_bin, tmp_path):
    """No triangles: no nodes, a 1-bit link, and the walk misses."""
    path = os.path.join(str(tmp_path), "empty.bin")
    open(path, "wb").close()
    st = _run_check(check_bin, path, "3:4:38", 16, 0)
    assert st["violations"] == 0 and st["nodes"] == 0 and st["link_bits"] == 1


# ---------------------------------------------------------------------------------------------------
# GPU: the culling megakernel against the oracle
# ---------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(oracle_lib, key, sc, ubo, W, H, spp):
    """The oracle's image and ray counts, once per (scene, size, spp): shared by the key-width variants."""
    if key not in _ORACLE:
        o = np.zeros((H, W, 4), np.float32)
        so = oracle_lib.trace_camera(sc.desc(), ubo, W, H, o, spp=spp)
        o.setflags(write=False)
        _ORACLE[key] = (o, so.extension_rays, so.shadow_rays)
    return _ORACLE[key]


def _render_against_oracle(renderer, oracle_lib, key, sc, ubo, W, H, spp):
    import torch
    renderer.set_wavefront(False)
    renderer.upload_scene(sc)  # (reads PTGS_PT_STACK_KEY_BITS)
    acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    renderer.stats_reset()
    renderer.trace_camera(ubo, W, H, acc, spp=spp)
    torch.cuda.synchronize()
    st = renderer.stats()
    g = acc.cpu().numpy()
    o, ext, shd = _oracle(oracle_lib, key, sc, ubo, W, H, spp)
    ndiff = int(np.count_nonzero(np.any(g != o, axis=-1)))
    print(f"{key}: {ndiff} pixels differ, ext {st.extension_rays}/{ext} shadow {st.shadow_rays}/{shd}")
    assert np.array_equal(g, o), f"{ndiff} pixels differ"
    assert (st.extension_rays, st.shadow_rays) == (ext, shd)


def _force(monkeypatch, bits):
    if bits is None:
        monkeypatch.delenv("PTGS_PT_STACK_KEY_BITS", raising=False)
    else:
        monkeypatch.setenv("PTGS_PT_STACK_KEY_BITS", str(bits))


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [None, 0, 3])
def test_features_image_and_ray_counts(renderer, oracle_lib, bits, monkeypatch):
    """Transparent (blend, mask), punctual and emissive lights; 96x64 at 4 spp (two lanes per pixel)."""
    _force(monkeypatch, bits)
    sc = _scene("features")
    ubo = make_ubo(U.cornell_pose(96 / 64), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0))
    _render_against_oracle(renderer, oracle_lib, "features 96x64 4spp", sc, ubo, 96, 64, 4)


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [None, 0, 3])
def test_atrium_image_and_ray_counts(renderer, oracle_lib, bits, monkeypatch):
    _force(monkeypatch, bits)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    _render_against_oracle(renderer, oracle_lib, "atrium 96x64 4spp", sc, ubo, 96, 64, 4)


@pytest.mark.gpu
def test_atrium_one_sample_per_pixel(renderer, oracle_lib, monkeypatch):
    """spp = 1: the unpaired lane layout (8x8 tiles, one lane per pixel)."""
    _force(monkeypatch, None)
    sc = _scene("atrium")
    ubo = make_ubo(U.atrium_pose(), sc, 0, ambient=(0.3, 0.4, 0.5, 1.0))
    _render_against_oracle(renderer, oracle_lib, "atrium 96x64 1spp", sc, ubo, 96, 64, 1)
