"""The kernels that walk the canonical 4-wide tree, and the counting instantiations of both path tracers: the
wavefront tracer's extend and shadow kernels (pt_wavefront.hip: TravStack<39> and TravStack<25>, the shadow
kernel's own any-hit walk), the DEEP instantiations of pt_depth_kernel, pt_torus_kernel and pt_camera_kernel
(DevScene::deep_stack / pt_deep_stack), the STATS = true copies that PTGS_FLAG_COUNT_TRAVERSAL selects, and the
wavefront host code's four tuning variables.

Every comparison is np.array_equal on images and == on integer counts. There is no tolerance in this file.

A. Strips of thin triangles (bvh_soups.geometric_slivers) uploaded with PTGS_BVH_TRIES=1:4:38, whose canonical
   stack need sits at the kernels' LDS depths. _STRIPS holds them: the lengths are tree_budget_check's need_greedy
   (test_strip_lengths re-derives them on the CPU), the GPU tests assert scene_build().stack_need. A worst-case
   need says nothing about the rays of one render, so the file carries a float64 model of the stack pointer
   (stack_high_water) of both walks on the nodes read back from the device, evaluated on the un-jittered primary rays
   through every pixel's centre and corners; each case asserts how many pixels the model puts strictly above each
   LDS depth, so a change of scene cannot quietly stop exercising the overflow.
   What the model found ("Tests of the canonical walkers"):
     - the closest-hit walk of a primary ray cannot pass 38 on any strip of the issue's table, whatever the
       camera: the ray's tmax is 1e4 and the strip of need 40 is 2.2e4 long, so the root's two far leaves are never
       pushed (need - 2); the strips of need 46 and 47 are longer still. Those cases carry no condition for the
       extend walk and the megakernel (None in _STRIPS). A strip that starts at 1e-9 instead of 1e-5 (86 triangles,
       ratio 1.4, need 45) is 3.7e3 long: a long-lens camera at its narrow end puts 2048 pixels above 39.
     - the shadow ray starts 0.001 above the surface (pt_device.h sample_punctual), outside the boxes of the
       triangles narrower than about 0.004: on the table's strips of need 24, 25 and 26 no surface point reaches
       above 14. Strips that start at 0.01 (ratio 1.5: 29 triangles need 25, 30 triangles need 26) bracket the shadow
       kernel's 25 entries instead: need 25 fills the LDS part to its last entry, need 26 uses the first overflow
       entry in 224 pixels.
B. The wavefront tracer on the degenerate triangle sets of bvh_soups.py (test_bvh_build_gpu.py's check for the
   megakernel, with its ambient, pose and oracle images).
C. PTGS_FLAG_COUNT_TRAVERSAL: flag off counts nothing; flag on renders the same image; closest_hits agree between the
   tracers; lower bounds in the unit both tracers count a node step in (4 child-box tests: `nodes += 4`); an all-miss
   render and a one-node scene where node_visits is exact; accumulation, reset, determinism, row additivity, torus.
D. PTGS_WF_TRACE_RUN / SHADE_RUN / REFILL / BATCH, one fresh process per setting (tests/wf_knobs_child.py).

The reviewer's two mutations (not run on the GPU): `sp - N + 1` in TravStack::push or pop_nz loses the entry at index
N and repeats the ones above it, in both instantiations of the template. test_strip_renders' comparison with the
oracle catches it in the shadow kernel, where the model proves the overflow is used: at "wide26" (need 26) and at need
38, 39, 40 and 47. An emulation of both mutants on the model's shadow rays (this file's walk with the shifted index,
while the cases were chosen) changed the outcome of 57 of 282 sampled deep rays at "wide26" and of every sampled deep
ray at need 38, 40 and 47. The same emulation of the extend walk at "deep45" changed no hit of 200 sampled rays, all
of which pass 39: the lost entry is a leaf the ray misses. What "deep45" pins in the extend kernel and the DEEP
megakernel is that entries 39 to 44 are stored and read back per lane (a wrong stride or column would mix lanes).
`tc.nodes += 0` in a STATS instantiation fails test_one_node_scene_counts_exactly (node_visits == 4 * rays) for
whichever walk lost its count, and test_all_miss_render_counts_one_root_step_per_ray for a closest-hit walk."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import bvh_soups as B
import scenes_util as U
from pathtracer_gaussiansplatting_amd import (FLAG_COUNT_TRAVERSAL, HITDATA_DTYPE, PUNCTUAL_LIGHT_DTYPE, make_ubo,
                                              torus_push)
from pathtracer_gaussiansplatting_amd import scene as S
from pathtracer_gaussiansplatting_amd import synthetic as Y

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc")
NATIVE = os.path.join(HERE, "native")

PT_STACK = 30        # pt_device.h PTGS_PT_STACK: the plain megakernel's LDS entries
DEEP_STACK = 39      # pt_device.h PTGS_STACK: the DEEP instantiations', and the extend kernel's (PTGS_WF_LDS_EXT)
SHADOW_STACK = 25    # pt_wavefront.hip PTGS_WF_LDS_SHADOW
STACK_TOTAL = 48     # pt_device.h PTGS_STACK_TOTAL
NODE_STEP = 4        # pt_device.h / pt_wavefront.hip `nodes += 4`: a node step counts its four child-box tests
TRIES = "1:4:38"
AMBIENT = (0.3, 0.4, 0.5, 1.0)
W = H = 64
SPP = 2

# name: (need, triangles, ratio, first width, camera, pixels the model must put above 25 in the shadow walk,
#        pixels above 39 in the closest-hit walk). Cameras: "view" is test_launch_rule_at_its_boundary's, along the
# strip from above its narrow end; "tip" looks down at the first triangle, so that the shadow rays start where the
# chain is deepest; "along" is a long lens at the narrow end looking along the strip, so that the primary rays cross
# every box. None: no condition, because the need is below that depth + 1 (no walk can get there) or because the
# model reaches no pixel with any camera (the reason stands beside the case, and in the module docstring).
_STRIPS = {
    "need24": (24, 45, 1.3, 1e-5, "view", None, None),
    "need25": (25, 46, 1.3, 1e-5, "view", None, None),
    "need26": (26, 37, 1.5, 1e-5, "view", None, None),  # shadow: its rays start outside the narrow boxes, at most 14
    "need37": (37, 73, 1.3, 1e-5, "view", None, None),  # shadow: at most 26, from points on four triangles
    "need38": (38, 53, 1.5, 1e-5, "tip", 32, None),
    "need39": (39, 62, 1.4, 1e-5, "tip", 32, None),
    "need40": (40, 64, 1.4, 1e-5, "tip", 32, None),     # closest: 2.2e4 long, a primary ray ends at 1e4, at most 38
    "need47": (47, 50, 1.8, 1e-5, "tip", 32, None),     # the deepest that fits 1:4:38; closest: 5.8e7 long
    "wide25": (25, 29, 1.5, 1e-2, "tip", None, None),   # fills the shadow kernel's LDS part to its last entry
    "wide26": (26, 30, 1.5, 1e-2, "tip", 32, None),     # and uses its first overflow entry
    "deep45": (45, 86, 1.4, 1e-9, "along", None, 32),   # 3.7e3 long: the extend walk's and the DEEP megakernel's
                                                        # overflow (its shadow rays, back from far hits, reach 23)
}


def _strip_triangles(name):
    _, n, ratio, first, _, _, _ = _STRIPS[name]
    return B.geometric_slivers(n, ratio, first)


_LIGHT_SLOPE = 0.2


def _strip_light(name, tri):
    """One point light. "view" and "tip": above the strip's wide end, on the line of slope 0.2 through the narrow
    end, so that the shadow ray of a hit near the narrow end stays between the boxes' floors and roofs (roof 0.25 x)
    all the way along the strip, and both outcomes occur (the high side of a later triangle occludes some). "along": its rays meet the tilted triangles from below, hundreds of units along the
    strip, so the light sits below the narrow end and the shadow rays come back through the boxes. The intensity
    undoes the inverse-square falloff at that distance, so the light shows in the image."""
    xmax = float(tri[:, 3].max())
    light = np.zeros(1, PUNCTUAL_LIGHT_DTYPE)
    if _STRIPS[name][4] == "along":
        light["position"], light["intensity"] = [-0.5, 0.5, -0.1], 1.0e6
    else:
        light["position"], light["intensity"] = [xmax, 0.5, _LIGHT_SLOPE * xmax], max(xmax * xmax, 1.0)
    light["color"] = [1.0, 0.9, 0.8]
    light["type"] = 0
    return light


def _strip_pose(name, tri):
    kind = _STRIPS[name][4]
    xmax = float(tri[:, 3].max())
    if kind == "view":
        return S.Camera(aspect=1.0).look_at([-0.5, 0.5, 0.4], [xmax * 0.05, 0.5, 0.0])
    if kind == "along":
        # through the strip's first corner, rising 0.05 per unit (below the roofs, above the low side of the
        # surface), drifting from y = 0.05 to the high side, where it meets the surface after some 700 units
        eye = np.array([-0.012, 0.05, -0.012 * 0.05])
        return S.Camera(aspect=1.0, fov_deg=0.01).look_at(eye, eye + np.array([1.0, 0.9 / min(xmax, 9000.0), 0.05]))
    w = float(tri[0, 3] - tri[0, 0])  # the first triangle's width
    at = np.array([float(tri[0, 0]) + 0.2 * w, 0.7, 0.0])
    dist = max(10.0 * w, 0.02)
    fov = float(np.degrees(2.0 * w / (0.64 * dist)))  # (two triangle widths across the image)
    return S.Camera(aspect=1.0, fov_deg=fov).look_at(at + np.array([-0.5 * dist, 0.0, 0.4 * dist]), at)


_SCENES = {}


def _strip_scene(name):
    """(scene, pose, ubo, triangles [n, 9]) of a strip, built once."""
    if name not in _SCENES:
        tri = _strip_triangles(name)
        sc = B.scene(tri.reshape(-1, 3, 3), lights=[_strip_light(name, tri)[0]])
        assert len(sc.punctual_lights) == 1
        pose = _strip_pose(name, tri)
        _SCENES[name] = (sc, pose, make_ubo(pose, sc, 0, ambient=AMBIENT), tri)
    return _SCENES[name]


# ---------------------------------------------------------------------------------------------------
# the stack model (numpy, float64) on the 4-wide nodes and triangle records of ptgs_scene_get_bvh
# ---------------------------------------------------------------------------------------------------
_K = float(np.float32(1.0000004))  # pt_device.h box4: hit when tn <= tf * 1.0000004f


def _tri_hits(o, d, v0, e1, e2, tmin, tmax):
    """pt_device.h leaf_any's predicate in float64; broadcasts rays against triangles: (hit, t)."""
    pvec = np.cross(d, e2)
    det = np.sum(e1 * pvec, -1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        tvec = o - v0
        u = np.sum(tvec * pvec, -1) * inv
        qvec = np.cross(tvec, e1)
        v = np.sum(d * qvec, -1) * inv
        t = np.sum(e2 * qvec, -1) * inv
        hit = (det != 0.0) & ~(u < 0.0) & ~(u > 1.0) & ~(v < 0.0) & ~(u + v > 1.0) & (t >= tmin) & (t <= tmax)
    return hit, t


def _records(recs):
    r = np.asarray(recs, np.uint32).view(np.float32).reshape(-1, 12).astype(np.float64)
    return r[:, 0:3], r[:, 4:7], r[:, 8:11]  # v0, e1, e2 (bvh.h)


def closest_t(recs, o, d, tmin, tmax):
    """Brute force over every triangle record: (closest hit distance or tmax, hit, its record) per ray."""
    v0, e1, e2 = _records(recs)
    hit, t = _tri_hits(o[:, None, :], d[:, None, :], v0[None], e1[None], e2[None], tmin, tmax)
    t = np.where(hit, t, np.inf)
    which = t.argmin(axis=1)
    t = t.min(axis=1)
    return np.where(np.isfinite(t), t, tmax), np.isfinite(t), which


def stack_high_water(nodes, recs, o, d, tmin, tmax, walk):
    """The highest stack pointer of each ray's walk (layout: bvh_soups.tree_violations).
    "any":     pt_wf_shadow_kernel's walk: box tests capped by tmax; the first hit slot is entered, the other hit
               slots are pushed in slot order; a leaf with an accepted triangle ends the walk, any other leaf pops.
    "closest": enter_box4's order (the extend kernel, trace_closest): the nearest hit child is entered, the others are
               pushed farthest first. tmax holds the ray's final hit distance and caps the box tests from the first
               node on, where the kernel's cap shrinks only as hits are found: the model's walk visits a subset of
               the kernel's nodes in the kernel's order, so its stack pointer is a lower bound on the kernel's."""
    nodes = np.asarray(nodes, np.uint32)
    f = nodes[:, :24].view(np.float32).reshape(len(nodes), 6, 4).astype(np.float64)
    link = nodes[:, 24:28].view(np.int32).astype(np.int64)
    v0, e1, e2 = _records(recs)
    n = len(o)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    tmax = np.broadcast_to(np.asarray(tmax, np.float64), (n,)).copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        oinv = o * inv
    node, sp, high = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    stack = np.zeros((n, 3 * len(f) + 4), np.int64)
    active = np.ones(n, bool)

    def pop(rows):
        empty = sp[rows] == 0
        active[rows[empty]] = False
        rows = rows[~empty]
        sp[rows] -= 1
        node[rows] = stack[rows, sp[rows]]

    while active.any():
        idx = np.flatnonzero(active)
        inner = node[idx] >= 0
        ii = idx[inner]
        if len(ii):
            b = f[node[ii]]  # [k, 6, 4]
            with np.errstate(invalid="ignore"):  # (0 * inf: fmin / fmax drop the NaN, as the kernel's do)
                t0 = b[:, 0::2, :] * inv[ii][:, :, None] - oinv[ii][:, :, None]
                t1 = b[:, 1::2, :] * inv[ii][:, :, None] - oinv[ii][:, :, None]
                lo, hi = np.fmin(t0, t1), np.fmax(t0, t1)
                tn = np.fmax(np.fmax(lo[:, 0], lo[:, 1]), np.fmax(lo[:, 2], tmin))
                tf = np.fmin(np.fmin(hi[:, 0], hi[:, 1]), np.fmin(hi[:, 2], tmax[ii][:, None]))
                hit = tn <= tf * _K
            ln = link[node[ii]]
            nh = hit.sum(axis=1)
            if walk == "closest":
                order, pushes = np.argsort(np.where(hit, tn, np.inf), axis=1, kind="stable"), (3, 2, 1)
            else:
                order, pushes = np.argsort(~hit, axis=1, kind="stable"), (1, 2, 3)
            for p in pushes:
                m = nh > p
                rows = ii[m]
                stack[rows, sp[rows]] = ln[m, order[m, p]]
                sp[rows] += 1
            high[ii] = np.maximum(high[ii], sp[ii])
            some = nh > 0
            node[ii[some]] = ln[some, order[some, 0]]
            pop(ii[~some])
        li = idx[~inner]
        if len(li):
            if walk == "any":
                leaf = ~node[li]
                first, count = leaf & 0x07FFFFFF, (leaf >> 27) + 1
                occ = np.zeros(len(li), bool)
                for k in range(int(count.max())):
                    t = np.minimum(first + k, len(v0) - 1)
                    occ |= _tri_hits(o[li], d[li], v0[t], e1[t], e2[t], tmin, tmax[li])[0] & (k < count)
                active[li[occ]] = False
                li = li[~occ]
            pop(li)
    return high


def camera_rays(pose, w, h):
    """pt_device.h primary_ray without its jitter: the rays through every pixel's centre and four corners,
    (origins, directions) [h * w * 5, 3] in float64, the five rays of a pixel adjacent."""
    iv = np.linalg.inv(np.asarray(pose.view, np.float64).reshape(4, 4).T)
    ip = np.linalg.inv(np.asarray(pose.proj, np.float64).reshape(4, 4).T)
    y, x = np.mgrid[0:h, 0:w]
    offs = np.array([[0.5, 0.5], [0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0]])
    ux = (x.reshape(-1, 1) + offs[None, :, 0]) / w * 2.0 - 1.0
    uy = (y.reshape(-1, 1) + offs[None, :, 1]) / h * 2.0 - 1.0
    tgt = np.stack([ux, uy, np.ones_like(ux), np.ones_like(ux)], -1) @ ip.T
    dc = tgt[..., :3] / tgt[..., 3:4]
    dc /= np.linalg.norm(dc, axis=-1, keepdims=True)
    d = dc @ iv[:3, :3].T
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    return np.broadcast_to(iv[:3, 3], d.shape).reshape(-1, 3).copy(), d.reshape(-1, 3)


def model_pixels(name, nodes, recs):
    """(pixels whose five shadow segments all reach a stack pointer above 25, pixels whose five primary rays all
    reach above 39, and above 30, the highest of the pixels' lowest pointers in the two walks) for a strip's camera
    and light. The shadow
    segments run from the primary rays' surface points, lifted 0.001 along the triangle's normal as sample_punctual
    lifts them, to the light, over [0.001, distance - 0.005]."""
    sc, pose, _, tri = _strip_scene(name)
    o, d = camera_rays(pose, W, H)
    t, hit, which = closest_t(recs, o, d, 0.001, 10000.0)
    hc = stack_high_water(nodes, recs, o, d, 0.001, t, "closest").reshape(-1, 5).min(axis=1)
    _, e1, e2 = _records(recs)
    nrm = np.cross(e1[which], e2[which])
    nrm /= np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-300)
    nrm *= np.where(np.sum(nrm * d, axis=1) > 0.0, -1.0, 1.0)[:, None]  # (facing the viewer)
    so = o + d * t[:, None] + nrm * 0.001
    to = np.asarray(sc.punctual_lights["position"][0], np.float64) - so
    dist = np.linalg.norm(to, axis=1)
    ha = stack_high_water(nodes, recs, so, to / dist[:, None], 0.001, dist - 0.005, "any")
    ha = np.where(hit, ha, 0).reshape(-1, 5).min(axis=1)
    return {"shadow>25": int((ha > SHADOW_STACK).sum()), "closest>39": int((hc > DEEP_STACK).sum()),
            "closest>30": int((hc > PT_STACK).sum()), "shadow max": int(ha.max()), "closest max": int(hc.max())}


def _check_model(name, nodes, recs):
    _, _, _, _, _, px_shadow, px_closest = _STRIPS[name]
    m = model_pixels(name, nodes, recs)
    if px_shadow is not None:
        assert m["shadow>25"] >= px_shadow, (name, m)
    if px_closest is not None:
        assert m["closest>39"] >= px_closest, (name, m)
    if name == "wide25":
        assert m["shadow max"] == SHADOW_STACK, m  # (the LDS part's last entry, index 24, is written)
    return m


# ---------------------------------------------------------------------------------------------------
# CPU: the strips' lengths and the model on the host-built tree
# ---------------------------------------------------------------------------------------------------
def _native(name, extra_srcs=()):
    if not shutil.which("g++"):
        pytest.skip("g++ not available")
    out_dir = os.path.join(NATIVE, "_build")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, name + "_walks")
    srcs = [os.path.join(CSRC, "bvh.cpp")] + [os.path.join(CSRC, s) for s in extra_srcs] + [os.path.join(NATIVE, name + ".cpp")]
    deps = srcs + [os.path.join(CSRC, h) for h in ("bvh.h", "bvh_opt.h", "stack_key.h")]
    if not os.path.exists(out) or any(os.path.getmtime(x) > os.path.getmtime(out) for x in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.fixture(scope="module")
def budget_check():
    return _native("tree_budget_check", ("bvh_opt.cpp",))


@pytest.fixture(scope="module")
def tree_dump():
    return _native("canonical_tree_dump")


def _run_native(binary, args):
    r = subprocess.run([binary] + [str(a) for a in args], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    return dict(zip(w[1::2], map(int, w[2::2])))


@pytest.mark.parametrize("name", sorted(_STRIPS))
def test_strip_lengths(budget_check, tree_dump, tmp_path, name):
    """tree_budget_check's need_greedy of every strip is the need _STRIPS says, below PTGS_STACK_TOTAL; and the model
    on the host-built canonical tree (canonical_tree_dump: build_bvh + collapse_bvh4, the upload's host path) meets
    the case's thresholds without a GPU."""
    need = _STRIPS[name][0]
    tri = _strip_triangles(name)
    assert len(tri) < 100
    path = os.path.join(str(tmp_path), "tris.bin")
    tri.tofile(path)
    leaf, fan, depth = TRIES.split(":")
    st = _run_native(budget_check, [path, leaf, fan, depth])
    assert st["violations"] == 0 and st["need_greedy"] == need < STACK_TOTAL
    npath, rpath = os.path.join(str(tmp_path), "nodes.bin"), os.path.join(str(tmp_path), "recs.bin")
    dump = _run_native(tree_dump, [path, leaf, fan, depth, npath, rpath])
    assert dump["need"] == need
    nodes = np.fromfile(npath, np.uint32).reshape(-1, 32)
    recs = np.fromfile(rpath, np.uint32).reshape(-1, 12)
    assert len(nodes) == dump["nodes"] and B.tree_violations(nodes, recs, tri.reshape(-1, 3, 3), 1, 4) == []
    m = _check_model(name, nodes, recs)
    print(f"{name}: need {need}, {len(tri)} triangles, model {m}")


def test_model_on_a_known_tree():
    """The model itself, on a hand-made tree: one root whose four leaves a ray along x crosses in order. The
    closest-hit walk enters the nearest and holds three entries; capped in front of the third box it holds one; the
    any-hit walk ends at the first triangle it hits with its three pushes made; a ray that misses every box holds
    none."""
    tri = np.zeros((4, 3, 3), np.float32)
    for k in range(4):
        tri[k] = [[k + 0.5, -1.0, -1.0], [k + 0.5, 1.0, -1.0], [k + 0.5, 0.0, 1.0]]
    nodes = np.zeros((1, 32), np.uint32)
    f = nodes[:, :24].view(np.float32).reshape(1, 6, 4)
    for k in range(4):
        f[0, :, k] = [k, k + 1.0, -1.0, 1.0, -1.0, 1.0]
        nodes[0, 24 + k] = np.uint32(~np.int64(k) & 0xFFFFFFFF)  # leaf of one triangle
    recs = np.zeros((4, 12), np.float32)
    recs[:, 0:3], recs[:, 4:7], recs[:, 8:11] = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    recs = recs.view(np.uint32)
    o = np.array([[-1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [-1.0, 5.0, 0.0]])
    d = np.array([[1.0, 0.0, 0.0]] * 3)
    t, hit, which = closest_t(recs, o, d, 0.001, 100.0)
    assert hit.tolist() == [True, True, False] and np.allclose(t[:2], 1.5) and which[:2].tolist() == [0, 0]
    assert stack_high_water(nodes, recs, o, d, 0.001, 100.0, "closest").tolist() == [3, 3, 0]
    assert stack_high_water(nodes, recs, o, d, 0.001, [2.5, 100.0, 100.0], "closest").tolist() == [1, 3, 0]
    assert stack_high_water(nodes, recs, o, d, 0.001, 100.0, "any").tolist() == [3, 3, 0]


# ---------------------------------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle(oracle_lib, key, sc, ubo, w, h, spp, init=None):
    """The oracle's image and (extension, shadow, samples) counts, once per (scene, size, spp)."""
    if key not in _ORACLE:
        o = np.zeros((h, w, 4), np.float32) if init is None else init.copy()
        so = oracle_lib.trace_camera(sc.desc(), ubo, w, h, o, spp=spp)
        o.setflags(write=False)
        _ORACLE[key] = (o, (so.extension_rays, so.shadow_rays, so.samples))
    return _ORACLE[key]


def _counters(st):
    return (st.extension_rays, st.shadow_rays, st.samples, st.node_visits, st.tri_tests, st.closest_hits)


def _trace(renderer, ubo, w, h, spp, wavefront, flags=0, rows=None, reset=True, init=None):
    """One trace_camera on the resident scene: (image, the six counters)."""
    import torch
    renderer.set_wavefront(wavefront)
    renderer.set_flags(flags)
    try:
        acc = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        if init is not None:
            acc.copy_(torch.from_numpy(init))
        if reset:
            renderer.stats_reset()
        renderer.trace_camera(ubo, w, h, acc, spp=spp, rows=rows)
        torch.cuda.synchronize()
        st = renderer.stats()
    finally:
        renderer.set_wavefront(False)
        renderer.set_flags(0)
    return acc.cpu().numpy(), _counters(st)


def _bvh_arrays(renderer):
    bb = renderer.bvh_buffers()
    nodes = np.zeros((bb.num_nodes, 32), np.uint32)
    recs = np.zeros((bb.num_triangles, 12), np.uint32)
    renderer.copy_d2h(nodes, bb.nodes, nodes.nbytes)
    renderer.copy_d2h(recs, bb.triangles, recs.nbytes)
    return nodes, recs


def _upload_strip(renderer, monkeypatch, name):
    """The strip with 1-triangle leaves, its canonical nodes converted as they are for the megakernel."""
    monkeypatch.setenv("PTGS_BVH_TRIES", TRIES)
    monkeypatch.setenv("PTGS_PT_TREE_OPT", "0")
    sc, pose, ubo, tri = _strip_scene(name)
    renderer.set_wavefront(False)
    renderer.set_flags(0)
    renderer.upload_scene(sc)
    need = _STRIPS[name][0]
    b = renderer.scene_build()
    assert b.stack_need == need and b.deep_stack == (need >= DEEP_STACK)
    assert (b.leaf, b.fan, b.depth_budget) == (1, 4, 38)
    return sc, ubo, tri


# ---------------------------------------------------------------------------------------------------
# A. strips at the stack boundaries
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_STRIPS))
def test_strip_renders(renderer, oracle_lib, monkeypatch, name):
    """64x64 at 2 spp. The wavefront tracer (TravStack<39> extend, TravStack<25> shadow) and the megakernel on the
    canonical conversion (plain below need 30, DEEP from 30 on, overflow entries from 39 on) give the oracle's image and
    ray counts; shadow rays are cast; the launch rule of test_pt_stack_budget._check_rule holds; the model on the
    nodes read back from the device puts the case's pixels above the LDS depths."""
    need = _STRIPS[name][0]
    sc, ubo, tri = _upload_strip(renderer, monkeypatch, name)
    nodes, recs = _bvh_arrays(renderer)
    assert B.tree_violations(nodes, recs, tri.reshape(-1, 3, 3), 1, 4) == []
    m = _check_model(name, nodes, recs)
    stack, opt, build = renderer.scene_pt_stack(), renderer.scene_tree_opt(), renderer.scene_build()
    print(f"{name}: need {need}, deep_stack {build.deep_stack}, scene_pt_stack() {stack}, model pixels {m}")
    # the launch rule (test_pt_stack_budget._check_rule), on the canonical conversion
    lds, walked, deep = stack
    assert opt.applied == 0 and walked == need < STACK_TOTAL
    assert deep == (need >= PT_STACK) and lds == (DEEP_STACK if deep else PT_STACK)
    o, counts = _oracle(oracle_lib, name, sc, ubo, W, H, SPP)
    assert counts[1] > 0 and counts[2] == W * H * SPP
    for wavefront in (True, False):
        img, c = _trace(renderer, ubo, W, H, SPP, wavefront)
        ndiff = int(np.count_nonzero(np.any(img != o, axis=-1)))
        assert np.array_equal(img, o), f"{'wavefront' if wavefront else 'megakernel'}: {ndiff} pixels differ"
        assert c[:3] == counts and c[1] > 0 and c[3:] == (0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_STRIPS))
def test_strip_depth(renderer, oracle_lib, monkeypatch, name):
    """trace_depth against the oracle's, as test_hybrid_gpu.test_depth_parity: pt_depth_kernel<false, true> from
    need 39 on."""
    import torch
    sc, ubo, _ = _upload_strip(renderer, monkeypatch, name)
    d = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    renderer.trace_depth(ubo, W, H, d)
    torch.cuda.synchronize()
    ref = oracle_lib.trace_depth(sc.desc(), ubo, W, H)
    assert np.array_equal(d.cpu().numpy(), ref)
    assert np.isfinite(ref).any()  # (the strip is seen)


def _torus_case(sc, tri):
    """The torus of test_raster_gpu.test_torus_parity, moved over the strip's wide part and scaled to it, so that a
    good part of its rays reach the strip."""
    xmax = float(tri[:, 3].max())
    s = min(xmax, 2000.0) / 8.0
    model = np.eye(4, dtype=np.float32)
    model[0, 0] = model[1, 1] = model[2, 2] = s
    model[0, 3], model[1, 3], model[2, 3] = 4.0 * s, 0.5, -3.0 * s  # (row-major here, column-major below)
    return torus_push(model=model.T.reshape(16), major_radius=3.5, minor_radius=1.0, height=3.0)


def _torus(renderer, oracle_lib, sc, push, samples, frames, flags=0):
    import torch
    hits_d = torch.zeros(len(samples) * 12, dtype=torch.float32, device="cuda")
    ds = torch.from_numpy(np.ascontiguousarray(samples.view(np.float32))).cuda()
    hits_o = np.zeros(len(samples), HITDATA_DTYPE) if oracle_lib is not None else None
    renderer.set_wavefront(False)
    renderer.set_flags(flags)
    try:
        renderer.stats_reset()
        for frame in range(frames):
            ubo = make_ubo(U.cornell_pose(), sc, frame, ambient=(0.1, 0.1, 0.1, 1.0))
            renderer.trace_torus(ubo, push, ds, len(samples), hits_d)
            if hits_o is not None:
                oracle_lib.trace_torus(sc.desc(), ubo, push, samples, hits_o)
        torch.cuda.synchronize()
        st = renderer.stats()
    finally:
        renderer.set_flags(0)
    return hits_d.cpu().numpy().view(HITDATA_DTYPE), hits_o, _counters(st)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_STRIPS))
def test_strip_torus(renderer, oracle_lib, monkeypatch, name):
    """The torus tracer against the oracle's, 3000 rays over 3 frames, field by field as test_torus_parity:
    pt_torus_kernel<false, false, true> from need 39 on."""
    sc, _, tri = _upload_strip(renderer, monkeypatch, name)
    hg, ho, _ = _torus(renderer, oracle_lib, sc, _torus_case(sc, tri), Y.torus_samples(3000), 3)
    for field in ("pos", "flag", "normal", "color"):
        assert np.array_equal(hg[field], ho[field]), field
    assert np.count_nonzero(ho["flag"] > 0) > 0  # (some rays reach the strip)


# ---------------------------------------------------------------------------------------------------
# B. the wavefront tracer on the degenerate sets
# ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(B.SETS) + ["soup1025", "soup4097"])
def test_wavefront_on_degenerate_sets(renderer, oracle_lib, monkeypatch, name):
    """Coincident and zero-area triangles, the planar grid, the line, the offset soup and two soup sizes, host
    builder, default tries, 64x48 at 2 spp: the wavefront tracer gives the oracle's image and ray counts
    (test_bvh_build_gpu.py's scene, pose, ambient and cached oracle image)."""
    import test_bvh_build_gpu as G
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    monkeypatch.delenv("PTGS_PT_TREE_OPT", raising=False)
    sc, ubo, _ = G._scene(name)
    img, rays = G._oracle(oracle_lib, name)
    renderer.set_wavefront(False)
    renderer.set_flags(0)
    renderer.upload_scene(sc)
    assert renderer.scene_build().builder == G.HOST
    got, c = _trace(renderer, ubo, G.W, G.H, G.SPP, True)
    assert np.array_equal(got, img), f"{int(np.count_nonzero(np.any(got != img, -1)))} pixels differ"
    assert c[:2] == rays and c[2] == G.W * G.H * G.SPP


# ---------------------------------------------------------------------------------------------------
# C. the counting instantiations
# ---------------------------------------------------------------------------------------------------
_FEATURES = {}


def _count_scene(renderer, monkeypatch, name):
    """Upload one of part C's scenes: (scene, ubo, w, h, oracle key)."""
    if name in _STRIPS:
        sc, ubo, _ = _upload_strip(renderer, monkeypatch, name)
        return sc, ubo, W, H, name
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    monkeypatch.delenv("PTGS_PT_TREE_OPT", raising=False)
    if name not in _FEATURES:
        sc = U.features(textured=name == "textured")
        _FEATURES[name] = (sc, make_ubo(U.cornell_pose(160 / 120), sc, 0, ambient=(0.05, 0.05, 0.08, 1.0)))
    sc, ubo = _FEATURES[name]
    renderer.set_wavefront(False)
    renderer.set_flags(0)
    renderer.upload_scene(sc)
    return sc, ubo, 160, 120, name + " 160x120"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["features", "textured", "need40", "wide26", "deep45"])
def test_counting_renders_the_same_image(renderer, oracle_lib, monkeypatch, name):
    """Both tracers, flag off then on: the counters stay zero without the flag; with it the image is the flag-off
    image and the oracle's bit for bit and the ray counts are equal; closest_hits agree between the tracers and lie in
    (0, extension_rays]; tri_tests >= closest_hits; node_visits >= 4 * (extension + shadow rays), every ray testing the
    root's four boxes at least once; a second identical call gives identical counters (the slot-to-wave mapping of the
    wavefront stages and the tile-to-wave mapping of the megakernel do not depend on timing: the tile schedule only
    reorders whole one-wave tiles)."""
    sc, ubo, w, h, key = _count_scene(renderer, monkeypatch, name)
    o, counts = _oracle(oracle_lib, key, sc, ubo, w, h, SPP)
    hits = {}
    for wavefront in (False, True):
        off, c_off = _trace(renderer, ubo, w, h, SPP, wavefront)
        on, c_on = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
        again, c_again = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
        print(f"{name} {'wavefront' if wavefront else 'megakernel'}: {c_on}")
        assert c_off[3:] == (0, 0, 0) and c_off[:3] == counts
        assert np.array_equal(off, o) and np.array_equal(on, off) and np.array_equal(again, on)
        assert c_on[:3] == counts and c_again == c_on
        ext, shd, _, nodes, tris, ch = c_on
        assert 0 < ch <= ext and tris >= ch
        assert nodes >= NODE_STEP * (ext + shd) and nodes % NODE_STEP == 0
        hits[wavefront] = ch
    assert hits[False] == hits[True]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["need40", "wide26"])
def test_all_miss_render_counts_one_root_step_per_ray(renderer, monkeypatch, name):
    """A camera at the strip's narrow end looking away from it: every primary ray misses every box of the root, so
    each sample is one extension ray of exactly one node step, no triangle test, no hit, no shadow ray."""
    sc, _, _ = _upload_strip(renderer, monkeypatch, name)
    pose = S.Camera(aspect=1.0).look_at([-0.5, 0.5, 0.4], [-10.0, 0.5, 0.4])
    ubo = make_ubo(pose, sc, 0, ambient=AMBIENT)
    for wavefront in (False, True):
        _, c = _trace(renderer, ubo, W, H, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
        assert c == (W * H * SPP, 0, W * H * SPP, NODE_STEP * W * H * SPP, 0, 0), (wavefront, c)


def _one_node_scene():
    """A floor of two triangles, a small plate of two above it and a point light above the plate: four triangles,
    so the canonical tree (and the megakernel's copy) is the root alone and every walk is exactly one node step."""
    fl, pl = 4.0, 0.7
    quad = lambda s, y: [[[-s, y, -s], [s, y, s], [s, y, -s]], [[-s, y, -s], [-s, y, s], [s, y, s]]]  # noqa: E731
    tri = np.array(quad(fl, 0.0) + quad(pl, 1.0), np.float32)
    light = np.zeros(1, PUNCTUAL_LIGHT_DTYPE)
    light["position"], light["color"], light["intensity"], light["type"] = [0.3, 3.0, 0.2], [1.0, 1.0, 1.0], 30.0, 0
    sc = B.scene(tri, lights=[light[0]])
    pose = S.Camera(aspect=1.0).look_at([3.0, 3.5, 4.0], [0.0, 0.3, 0.0])
    return sc, make_ubo(pose, sc, 0, ambient=AMBIENT)


@pytest.mark.gpu
def test_one_node_scene_counts_exactly(renderer, oracle_lib, monkeypatch):
    """Four triangles: one 4-wide node. Every extension ray and every shadow ray tests the root once and has no
    other node to test, so node_visits == 4 * (extension_rays + shadow_rays) in both tracers: a walk (closest-hit or
    any-hit, of either tracer) that stopped counting its node steps breaks the equality. Lit and shadowed floor
    points both occur."""
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)
    monkeypatch.delenv("PTGS_PT_TREE_OPT", raising=False)
    sc, ubo = _one_node_scene()
    renderer.set_wavefront(False)
    renderer.set_flags(0)
    renderer.upload_scene(sc)
    assert renderer.scene_info().num_bvh_nodes == 1 and renderer.scene_tree_opt().num_nodes == 1
    o, counts = _oracle(oracle_lib, "one node", sc, ubo, W, H, SPP)
    assert counts[1] > 0
    got = {}
    for wavefront in (False, True):
        img, c = _trace(renderer, ubo, W, H, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
        assert np.array_equal(img, o) and c[:3] == counts
        ext, shd, _, nodes, tris, ch = c
        assert nodes == NODE_STEP * (ext + shd), (wavefront, c)
        assert 0 < ch < ext and ch <= tris <= 4 * (ext + shd)
        got[wavefront] = c
    assert got[False][5] == got[True][5]


@pytest.mark.gpu
@pytest.mark.parametrize("wavefront", [False, True])
def test_counters_accumulate_and_reset(renderer, monkeypatch, wavefront):
    """Two counted renders without stats_reset() between them give exactly twice one render's six counters;
    stats_reset() returns all six to zero."""
    _, ubo, w, h, _ = _count_scene(renderer, monkeypatch, "features")
    _, one = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
    _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
    _, two = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL, reset=False)
    assert all(v > 0 for v in one) and two == tuple(2 * v for v in one)
    renderer.stats_reset()
    assert _counters(renderer.stats()) == (0, 0, 0, 0, 0, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("wavefront", [False, True])
def test_counted_rows_add_up(renderer, monkeypatch, wavefront):
    """Rows [0, 64) and [64, 120) of the features render add up to the full frame in extension rays, shadow rays,
    samples and closest_hits. (node_visits and tri_tests are not asserted to add up: the postponed-leaf walk culls
    with a hit distance whose timing depends on the other lanes of the wave.)"""
    _, ubo, w, h, _ = _count_scene(renderer, monkeypatch, "features")
    full, c = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL)
    top, a = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL, rows=(0, 64))
    bottom, b = _trace(renderer, ubo, w, h, SPP, wavefront, FLAG_COUNT_TRAVERSAL, rows=(64, 120))
    for k in (0, 1, 2, 5):
        assert a[k] + b[k] == c[k] and a[k] > 0 and b[k] > 0, (k, a, b, c)
    assert np.array_equal(top[:64], full[:64]) and np.array_equal(bottom[64:], full[64:])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["need40", "features"])
def test_torus_counting(renderer, monkeypatch, name):
    """pt_torus_kernel<true, *, *>: the hit data with the flag equals the hit data without it, word for word; the
    flag-off run counts nothing; closest_hits <= extension_rays, every ray tests the root."""
    sc, _, _, _, _ = _count_scene(renderer, monkeypatch, name)
    push = _torus_case(sc, _strip_scene(name)[3]) if name in _STRIPS else torus_push(major_radius=3.5, minor_radius=1.0, height=3.0)
    samples = Y.torus_samples(3000)
    off, _, c_off = _torus(renderer, None, sc, push, samples, 2)
    on, _, c_on = _torus(renderer, None, sc, push, samples, 2, FLAG_COUNT_TRAVERSAL)
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    assert c_off[3:] == (0, 0, 0) and c_on[:3] == c_off[:3] and c_on[2] == 2 * len(samples)
    ext, shd, _, nodes, tris, ch = c_on
    assert 0 < ch <= ext and tris >= ch and nodes >= NODE_STEP * (ext + shd)


# ---------------------------------------------------------------------------------------------------
# D. the wavefront tracer's tuning variables, in fresh processes
# ---------------------------------------------------------------------------------------------------
_KNOBS = [(64, 64, 1, 1), (65536, 65536, 64, 3), (128, 65536, 33, 256), (256, 256, 16, 16)]


def _honoured(setting):
    """pt_wavefront.hip's own rule: wf_env takes a run of >= 64, caps it at 65536 and rounds it down to a multiple
    of 64 (else the default); the refill threshold is taken in 1..64, the batch in 1..256."""
    trace, shade, refill, batch = setting
    return all(v >= 64 and (min(v, 65536) & ~63) == v for v in (trace, shade)) and 1 <= refill <= 64 and 1 <= batch <= 256


def test_knob_settings_are_ones_the_library_honours():
    src = open(os.path.join(CSRC, "pt_wavefront.hip")).read()
    # the rule _honoured restates, as the source states it
    assert "return v >= 64 ? (uint32_t)(std::min(v, 65536L) & ~63L) : dflt;" in src
    assert re.search(r'getenv\("PTGS_WF_REFILL"\);\s*const long v = [^;]*;\s*return v >= 1 && v <= 64 \?', src)
    assert re.search(r'getenv\("PTGS_WF_BATCH"\);\s*const long v = [^;]*;\s*return v >= 1 && v <= 256 \?', src)
    for name in ("PTGS_WF_TRACE_RUN", "PTGS_WF_SHADE_RUN"):
        assert f'wf_env("{name}", {name})' in src
    assert all(_honoured(s) for s in _KNOBS) and len(set(_KNOBS)) == len(_KNOBS)
    assert not _honoured((63, 64, 1, 1)) and not _honoured((100, 64, 1, 1)) and not _honoured((64, 64, 65, 1))
    assert not _honoured((64, 64, 1, 257)) and not _honoured((64, 131072, 1, 1))


@pytest.mark.gpu
def test_wavefront_knobs_in_fresh_processes(renderer, oracle_lib, tmp_path):
    """Run lengths of one window and of 65536 slots (the 16-bit ring offsets' limit; cornell at 512x512 is exactly
    four such runs), a refill threshold of every idle lane, of 64 and of 33, batches of 1, of 3 (7 spp: 3, 3, 1) and of
    256, and the defaults: every child's two images equal the oracle's and each other's, with equal counts. The first
    child that fails ends the test."""
    import wf_knobs_child as K
    feat, feat_ubo, init = K.features_case()
    corn, corn_ubo = K.cornell_case()
    fo, fcounts = _oracle(oracle_lib, "knobs features", feat, feat_ubo, K.FW, K.FH, K.FSPP, init=init)
    co, ccounts = _oracle(oracle_lib, "knobs cornell", corn, corn_ubo, K.CW, K.CH, 1)
    assert fcounts[2] == K.FW * K.FH * K.FSPP and ccounts[2] == 4 * 65536
    for setting in _KNOBS:
        out = os.path.join(str(tmp_path), "knobs_%d_%d_%d_%d.npz" % setting)
        env = {**os.environ, "PYTHONPATH": os.pathsep.join([ROOT, HERE, os.environ.get("PYTHONPATH", "")])}
        for var, v in zip(("PTGS_WF_TRACE_RUN", "PTGS_WF_SHADE_RUN", "PTGS_WF_REFILL", "PTGS_WF_BATCH"), setting):
            env[var] = str(v)
        r = subprocess.run([sys.executable, os.path.join(HERE, "wf_knobs_child.py"), out], env=env, timeout=120,
                           capture_output=True, text=True)
        assert r.returncode == 0, (setting, (r.stdout + r.stderr)[-4000:])
        z = np.load(out)
        assert np.array_equal(z["features"], fo), setting
        assert np.array_equal(z["cornell"], co), setting
        assert tuple(z["features_counts"].tolist()) == fcounts and tuple(z["cornell_counts"].tolist()) == ccounts, setting
