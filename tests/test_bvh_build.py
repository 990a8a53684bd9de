"""The host BVH build (bvh.cpp build_bvh + collapse_bvh4), the reference the GPU builders are compared
with, on the edge-case triangle sets of bvh_soups.py.

tests/native/bvh_build_check.cpp is a stand-alone program (its own main, host code only), built here with
g++ -fsanitize=address,undefined. It builds the tree at a (leaf size, fan-out, depth budget) and checks:
every triangle in exactly one leaf, leaf sizes, every child box of the BVH2 and of the 4-wide nodes
contains its subtree's vertices exactly, the depth within its budget, the balanced splits the budget
forces (n / 2 left, centroids ordered along the widest axis), the reported stack need / depths against a
recomputation, the fan-out cap and the empty slots. Every condition is an integer count: zero violations."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import bvh_soups as B

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
    out = os.path.join(out_dir, "bvh_build_check")
    srcs = [os.path.join(CSRC, "bvh.cpp"), os.path.join(NATIVE, "bvh_build_check.cpp")]
    deps = srcs + [os.path.join(CSRC, "bvh.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        cmd = ["g++", "-O1", "-g", "-std=c++17", "-fno-omit-frame-pointer", "-ffp-contract=off",
               "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC] + srcs + ["-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


def _run(check_bin, tmp_path, name, tries, dump=None):
    tri = B.get(name)
    path = os.path.join(str(tmp_path), "tris.bin")
    np.ascontiguousarray(tri, np.float32).tofile(path)
    leaf, fan, depth = tries.split(":")
    r = subprocess.run([check_bin, path, leaf, fan, depth] + ([dump] if dump else []), capture_output=True, text=True,
                       timeout=300,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0",
                            "UBSAN_OPTIONS": "print_stacktrace=1"})
    print(name, tries, r.stdout.strip())
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    w = r.stdout.split()
    st = dict(zip(w[1::2], map(int, w[2::2])))
    assert st["violations"] == 0 and st["tris"] == len(tri)
    assert st["maxleaf"] <= int(leaf) and st["depth2"] <= int(depth)
    assert st["stack"] < 39  # (PTGS_STACK: none of these sets may fall back to another tree shape)
    return st


ALL_SETS = ["soup%d" % n for n in (15,) + B.SOUP_SIZES] + sorted(B.SETS)


@pytest.mark.parametrize("name", ALL_SETS)
def test_host_tree_of_every_set(check_bin, tmp_path, name):
    """The default tree (3-triangle leaves, fan-out 4, depth budget 38) of every set: zero violations,
    and no budget-forced split (the budget is far away: the GPU tests' default cases compare SAH splits)."""
    st = _run(check_bin, tmp_path, name, "3:4:38")
    assert st["balanced"] == 0
    assert st["leaves4"] == st["leaves"]


@pytest.mark.parametrize("tries", ["4:4:10", "4:4:12", "3:4:11"])
def test_depth_budget_forces_balanced_splits(check_bin, tmp_path, tries):
    """soup(2500) at depth budgets below its SAH tree's depth: the tree honours the budget and the
    program counts the balanced splits the budget forced (otherwise the case tests nothing). At
    4:4:10 and 3:4:11 the root itself is balanced (0 + ceil(log2(2500 / leaf)) + 1 = 11 is not below
    the budget), so no split is an SAH split and the depth is ceil(log2(2500 / leaf)); at 4:4:12 the
    root and the levels below it are SAH splits, the deeper ones balanced."""
    st = _run(check_bin, tmp_path, "soup2500", tries)
    assert st["balanced"] > 0
    free = _run(check_bin, tmp_path, "soup2500", tries.rsplit(":", 1)[0] + ":38")
    assert free["balanced"] == 0  # (the same leaf size with the budget out of reach takes none)
    if tries == "4:4:12":
        assert st["sah"] > 0
    else:
        assert st["sah"] == 0 and st["depth2"] == 10


@pytest.mark.parametrize("tries", ["3:3:38", "3:2:38", "1:4:38", "2:4:38"])
def test_fan_out_and_leaf_sizes(check_bin, tmp_path, tries):
    """Fan-out 3 and 2 (the collapse's fallback shapes) and leaf sizes 1 and 2 on soup(2500)."""
    st = _run(check_bin, tmp_path, "soup2500", tries)
    leaf, fan, _ = map(int, tries.split(":"))
    if fan == 2:  # nothing is opened: one 2-wide node per BVH2 node, two empty slots each
        assert st["nodes4"] == st["nodes2"] and st["empty"] == 2 * st["nodes4"]
    if fan == 3:
        assert st["empty"] >= st["nodes4"]
    assert st["leaves4"] == st["leaves"]


@pytest.mark.parametrize("name,tries", [("soup2049", "3:4:38"), ("dup_mix", "3:3:38"), ("grid", "2:2:38")])
def test_numpy_restatement_agrees_and_catches_damage(check_bin, tmp_path, name, tries):
    """bvh_soups.tree_violations (what the GPU tests apply to the device trees) on the host tree the
    program dumps: no violation, but one under a smaller fan-out cap; a leaf box's plane moved inside
    its triangles' bounds by one float step, a leaf range shifted by one, a leaf's slot emptied and an
    interior link cut are each reported."""
    dump = os.path.join(str(tmp_path), "tree.bin")
    st = _run(check_bin, tmp_path, name, tries, dump)
    tri = B.get(name)
    leaf, fan, _ = map(int, tries.split(":"))
    raw = np.fromfile(dump, np.uint32)
    n4 = int(raw[0])
    assert n4 == st["nodes4"] and len(raw) == 1 + 32 * n4 + 12 * len(tri)
    nodes, recs = raw[1:1 + 32 * n4].reshape(n4, 32), raw[1 + 32 * n4:].reshape(-1, 12)
    assert B.tree_violations(nodes, recs, tri, leaf, fan) == []
    assert B.tree_violations(nodes, recs, tri, leaf, fan - 1) != [] or fan == 2
    links = nodes[:, 24:28].view(np.int32)
    leaf_at = np.argwhere(links < 0)
    i, j = (int(x) for x in leaf_at[len(leaf_at) // 2])

    def damaged(edit):
        m = nodes.copy()
        edit(m, m[:, :24].view(np.float32), m[:, 24:28].view(np.int32))
        return B.tree_violations(m, recs, tri, leaf, fan)

    def lo_inward(m, f, l):  # the tight plane of a leaf box: the padding is a few float steps at most
        L = ~int(l[i, j])
        first, count = L & 0x07FFFFFF, (L >> 27) + 1
        vmin = tri[recs[first:first + count, 11]].reshape(-1, 3)[:, 0].min()
        f[i, j] = np.nextafter(vmin, np.float32(np.inf), dtype=np.float32)

    def shift_leaf(m, f, l):
        l[i, j] = ~((~int(l[i, j])) + 1)

    def drop_leaf(m, f, l):
        f[i, j::4] = 1e30
        l[i, j] = 0

    def back_link(m, f, l):
        k = int(np.argwhere(l > 0)[-1][0])
        l[k][l[k] > 0] = 0

    for edit in (lo_inward, shift_leaf, drop_leaf, back_link):
        assert damaged(edit) != [], edit.__name__
