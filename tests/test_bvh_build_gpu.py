"""The GPU BVH builders (bvh_sah_gpu.hip, bvh_gpu.hip) and the GPU 4-wide collapse (bvh_collapse_gpu.hip)
on the edge-case triangle sets of bvh_soups.py, against the host build (bvh.cpp) and the CPU oracle.

Every case uploads its scene on the host path and with PTGS_FLAG_GPU_BVH, and asserts, always:
  - Renderer.scene_build() names the requested builder and the first (leaf, fan, depth budget) try: none
    of these sets may fall back (test_bvh_build.py: their stack needs are 13 .. 30, the limit is 39),
    and a fallen-back upload would make every comparison below trivially true;
  - bvh_soups.tree_violations (the numpy restatement of tests/native/bvh_build_check.cpp) finds nothing
    wrong with the 4-wide nodes and triangle records read back from the device;
  - a 64x48, 2 spp megakernel render equals the oracle's bit for bit, ray counts included.
GPU SAH, additionally, wherever no balanced split meets tied centroids: the 4-wide nodes equal the host's
word for word, every leaf holds the same triangles, node count / depth / largest leaf are equal.
There is no tolerance in this file: np.array_equal and integer counts only."""
import numpy as np
import pytest

import bvh_soups as B
from pathtracer_gaussiansplatting_amd import FLAG_GPU_BVH, FLAG_GPU_LBVH, make_ubo
from test_pt_gpu import _bvh_arrays, _leaf_sets_equal

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

W, H, SPP = 64, 48, 2
AMBIENT = (0.3, 0.4, 0.5, 1.0)
HOST, GPU_SAH, GPU_LBVH = 0, 1, 2
DEFAULT_TRY = (3, 4, 38)  # bvh_tries.h default_bvh_tries()[0]

_SCENES = {}
_ORACLE = {}


def _scene(name):
    """(scene, ubo, triangles in flattening order) of a named set, built once."""
    if name not in _SCENES:
        sc = B.scene(B.get(name))
        tri = B.triangles(sc)
        assert np.array_equal(tri, B.get(name))
        pose = B.pose(tri, W / H, close=name != "grid")  # (the grid's cells are large enough from afar)
        _SCENES[name] = (sc, make_ubo(pose, sc, 0, ambient=AMBIENT), tri)
    return _SCENES[name]


def _oracle(oracle_lib, name):
    """The oracle's image and ray counts of a named set, rendered once (no test changes them)."""
    if name not in _ORACLE:
        sc, ubo, _ = _scene(name)
        img = np.zeros((H, W, 4), np.float32)
        st = oracle_lib.trace_camera(sc.desc(), ubo, W, H, img, spp=SPP)
        assert st.extension_rays >= W * H * SPP + 256  # (the triangles are seen: every hit adds a ray)
        img.setflags(write=False)
        _ORACLE[name] = (img, (st.extension_rays, st.shadow_rays))
    return _ORACLE[name]


def _upload(renderer, name, flags):
    """Upload with `flags`, render with the megakernel, read the tree back."""
    sc, ubo, _ = _scene(name)
    renderer.set_wavefront(False)
    renderer.set_flags(flags)
    try:
        renderer.upload_scene(sc)
        out = {"build": renderer.scene_build(), "info": renderer.scene_info()}
        out["nodes"], out["recs"] = _bvh_arrays(renderer)
        acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        renderer.stats_reset()
        renderer.trace_camera(ubo, W, H, acc, spp=SPP)
        torch.cuda.synchronize()
        st = renderer.stats()
        out["img"], out["rays"] = acc.cpu().numpy(), (st.extension_rays, st.shadow_rays)
    finally:
        renderer.set_flags(0)
    return out


def _always(up, oracle_lib, name, builder, tries):
    """The conditions every upload meets, whichever builder made the tree."""
    _, _, tri = _scene(name)
    b = up["build"]
    leaf, fan, depth = tries
    assert b.builder == builder, f"{name}: builder {b.builder}, wanted {builder} (a fallback?)"
    assert (b.leaf, b.fan, b.depth_budget) == (0 if builder == GPU_LBVH else leaf, fan, depth)
    assert b.stack_need < 39 and b.deep_stack == 0
    max_leaf = 4 if builder == GPU_LBVH else leaf  # (bvh_gpu.hip GS_BVH_LEAF)
    assert B.tree_violations(up["nodes"], up["recs"], tri, max_leaf, fan) == []
    assert up["info"].num_bvh_nodes == len(up["nodes"]) and up["info"].max_leaf_size <= max_leaf
    img, rays = _oracle(oracle_lib, name)
    assert np.array_equal(up["img"], img), f"{int(np.count_nonzero(np.any(up['img'] != img, -1)))} pixels differ"
    assert up["rays"] == rays


def _first_difference(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(np.any(a[:n] != b[:n], axis=1))
    return f"{len(a)} / {len(b)} nodes, first differing node {int(d[0]) if len(d) else n} (breadth first)"


def _is_the_host_tree(host, gpu):
    assert len(gpu["nodes"]) == len(host["nodes"]) and np.array_equal(gpu["nodes"], host["nodes"]), \
        _first_difference(gpu["nodes"], host["nodes"])
    assert _leaf_sets_equal(host["nodes"], host["recs"], gpu["recs"])
    hi, gi = host["info"], gpu["info"]
    assert (gi.num_bvh_nodes, gi.bvh_depth, gi.max_leaf_size) == (hi.num_bvh_nodes, hi.bvh_depth, hi.max_leaf_size)
    assert (gpu["build"].stack_need, gpu["build"].deep_stack) == (host["build"].stack_need, host["build"].deep_stack)


def _sah_case(renderer, oracle_lib, name, tries=DEFAULT_TRY, same_tree=True):
    host = _upload(renderer, name, 0)
    _always(host, oracle_lib, name, HOST, tries)
    gpu = _upload(renderer, name, FLAG_GPU_BVH)
    _always(gpu, oracle_lib, name, GPU_SAH, tries)
    if same_tree:
        _is_the_host_tree(host, gpu)
    return host, gpu


@pytest.fixture
def default_tries(monkeypatch):
    monkeypatch.delenv("PTGS_BVH_TRIES", raising=False)


@pytest.mark.parametrize("n", B.SOUP_SIZES)
def test_gpu_sah_soup_sizes(renderer, oracle_lib, default_tries, n):
    """soup(n) at the sizes where bvh_sah_gpu.hip changes path: 16 is the smallest scene the GPU path
    takes, 1024 is built by phase B alone, 1025 is the smallest phase-A root, 2048 fills one chunk, 2049
    has a second chunk of one reference, 4097 has three chunks and children that are phase-A tasks
    themselves. The GPU tree is the host tree."""
    _sah_case(renderer, oracle_lib, f"soup{n}")


def test_small_scene_falls_back_to_the_host_build(renderer, oracle_lib, default_tries):
    """Below 16 triangles the flagged upload uses the host build (api.cpp), and says so."""
    up = _upload(renderer, "soup15", FLAG_GPU_BVH)
    _always(up, oracle_lib, "soup15", HOST, DEFAULT_TRY)
    up = _upload(renderer, "soup15", FLAG_GPU_BVH | FLAG_GPU_LBVH)
    _always(up, oracle_lib, "soup15", HOST, DEFAULT_TRY)


@pytest.mark.parametrize("name", ["grid", "line1500", "degenerate", "offset"])
def test_gpu_sah_degenerate_sets(renderer, oracle_lib, default_tries, name):
    """Centroid bounds of zero extent on one axis (grid: a plane, with many tied SAH costs and two
    triangles per box) or two (line), zero-area triangles, coordinates of 1e5 (the absolute padding):
    the GPU tree is the host tree. None of these takes a balanced split among tied centroids: the
    budget is out of reach and the only coincident centroids (the grid's pairs) fit a leaf."""
    _sah_case(renderer, oracle_lib, name)


@pytest.mark.parametrize("name", ["dup_all", "dup_mix"])
def test_gpu_sah_coincident_triangles(renderer, oracle_lib, default_tries, name):
    """600 copies of one triangle, and 300 copies among 2000 others: their centroids tie, no SAH split
    separates them, and both builders fall to the balanced split, whose order among equal centroids
    bvh.cpp leaves to std::nth_element (unspecified) and bvh_sah_gpu.hip fixes by position. The host
    tree need not be reproduced here: the conditions that must still hold are the validity of the GPU
    tree (every triangle in one leaf, boxes contain their subtrees, leaf size and fan-out kept), the
    builder record, and the image and ray counts of the oracle."""
    _sah_case(renderer, oracle_lib, name, same_tree=False)


@pytest.mark.parametrize("tries", ["4:4:10", "4:4:12", "3:4:11"])
def test_gpu_sah_depth_budgets(renderer, oracle_lib, monkeypatch, tries):
    """soup(2500), no tied centroids, at depth budgets that force balanced splits (test_bvh_build.py
    counts them on the host tree): at 4:4:10 and 3:4:11 the root task of 2500 references, larger than a
    phase-B task, is handed whole from phase A to phase B and every split is balanced; at 4:4:12 the
    upper levels are SAH splits. The host upload under the same PTGS_BVH_TRIES is the reference."""
    monkeypatch.setenv("PTGS_BVH_TRIES", tries)
    host, gpu = _sah_case(renderer, oracle_lib, "soup2500", tuple(map(int, tries.split(":"))))
    assert gpu["info"].bvh_depth == host["info"].bvh_depth


@pytest.mark.parametrize("tries", ["3:3:38", "3:2:38", "2:4:38", "1:4:38"])
def test_gpu_collapse_fan_out_and_leaf_sizes(renderer, oracle_lib, monkeypatch, tries):
    """collapse_bvh4_gpu below fan-out 4 (what a too-deep scene gets) and the GPU SAH build at leaf
    sizes other than 3, on soup(2500): word for word the host upload under the same PTGS_BVH_TRIES."""
    monkeypatch.setenv("PTGS_BVH_TRIES", tries)
    leaf, fan, depth = map(int, tries.split(":"))
    host, gpu = _sah_case(renderer, oracle_lib, "soup2500", (leaf, fan, depth))
    assert gpu["build"].fan == fan and gpu["info"].max_leaf_size <= leaf
    occupied = (gpu["nodes"][:, 0:4].view(np.float32) != np.float32(1e30)).sum(axis=1)
    assert occupied.max() == fan


@pytest.mark.parametrize("name", ["soup16", "soup1025", "grid", "dup_all", "dup_mix"])
def test_gpu_lbvh_sets(renderer, oracle_lib, default_tries, name):
    """The GPU LBVH: identical Morton codes (dup_all, dup_mix, the grid's pairs) leave Karras' split to
    the index bits of the keys. Its tree is its own; validity, the builder record and the oracle's
    image hold."""
    up = _upload(renderer, name, FLAG_GPU_BVH | FLAG_GPU_LBVH)
    _always(up, oracle_lib, name, GPU_LBVH, DEFAULT_TRY)
