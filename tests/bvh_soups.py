"""Small seeded triangle sets for the BVH builders' tests (host SAH, GPU SAH, GPU LBVH, the collapses).

Every generator is deterministic from its seed and returns float32 triangles [n, 3, 3]; scene(tri) wraps
them into a Scene with one diffuse material (the tests add a non-zero ambient so the image is not black).
The sets sit at the sizes and degeneracies at which the builders take another path (bvh_sah_gpu.hip:
1024-reference phase boundary, 2048-reference chunks; centroid bounds of zero extent; identical
centroids / Morton keys; zero-area triangles; coordinates far from the origin)."""
from __future__ import annotations

import numpy as np

import scenes_util as U
from pathtracer_gaussiansplatting_amd import scene as S
from pathtracer_gaussiansplatting_amd._abi import PRIMITIVE_DTYPE, VERTEX_DTYPE

CUBE = 6.0     # soup centres: uniform in [-CUBE / 2, CUBE / 2]^3
JITTER = 0.05  # vertices within +-JITTER of the centre


def centroids(tri):
    """bvh.cpp Ref::c: 0.5 * (box lo + box hi) in float32, [n, 3]."""
    tri = np.asarray(tri, np.float32)
    return (np.float32(0.5) * (tri.min(axis=1) + tri.max(axis=1))).astype(np.float32)


def _no_axis_ties(c):
    return all(len(np.unique(c[:, a])) == len(c) for a in range(3))


def soup(n, seed=1):
    """n small triangles, centres uniform in a 6-unit cube. No two centroids tie, on any axis (a triangle
    whose centroid would tie is drawn again from the same stream)."""
    rng = np.random.default_rng([seed, n])
    tri = np.zeros((n, 3, 3), np.float32)
    todo = np.arange(n)
    for _ in range(64):
        ctr = rng.uniform(-CUBE / 2, CUBE / 2, (len(todo), 1, 3))
        tri[todo] = (ctr + rng.uniform(-JITTER, JITTER, (len(todo), 3, 3))).astype(np.float32)
        c = centroids(tri)
        bad = np.zeros(n, bool)
        for a in range(3):
            _, first, counts = np.unique(c[:, a], return_index=True, return_counts=True)
            keep = np.zeros(n, bool)
            keep[first] = True
            bad |= ~keep
        todo = np.flatnonzero(bad)
        if len(todo) == 0:
            break
    assert _no_axis_ties(centroids(tri))
    return tri


def grid(nu=34, nv=34):
    """The nu x nv x 2 regular grid in the plane y = 0 (2312 triangles): zero centroid extent in y, the
    two triangles of a cell share their box (so their centroid), and many SAH costs tie."""
    s = (np.arange(nu + 1) / nu * CUBE - CUBE / 2).astype(np.float32)
    t = (np.arange(nv + 1) / nv * CUBE - CUBE / 2).astype(np.float32)
    X, Z = np.meshgrid(s, t, indexing="ij")
    P = np.stack([X, np.zeros_like(X), Z], -1)  # [nu + 1, nv + 1, 3]
    a, b, c, d = P[:-1, :-1], P[:-1, 1:], P[1:, 1:], P[1:, :-1]  # (winding: normal +y)
    tri = np.stack([np.stack([a, b, c], -2), np.stack([a, c, d], -2)], -3)  # [nu, nv, 2, 3, 3]
    return np.ascontiguousarray(tri.reshape(-1, 3, 3), np.float32)


def line(n, seed=2):
    """One triangle shape at n distinct x (shuffled order): the centroids differ in x only."""
    rng = np.random.default_rng([seed, n])
    x = (np.arange(n, dtype=np.float64) / n * CUBE - CUBE / 2).astype(np.float32)
    x = x[rng.permutation(n)]
    # (offsets that are exact in float32 at |x| <= 4, so every box has the same y, z and x extent)
    shape = np.array([[-0.03125, -0.03125, 0.0], [0.03125, -0.03125, 0.015625], [0.0, 0.046875, -0.015625]], np.float32)
    tri = np.broadcast_to(shape, (n, 3, 3)).copy()
    tri[:, :, 0] += x[:, None]
    c = centroids(tri)
    assert len(np.unique(c[:, 0])) == n and len(np.unique(c[:, 1])) == 1 and len(np.unique(c[:, 2])) == 1
    return tri


def dup_all(n=600, seed=3):
    """One triangle n times: every centroid, box and Morton key is the same."""
    return np.repeat(soup(16, seed)[5:6], n, axis=0)


def dup_mix(seed=4):
    """soup(2000) plus 300 copies of one of its triangles (2300 triangles)."""
    tri = soup(2000, seed)
    return np.concatenate([tri, np.repeat(tri[777:778], 300, axis=0)])


def degenerate(seed=5):
    """soup(1200) with 50 triangles collapsed to a point and 50 to a segment (zero area)."""
    tri = soup(1200, seed)
    rng = np.random.default_rng([seed, 99])
    pick = rng.permutation(1200)[:100]
    tri[pick[:50], 1] = tri[pick[:50], 0]
    tri[pick[:50], 2] = tri[pick[:50], 0]
    tri[pick[50:], 2] = tri[pick[50:], 1]
    return tri


OFFSET = (1e5, -2e5, 3e4)


def offset(seed=6):
    """soup(1500) translated by (1e5, -2e5, 3e4): the coordinates round to float32 steps of up to 1/64
    (the boxes' absolute padding comes from the largest coordinate, bvh.cpp pad_abs)."""
    return (soup(1500, seed).astype(np.float64) + np.asarray(OFFSET)).astype(np.float32)


def strip(x):
    """Thin triangles side by side along x, one per interval of the ascending positions x (each 1 long in y,
    slightly tilted in z), float32 [n, 9]."""
    t = np.zeros((len(x) - 1, 9), np.float32)
    t[:, 0], t[:, 3], t[:, 6] = x[:-1], x[1:], x[:-1]
    t[:, 4] = 1.0
    t[:, 7], t[:, 8] = 1.0, x[:-1] * np.float32(0.25)
    return t


def geometric_slivers(n, ratio, first=1e-5):
    """A strip of n triangles, every one `ratio` times as wide as the one before (the first `first`): the SAH build
    splits the wide end off again and again, so the tree is a chain and its stack need grows with n, not log n."""
    return strip((np.float64(ratio) ** np.arange(n + 1) * first).astype(np.float32))


def scene(tri, lights=()):
    """A Scene of the triangles (one object, one mesh, one diffuse material), in this order. lights: scene-level
    punctual lights (PUNCTUAL_LIGHT_DTYPE records, SceneBuilder.add_punctual_light); none by default."""
    tri = np.ascontiguousarray(tri, np.float32)
    n = len(tri)
    nrm = np.cross((tri[:, 1] - tri[:, 0]).astype(np.float64), (tri[:, 2] - tri[:, 0]).astype(np.float64))
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-300), [0.0, 1.0, 0.0])
    v = np.zeros(3 * n, VERTEX_DTYPE)
    v["pos"] = tri.reshape(-1, 3)
    v["normal"] = np.repeat(nrm, 3, axis=0)
    v["color"] = 1.0
    v["tangent"] = [1.0, 0.0, 0.0, 0.0]
    prims = np.zeros(1, PRIMITIVE_DTYPE)
    prims["index_count"] = 3 * n
    m = S.default_material()
    m["metallic_factor"] = 0.0
    m["base_color_factor"] = [0.8, 0.7, 0.6, 1.0]
    b = S.SceneBuilder().add_object(v, np.arange(3 * n, dtype=np.uint32), prims, m)
    for light in lights:
        b.add_punctual_light(light)
    sc = b.finalize()
    sc.blue_noise = U.blue_noise()
    return sc


def triangles(sc):
    """The scene's triangles in flattening order (api.cpp ptgs_scene_upload), float32 [n, 3, 3]."""
    pos = np.asarray(sc.vertices["pos"], np.float32)
    out = []
    for m, cnt in zip(sc.meshes, sc.mesh_index_count):
        cnt = int(cnt)
        if cnt < 3:
            continue
        idx = np.asarray(sc.indices[int(m["index_offset"]):int(m["index_offset"]) + cnt // 3 * 3], np.int64)
        out.append(pos[idx + int(m["vertex_offset"])].reshape(-1, 3, 3))
    return np.ascontiguousarray(np.concatenate(out), np.float32)


def pose(tri, aspect=64 / 48, close=True):
    """A camera looking at the set's middle: from outside its bounds, or (close: the soups' triangles are
    a fraction of a pixel from there) from 0.3 units in front of the triangle nearest the middle, which
    then fills a good part of the view with the rest of the set around and behind it."""
    tri = np.asarray(tri, np.float64)
    lo, hi = tri.reshape(-1, 3).min(0), tri.reshape(-1, 3).max(0)
    mid = 0.5 * (lo + hi)
    r = max(float(np.max(hi - lo)), 0.5)
    d = np.array([0.35, 0.8, 1.1])
    if not close:
        return S.Camera(aspect=aspect).look_at(mid + d * r, mid)
    ctr = tri.mean(axis=1)
    near = np.argsort(np.linalg.norm(ctr - mid, axis=1), kind="stable")[:32]
    nrm = np.cross(tri[near, 1] - tri[near, 0], tri[near, 2] - tri[near, 0])
    k = int(np.argmax(np.linalg.norm(nrm, axis=1)))  # the largest of the 32 nearest, seen face on
    n = nrm[k] / np.linalg.norm(nrm[k])
    up = (0.0, 1.0, 0.0) if abs(n[1]) < 0.9 else (1.0, 0.0, 0.0)
    return S.Camera(aspect=aspect, fov_deg=25.0).look_at(ctr[near[k]] + n * 0.3, ctr[near[k]], up)


def tree_violations(nodes, recs, tri, leaf, fan):
    """The validity conditions of tests/native/bvh_build_check.cpp on 4-wide nodes (u32 [n, 32]) and
    triangle records (u32 [t, 12]) as ptgs_scene_get_bvh exposes them, against the input triangles
    (float32 [t, 3, 3], record word 11 is the triangle's index): a list of violation strings, empty
    when the tree is valid. Every triangle in exactly one record and one leaf; leaves of 1 .. leaf
    triangles inside the array; 2 .. fan occupied slots, in front, the others the 1e30 point boxes with
    link 0; every node but the root linked once, from a lower index; every child box contains every
    vertex below it (exact float compares: the boxes are padded outward)."""
    nodes = np.asarray(nodes, np.uint32)
    recs = np.asarray(recs, np.uint32)
    tri = np.asarray(tri, np.float32)
    nt, nn = len(tri), len(nodes)
    bad = []
    if len(recs) != nt:
        return [f"{len(recs)} records for {nt} triangles"]
    gid = recs[:, 11].astype(np.int64)
    if not np.array_equal(np.sort(gid), np.arange(nt)):
        return ["record ids are no permutation of the triangles"]
    vlo, vhi = tri.min(axis=1)[gid], tri.max(axis=1)[gid]  # per record
    f = nodes[:, :24].view(np.float32).reshape(nn, 6, 4)   # [node, (lo.x hi.x lo.y hi.y lo.z hi.z), slot]
    link = nodes[:, 24:28].view(np.int32)
    if np.any(nodes[:, 28:32] != 0):
        bad.append("unused node words not zero")
    empty = np.all(f == np.float32(1e30), axis=1)           # [node, slot]
    occupied = (~empty).sum(axis=1)
    if np.any(occupied < 2) or np.any(occupied > fan):
        bad.append(f"occupied slots outside 2..{fan}: {np.unique(occupied).tolist()}")
    if np.any(empty[:, :-1] & ~empty[:, 1:]):
        bad.append("occupied slot after an empty one")
    if np.any(link[empty] != 0):
        bad.append("empty slot with a link")
    cover = np.zeros(nt, np.int64)
    linked = np.zeros(nn, np.int64)
    blo = np.full((nn, 3), np.inf, np.float32)
    bhi = np.full((nn, 3), -np.inf, np.float32)
    for i in range(nn - 1, -1, -1):  # children after parents (breadth-first numbering)
        for j in range(4):
            if empty[i, j]:
                continue
            ln = int(link[i, j])
            if ln < 0:
                L = ~ln
                first, count = L & 0x07FFFFFF, (L >> 27) + 1
                if first + count > nt or count > leaf:
                    bad.append(f"node {i} slot {j}: leaf [{first}, +{count})")
                    continue
                cover[first:first + count] += 1
                lo, hi = vlo[first:first + count].min(axis=0), vhi[first:first + count].max(axis=0)
            elif ln <= i or ln >= nn:
                bad.append(f"node {i} slot {j}: link {ln}")
                continue
            else:
                linked[ln] += 1
                lo, hi = blo[ln], bhi[ln]
            if not (np.all(f[i, 0::2, j] <= lo) and np.all(f[i, 1::2, j] >= hi)):
                bad.append(f"node {i} slot {j}: box does not contain its subtree")
            blo[i] = np.minimum(blo[i], lo)
            bhi[i] = np.maximum(bhi[i], hi)
    if np.any(cover != 1):
        bad.append(f"{int(np.count_nonzero(cover != 1))} records not in exactly one leaf")
    if np.any(linked[1:] != 1):
        bad.append(f"{int(np.count_nonzero(linked[1:] != 1))} nodes not linked exactly once")
    return bad


# name -> generator of the fixed sets (soup sizes are made by soup(n))
SETS = {"grid": grid, "line1500": lambda: line(1500), "dup_all": dup_all, "dup_mix": dup_mix,
        "degenerate": degenerate, "offset": offset}
SOUP_SIZES = (16, 17, 1024, 1025, 2048, 2049, 4097)

_TRI = {}


def get(name):
    """The named set ("soup<n>" or a key of SETS), generated once."""
    if name not in _TRI:
        _TRI[name] = soup(int(name[4:])) if name.startswith("soup") else SETS[name]()
        _TRI[name].setflags(write=False)
    return _TRI[name]
