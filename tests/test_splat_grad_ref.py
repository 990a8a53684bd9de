"""The backward pass's reference (tests/splat_grad_ref.py) and its cases, checked without a GPU: the float64
evaluation reproduces the oracle's image, every case has the structure the GPU tests rely on and no borderline
decision, the per-Gaussian projection backward built for the host matches the reference, and the native library
exports the backward entry point. The frame cases (FRAME_CASES) are checked likewise, with their mask in the place
of the zero count."""
import os
import struct
import subprocess

import numpy as np
import pytest

import splat_grad_ref as R

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=sorted(R.CASES))
def case(request, oracle_lib):
    c = R.case_reference(request.param, oracle_lib)
    c["name"] = request.param
    return c


def _counts(c):
    rg = np.asarray(c["frame"]["ranges"]).reshape(-1, 2)
    return (rg[:, 1] - rg[:, 0]).astype(np.int64)


def test_reference_image_matches_the_oracle(case):
    err = R.rel_l2(case["r64"]["image"], case["frame"]["image"])
    print(f"{case['name']}: float64 reference vs oracle image rel L2 {err:.2e}")
    assert err < 1e-4, err


def test_no_borderline_decisions(case):
    """A condition on the seeds, not a tolerance: no skip / clamp / stop decision lies within 1e-3 relative of
    its threshold, in the float64 and in the float32 run."""
    assert case["r64"]["borderline"] == 0 and case["r32"]["borderline"] == 0
    assert case["r32"]["clamped"] == case["r64"]["clamped"] and case["r32"]["stopped"] == case["r64"]["stopped"]


def test_float32_reference_error(case):
    """e32, the float32 run of the same reference against its float64 run: the GPU bound is max(1e-4, 8 e32)."""
    for k in R.GRAD_KEYS:
        ref = case["r64"]["grads"][k]
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
        e32 = R.rel_l2(case["r32"]["grads"][k], ref)
        print(f"{case['name']} {k}: e32 {e32:.2e}")
        assert e32 < 1e-4  # (float32 itself stays well inside the project's 1e-4 allowance)


def test_case_structure(case):
    f, g, W, H = case["frame"], case["g"], case["W"], case["H"]
    cnt = _counts(case)
    gx, gy = (W + 15) // 16, (H + 15) // 16
    grid = cnt.reshape(gy, gx)
    assert any(v != 0.0 for v in case["bg"]) and np.count_nonzero(case["dL"][..., 3]) > 0  # (d)
    if case["name"] == "edges":  # (a)
        assert (W % 16, H % 16) != (0, 0) and W % 16 and H % 16
        assert grid[:, -1].max() > 0 and grid[-1, :].max() > 0  # pairs in partial tiles on both edges
        assert (cnt == 0).any() and (cnt > 0).any()
        view = np.asarray(case["ubo"].view, np.float64).reshape(4, 4).T
        d = -(np.c_[g["means"].astype(np.float64), np.ones(len(g["means"]))] @ view.T)[:, 2]
        near, behind = (d > 0) & (d <= 0.2), d < 0
        assert near.any() and behind.any()
        culled = f["radii"] == 0
        assert culled[near].all() and culled[behind].all()
        for k in R.GRAD_KEYS:  # a culled Gaussian has exactly zero gradients
            assert not np.any(case["r64"]["grads"][k][culled])
    if case["name"] == "batches":  # (b)
        assert cnt.max() > 256 and ((cnt > 0) & (cnt <= 64)).any()
        assert f["touched"].max() >= 4
    if case["name"] == "opaque":  # (c)
        assert np.count_nonzero(g["opacities"] == 1.0) > 0
        assert case["r64"]["clamped"] >= 1 and case["r64"]["stopped"] >= 1
    view = np.asarray(case["ubo"].view, np.float64).reshape(4, 4).T
    listed = np.zeros(len(g["means"]), bool)
    listed[f["vals"][:f["K"]]] = True
    gr, tiles = case["r64"]["grads"], case["r64"]["tiles"]
    if case["name"] in ("posed", "clamp", "chunks", "deep", "deep_stop"):
        # a general view: all nine entries of the rotation and the translation are non-zero
        assert np.abs(view[:3, :3]).min() > 0.1 and np.abs(view[:3, 3]).min() > 0.1
    if case["name"] == "posed":  # (e)
        assert W % 16 and H % 16 and grid[:, -1].max() > 0 and grid[-1, :].max() > 0
        zero_o, small_q = 11, 23
        assert g["opacities"][zero_o] == 0.0 and listed[zero_o] and f["radii"][zero_o] > 0
        for k in R.GRAD_KEYS:  # a Gaussian of opacity 0.0: exactly zero, everywhere
            assert not np.any(gr[k][zero_o]) and not np.any(case["r32"]["grads"][k][zero_o])
        assert np.linalg.norm(g["rotations"][small_q]) < 0.01 and listed[small_q]
        assert np.isfinite(gr["rotations"][small_q]).all() and np.linalg.norm(gr["rotations"][small_q]) > 0
    if case["name"] == "clamp":  # (f)
        cx, cy = R.ewa_clamped(g, case["ubo"], f)
        assert (cx & ~cy).sum() >= 2 and (cy & ~cx).sum() >= 2 and (cx & cy).sum() >= 1
        both = np.flatnonzero(cx | cy)
        assert listed[both].all() and (np.linalg.norm(gr["means"][both], axis=1) > 0).all()
    if case["name"] == "chunks":  # (g)
        for (tx, ty), want in R.CHUNK_TILES.items():
            t = tiles[ty * gx + tx]
            assert grid[ty, tx] == want == t["n"]
            assert (t["first"] == t["n"]).any()  # a pixel that walks the whole list
            assert t["quads"][-1] != 0  # the last entry (a chunk or a batch of its own in 65, 257) contributes
            single = np.isin(t["quads"], (1, 2, 4, 8))
            assert single.sum() >= 8 and (~single & (t["quads"] != 0)).sum() >= 8  # one quadrant only / several
        assert sorted(cnt[cnt > 0]) == sorted(R.CHUNK_TILES.values())
        assert (f["touched"][f["radii"] > 0] == 1).all()  # every Gaussian touches its own tile only
    if case["name"] == "deep":  # (h)
        walk = tiles[R.DEEP_WALK_TILE[1] * gx + R.DEEP_WALK_TILE[0]]
        assert walk["n"] > 512 and (walk["first"] >= 512).any() and walk["quads"][512:].any()  # three batches walked
        mixed = tiles[R.DEEP_MIXED_TILE[1] * gx + R.DEEP_MIXED_TILE[0]]
        assert mixed["n"] > 256 and (mixed["first"] < 256).any()  # pixels that stop inside the first batch ...
        assert (mixed["first"] >= 256).any() and mixed["quads"][256:].any()  # ... and pixels that walk into the second
    if case["name"] == "deep_stop":  # (i)
        assert len(tiles) == 1 and tiles[0]["n"] > 256
        assert len(tiles[0]["first"]) == 256 and tiles[0]["first"].max() < 256  # every pixel stops in the first batch


@pytest.fixture(scope="module")
def project_backward_bin(tmp_path_factory):
    """csrc/splat_backward_math.h compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("pbh") / "project_backward_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "project_backward_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_projection_backward_on_the_host(case, project_backward_bin, tmp_path):
    """The per-Gaussian projection backward (the function the GPU kernel calls), built for the host and fed the
    reference's dL/d(means2d, conic): dL/d(means, scales, rotations) within max(1e-4, 8 e32) of the reference, per
    array and on each of splat_grad_ref.subsets (the quarters by gradient norm, the Gaussians beyond the EWA clamp),
    e32 taken on the same rows."""
    _host_projection_backward(case, project_backward_bin, tmp_path)


def _host_projection_backward(case, project_backward_bin, tmp_path):
    g, W, H, u = case["g"], case["W"], case["H"], case["ubo"]
    view, proj = np.array(u.view, np.float32), np.array(u.proj, np.float32)
    mvp = (proj.reshape(4, 4).T @ view.reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    p00, p11 = float(proj[0]), float(proj[5])
    cam = view.tobytes() + mvp.tobytes() + struct.pack("<ffffIII", p00 * W * 0.5, p11 * H * 0.5, 1.3 / p00,
                                                       1.3 / abs(p11), W, H, (W + 15) // 16)
    vis = np.flatnonzero(case["frame"]["radii"] > 0)
    gr = case["r64"]["grads"]
    rows = np.concatenate([g["means"][vis], g["scales"][vis], g["rotations"][vis], gr["means2d"][vis],
                           gr["conics"][vis]], 1).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(cam + struct.pack("<I", len(vis)) + rows.tobytes())
    r = subprocess.run([project_backward_bin, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 10)
    assert np.isfinite(out).all()
    failed = []
    for k, sl in (("means", slice(0, 3)), ("scales", slice(3, 6)), ("rotations", slice(6, 10))):
        full = np.zeros(gr[k].shape, np.float64)  # (culled Gaussians: zero, as in the reference)
        full[vis] = out[:, sl]
        failed += R.check_bounds(case, k, full, "host projection backward")  # the whole array and every subset
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------
# the frame cases (splat_grad_ref.FRAME_CASES): training-size frames whose borderline pixels take no part
# ---------------------------------------------------------------------------------------------------------
GS_MID, GS_FUSED_MAX_SCAP, GS_FUSED_RUNS_PER_TILE = 512, 2048, 32  # csrc/splat_plan.h


@pytest.fixture(scope="module", params=sorted(R.FRAME_CASES))
def frame_case(request, oracle_lib):
    return R.frame_case_reference(request.param, oracle_lib)


def test_frame_case_structure(frame_case):
    """What the GPU tests rely on, from the oracle's frame: the list lengths that decide the front end and the
    sorts, the tile grid's extent, the pixels that stop and the pairs blended at 0.99."""
    c, name = frame_case, frame_case["name"]
    f, W, H = c["frame"], c["W"], c["H"]
    gx, gy = (W + 15) // 16, (H + 15) // 16
    grid = _counts(c).reshape(gy, gx)
    n, largest = len(c["g"]["means"]), int(grid.max())
    per_tile = R.touched_runs(f, W, H) / (gx * gy)
    print(f"{name}: {W}x{H}, {gx}x{gy} tiles, n {n}, K {f['K']}, longest list {largest}, lists above 256 / {GS_MID} / "
          f"1024: {(grid > 256).sum()} / {(grid > GS_MID).sum()} / {(grid > 1024).sum()}, touched runs per tile "
          f"{per_tile:.2f}, stopped {c['r64']['stopped']}, clamped {c['r64']['clamped']}, "
          f"projection workgroups {(n + 255) // 256}")
    assert f["K"] == int(grid.sum()) and any(v != 0.0 for v in c["bg"])
    assert per_tile <= GS_FUSED_RUNS_PER_TILE  # the policy asks for the fused front end
    if name == "crowd":  # above the fused rows' capacity (gs_plan_scap): three launches on every frame
        assert largest + largest // 4 > GS_FUSED_MAX_SCAP
        assert largest > 8 * 256 and (grid > 1024).sum() >= 2  # more than eight staged batches
    else:  # the second frame of a context is fused
        assert max(256, largest + largest // 4) <= GS_FUSED_MAX_SCAP
    if name in ("field", "layers"):
        assert largest > GS_MID and (grid > GS_MID).sum() >= 2  # the next frame plans the large-tile sort
        assert (grid > 256).sum() > (grid > GS_MID).sum()  # and lists sorted inside the blend remain
        assert per_tile <= 8  # (the host's tile order: well inside the policy's limit)
    if name == "field":
        assert (gx, gy) == (20, 12) and H % 16 and grid[-1].max() > 0  # the bottom row partial and populated
        assert f["K"] > 30000 and largest > 3 * 256  # more than three staged batches
        assert (n + 255) // 256 > 4 and (f["radii"] > 0).sum() > 4 * 256  # the projection backward's workgroups
    if name == "layers":
        assert np.count_nonzero(c["g"]["opacities"] == 1.0) > 1000
        stopped = sum(int((t["first"] < t["n"]).any()) for t in c["r64"]["tiles"])
        assert c["r64"]["stopped"] > 1000 and stopped > 16  # pixels that stop: in quantity, in many tiles
        assert c["r64"]["clamped"] > 100
    if name == "wide":
        assert (gx, gy) == (125, 3) and W % 16 == 8
        assert grid[:, gx - 2].max() >= 257  # the last full tile column: a second staged batch
        assert grid[:, gx - 1].max() > 0  # the partial tile column
        assert grid[:, 64:].max() > 0 and grid[:, 63].max() > 0 and grid[:, 0].max() > 0
    if name == "tall":
        assert (gx, gy) == (3, 69) and H % 16 == 8
        assert grid[gy - 1].max() >= 257 and grid[gy - 2].max() >= 257  # the last (partial) tile row, the last full one
        assert grid[64:].max() > 0 and grid[0].max() > 0
    if name in ("wide", "tall"):
        view = np.asarray(c["ubo"].view, np.float64).reshape(4, 4).T
        assert np.abs(view[:3, :3]).min() > 0.1 and np.abs(view[:3, 3]).min() > 0.1  # a general view


def test_frame_case_mask(frame_case):
    """The masked share is at most 1% of the pixels (a cap), the upstream gradient is exactly 0 there, and the
    float64 reference reports no borderline decision on a pixel with a non-zero upstream gradient."""
    c = frame_case
    share = float(c["mask"].mean())
    print(f"{c['name']}: masked {int(c['mask'].sum())} of {c['mask'].size} pixels ({100 * share:.2f}%), borderline "
          f"decisions {c['r64']['borderline']} (float32 run: {c['r32']['borderline']})")
    assert c["mask"].shape == (c["H"], c["W"]) and share <= R.MASK_CAP
    assert not np.any(c["dL"][c["mask"]]) and np.all(np.any(c["dL"][~c["mask"]] != 0.0, -1))
    live = np.any(c["dL"] != 0.0, -1)
    assert not np.any(c["r64"]["border_pixels"] & live)
    assert np.array_equal(c["r64"]["border_pixels"], c["mask"])  # (the decisions do not depend on dL)
    assert (c["r64"]["borderline"] > 0) == bool(c["mask"].any())


def test_frame_reference_image_matches_the_oracle(frame_case):
    keep = ~frame_case["mask"]
    err = R.rel_l2(frame_case["r64"]["image"][keep], frame_case["frame"]["image"][keep])
    print(f"{frame_case['name']}: float64 reference vs oracle image outside the mask rel L2 {err:.2e}")
    assert err < 1e-4, err


def test_frame_float32_reference_error(frame_case):
    """e32 per key: printed. The GPU bound max(1e-4, 8 e32) follows it, also where float32 resolves a pixel
    coordinate to 1.2e-4 only."""
    for k in R.GRAD_KEYS:
        ref = frame_case["r64"]["grads"][k]
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
        assert np.isfinite(frame_case["r32"]["grads"][k]).all()
        print(f"{frame_case['name']} {k}: e32 {R.rel_l2(frame_case['r32']['grads'][k], ref):.2e}")


def test_projection_backward_on_the_host_frames(frame_case, project_backward_bin, tmp_path):
    """test_projection_backward_on_the_host on the frame cases: up to 20000 Gaussians, 2D means up to 2000 px."""
    _host_projection_backward(frame_case, project_backward_bin, tmp_path)


def test_backward_entry_point_is_exported(native_lib):
    assert hasattr(native_lib, "ptgs_splat_gaussians_backward")
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_splat_gaussians_backward(None, None, None, 1, 1, None, None, None, None) == -1
