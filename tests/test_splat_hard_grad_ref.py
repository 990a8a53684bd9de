"""The gradient reference of the forward's hard cases (tests/splat_hard_grad_ref.py), checked without a GPU. These
are conditions on the cases and the reference, not tolerances: the frame built from splat_forward_ref is the CPU
oracle's, every decision the torch evaluation counts as borderline lies under the forward reference's mask, the mask
stays small, the evaluation renders splat_forward_ref's image and inverse depth, no visible Gaussian sits on the EWA
clamp's threshold, the float32 yardstick is finite and does not blow the bound up, and each case has the structure it
exists for. Then the per-Gaussian projection backward, built for the host with the sanitizers, is held to
splat_grad_ref.check_bounds on every case: the colour, the colour + depth and the depth-only gradients."""
import numpy as np
import pytest

import splat_depth_ref as Z
import splat_grad_ref as R
import splat_hard_grad_ref as HG
from test_splat_depth_ref import _host_projection_backward_depth, project_backward_depth_bin  # noqa: F401
from test_splat_grad_ref import _host_projection_backward, project_backward_bin  # noqa: F401

torch = pytest.importorskip("torch")

BEYOND_WITH_WEIGHT = {"giants": 20, "near": 3, "around": 7, "sizes_1x1": 2}  # observed; asserted as >= 1


@pytest.fixture(scope="module", params=HG.CASES)
def case(request):
    return HG.case_reference(request.param)


def test_the_cases_are_the_forwards():
    assert len(HG.CASES) == 13 and "over" not in HG.CASES and set(HG.CASES) | {"over"} == set(HG.F.CASES)


def test_frame_is_the_oracles(case, oracle_lib):
    """radii > 0 and every tile's list, in order, equal the CPU oracle's (which the GPU comparison does not use)."""
    c = case
    o = oracle_lib.splat_gaussians(c["g"], c["ubo"], c["W"], c["H"], bg=c["bg"])
    f = c["frame"]
    assert np.array_equal(np.asarray(o["radii"]) > 0, f["radii"] > 0)
    ro = np.asarray(o["ranges"]).reshape(-1, 2).astype(np.int64)
    assert len(ro) == len(f["ranges"]) and int(o["K"]) == f["K"]
    for (a, b), (p, q) in zip(ro, f["ranges"]):
        assert np.array_equal(np.asarray(o["vals"][a:b], np.int64), f["vals"][p:q])


def test_mask(case):
    """Both upstream gradients are exactly 0 on the mask and nowhere else, the masked share is at most MASK_CAP, every
    pixel the torch evaluation counts a borderline decision on is masked, and no visible Gaussian lies within
    CLAMP_MARGIN of the EWA clamp without its rectangle being masked."""
    c = case
    share = float(c["mask"].mean())
    outside = int((c["r64"]["border_pixels"] & ~c["mask"]).sum())
    print(f"{c['name']}: masked {int(c['mask'].sum())} of {c['mask'].size} pixels ({100 * share:.2f}%), borderline pixels "
          f"outside the mask {outside}, closest to the clamp {c['clamp_margin']:.1e}, clamp doubts {len(c['clamp_doubt'])}")
    assert c["mask"].shape == (c["H"], c["W"]) and share <= R.MASK_CAP
    assert np.array_equal(c["mask"], c["fwd"]["mask"]) or len(c["clamp_doubt"])
    assert outside == 0
    live = np.all(c["dL"] != 0.0, -1) & (c["dinv"] != 0.0)
    assert np.array_equal(live, ~c["mask"]) and not np.any(c["dL"][c["mask"]]) and not np.any(c["dinv"][c["mask"]])
    assert c["clamp_margin"] > HG.CLAMP_MARGIN or len(c["clamp_doubt"])
    for i in c["clamp_doubt"]:
        x0, y0, x1, y1 = c["fwd"]["r64"]["rect"][i]
        assert c["mask"][y0 * 16:y1 * 16, x0 * 16:x1 * 16].all()


def test_evaluation_renders_the_forward_reference(case):
    keep = ~case["mask"]
    for key in ("image", "invdepth"):
        err = float(np.abs(case["r64"][key] - case["fwd"]["r64"][key])[keep].max()) if keep.any() else 0.0
        print(f"{case['name']} {key}: torch evaluation vs splat_forward_ref outside the mask, max abs {err:.1e}")
        assert err <= 1e-12


def test_float32_yardstick(case):
    """r32 is finite everywhere, and max(1e-4, 8 e32) is at most BOUND_CAP on every (part, key, subset)."""
    worst = (0.0, None)
    for which, _, keys in HG.checked(case):
        p = Z.part(case, which)
        for k in keys:
            ref, r32 = p["r64"]["grads"][k], p["r32"]["grads"][k]
            assert np.isfinite(ref).all() and np.isfinite(r32).all(), (which, k)
            for name, idx in [("all", np.arange(len(ref)))] + R.subsets(p, k):
                bound = max(1e-4, 8.0 * R.rel_l2(r32[idx], ref[idx]))
                worst = max(worst, (bound, (which, k, name)))
                assert bound <= HG.BOUND_CAP, (which, k, name, bound)
    print(f"{case['name']}: largest bound {worst[0]:.1e} at {worst[1]}")
    for key in ("image", "invdepth"):
        assert np.isfinite(case["r32"][key]).all()


def test_case_structure(case):
    c, name = case, case["name"]
    fr, vis = c["fwd"]["r64"], c["frame"]["radii"] > 0
    moved = np.linalg.norm(c["r64"]["grads"]["means"], axis=1) > 0
    if name in BEYOND_WITH_WEIGHT:
        n = int((fr["beyond"].any(1) & vis & (fr["weight"] > 0) & moved).sum())
        print(f"{name}: visible Gaussians beyond the EWA clamp with weight and a gradient: {n}")
        assert n >= 1
        cx, cy = R.ewa_clamped(c["g"], c["ubo"], c["frame"])
        assert np.array_equal(cx | cy, fr["beyond"].any(1) & vis)  # (the "clamped" subset of check_bounds)
    if name == "opacity_edges":
        zero = vis & (c["g"]["opacities"] == 0.0)
        print(f"{name}: visible Gaussians of opacity 0.0: {int(zero.sum())}, pixels that stop {c['r64']['stopped']}")
        assert zero.sum() >= 1 and c["r64"]["stopped"] >= 1
        for which, _, keys in HG.checked(c):
            for k in keys:  # exactly zero in the reference as well
                assert not np.any(c["r64"][which][k][zero]) and not np.any(c["r32"][which][k][zero])
        for o in (1.0 / 255.0, 0.99, 1.0):
            assert (vis & (c["g"]["opacities"] == np.float32(o))).any()
    if name == "needles":
        assert c["r64"]["stopped"] >= 1
        s = c["g"]["scales"][vis]
        assert (s.max(1) / s.min(1) > 200).sum() > 100
    if name == "ties":
        m = c["g"]["means"]
        assert np.array_equal(m[1::2], m[0::2]) and (vis[0::2] & vis[1::2]).sum() > 10
    if name.startswith("sizes_"):
        assert (c["W"], c["H"]) == tuple(int(v) for v in name[6:].split("x"))
    for which, _, keys in HG.checked(c):  # a culled Gaussian has exactly zero gradients
        for k in keys:
            assert not np.any(c["r64"][which][k][~vis])
            assert np.linalg.norm(c["r64"][which][k]) > 0, (which, k)


def test_projection_backward_on_the_host(case, project_backward_bin, tmp_path):
    """gs_project_backward_one on the host, fed the reference's colour-only dL/d(means2d, conic)."""
    _host_projection_backward(Z.part(case, "grads_color"), project_backward_bin, tmp_path)


@pytest.mark.parametrize("which", ["grads", "grads_depth"])
def test_projection_backward_depth_on_the_host(case, project_backward_depth_bin, tmp_path, which):
    """gs_project_backward_one<true> on the host: the colour + depth gradients, and the depth part alone."""
    _host_projection_backward_depth(case, project_backward_depth_bin, tmp_path, which)
