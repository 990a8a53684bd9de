"""The depth supervision's reference (tests/splat_depth_ref.py), checked without a GPU: its inverse depth is the
colour blend of 1 / d, the upstream inverse-depth gradient is large enough for the depth part of the gradients to
show, the cases hold no borderline decision, the loss restatement matches a float64 autograd of the masked formula,
the projection backward's depth term built for the host matches the reference, and the native library exports the
three entry points."""
import os
import struct
import subprocess

import numpy as np
import pytest

import splat_depth_ref as Z
import splat_grad_ref as R

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=sorted(R.CASES))
def case(request, oracle_lib):
    return Z.case_reference(request.param, oracle_lib)


def test_invdepth_is_the_colour_blend_of_inverse_depth(case):
    """With colours (1/d, 1/d, 1/d) and a zero background, the image of splat_grad_ref.evaluate is D."""
    g, W, H = case["g"], case["W"], case["H"]
    d = Z.view_depth(torch.tensor(g["means"].astype(np.float64)), case["ubo"].view, torch.float64).numpy()
    vis = case["frame"]["radii"] > 0
    assert (d[vis] > 0.2).all()
    cols = np.zeros((len(d), 3), np.float64)
    cols[vis] = (1.0 / d[vis])[:, None]
    img = R.evaluate(dict(g, colors=cols), case["ubo"], W, H, (0.0, 0.0, 0.0), case["frame"], case["dL"])["image"]
    D = case["r64"]["invdepth"]
    assert D.max() > 0.05
    for ch in range(3):
        assert np.abs(img[..., ch] - D).max() < 1e-12
    # the colour image of the restatement is splat_grad_ref's own
    assert np.abs(case["r64"]["image"] - R.evaluate(g, case["ubo"], W, H, case["bg"], case["frame"],
                                                    case["dL"])["image"]).max() < 1e-12
    assert not np.any(D[case["r64"]["empty"]])
    if case["name"] == "edges":
        assert case["r64"]["empty"].any()


def test_depth_gradient_is_not_hidden_by_the_colour(case):
    """The depth-only gradient of the means is within 10x of the colour-only one, and the colour-only gradients
    are splat_grad_ref's."""
    gc, gd, base = case["r64"]["grads_color"], case["r64"]["grads_depth"], R._CACHE[case["name"]]["r64"]["grads"]
    ratio = np.linalg.norm(gd["means"]) / np.linalg.norm(gc["means"])
    print(f"{case['name']}: |d means| depth / colour {ratio:.3f}")
    assert 0.1 < ratio < 10.0
    for k in R.GRAD_KEYS:
        assert R.rel_l2(gc[k], base[k]) < 1e-12, k
        assert np.linalg.norm(gd[k]) > 0 or k == "colors"
        assert R.rel_l2(gc[k] + gd[k], case["r64"]["grads"][k]) < 1e-12, k
    assert not np.any(gd["colors"]) and not np.any(gc["invd"]) and np.linalg.norm(gd["invd"]) > 0


def test_no_borderline_decisions(case):
    assert case["r64"]["borderline"] == 0 and case["r32"]["borderline"] == 0
    assert case["r32"]["clamped"] == case["r64"]["clamped"] and case["r32"]["stopped"] == case["r64"]["stopped"]


def test_float32_reference_error(case):
    """e32 of the full and of the depth-only gradients: the GPU bound is max(1e-4, 8 e32)."""
    for which in ("grads", "grads_depth"):
        for k in R.GRAD_KEYS:
            ref = case["r64"][which][k]
            if which == "grads_depth" and k == "colors":
                continue
            e32 = R.rel_l2(case["r32"][which][k], ref)
            print(f"{case['name']} {which} {k}: e32 {e32:.2e}")
            assert np.isfinite(ref).all() and e32 < 1e-4


def _loss_case():
    rng = np.random.default_rng(77)
    H, W = 29, 37
    t = rng.uniform(0.5, 12.0, (H, W)).astype(np.float32)
    D = (1.0 / t + rng.normal(scale=0.05, size=(H, W))).astype(np.float32)
    t[0, 0], t[3, 5], t[7, 11], t[28, 36] = 0.0, -2.5, np.nan, np.inf
    t[10, 10], D[10, 10] = 2.0, 0.5  # an exact tie
    t[11, 3] = np.inf
    t[12, :4] = -1.0
    return D, t


def test_loss_restatement_against_float64_autograd():
    D, t = _loss_case()
    weight, scale = 0.7, 3.0
    terms, grad = Z.invdepth_l1(D, t, weight, scale)
    Dt = torch.tensor(D.astype(np.float64), requires_grad=True)
    tt = torch.tensor(t.astype(np.float64))
    sup = tt > 0
    inv = torch.where(sup, 1.0 / torch.where(sup, tt, torch.ones_like(tt)), torch.zeros_like(tt))
    mean = (torch.where(sup, (Dt - inv).abs(), torch.zeros_like(Dt))).sum() / D.size
    (scale * weight * mean).backward()
    m64 = float(mean.detach())
    assert int(sup.sum()) == terms[2] == D.size - 7
    assert abs(terms[1] - m64) < 1e-6 * m64 and abs(terms[0] - weight * m64) < 1e-6 * m64
    g64 = Dt.grad.numpy()
    assert np.abs(grad - g64).max() < 1e-6 * np.abs(g64).max()
    assert np.isfinite(terms).all() and np.isfinite(grad).all()
    for y, x in ((0, 0), (3, 5), (7, 11), (10, 10), (12, 2)):  # unsupervised pixels and the tie: exactly 0
        assert grad[y, x] == 0.0 and g64[y, x] == 0.0
    assert grad[28, 36] == np.float32(weight * scale / D.size) * np.sign(D[28, 36])  # a miss: the target is 0


@pytest.fixture(scope="module")
def project_backward_depth_bin(tmp_path_factory):
    """csrc/splat_backward_math.h with DEPTH compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("pbdh") / "project_backward_depth_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "project_backward_depth_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("which", ["grads", "grads_depth"])
def test_projection_backward_depth_on_the_host(case, project_backward_depth_bin, tmp_path, which):
    """gs_project_backward_one<true> on the host, fed the reference's dL/d(means2d, conic, 1/d): dL/d(means, scales,
    rotations) within max(1e-4, 8 e32) of the reference on the whole array and on each subset, for the full
    gradients and for the depth part alone."""
    _host_projection_backward_depth(case, project_backward_depth_bin, tmp_path, which)


def _host_projection_backward_depth(case, project_backward_depth_bin, tmp_path, which):
    g, W, H, u = case["g"], case["W"], case["H"], case["ubo"]
    view, proj = np.array(u.view, np.float32), np.array(u.proj, np.float32)
    mvp = (proj.reshape(4, 4).T @ view.reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    p00, p11 = float(proj[0]), float(proj[5])
    cam = view.tobytes() + mvp.tobytes() + struct.pack("<ffffIII", p00 * W * 0.5, p11 * H * 0.5, 1.3 / p00,
                                                       1.3 / abs(p11), W, H, (W + 15) // 16)
    vis = np.flatnonzero(case["frame"]["radii"] > 0)
    c = Z.part(case, which)
    gr = c["r64"]["grads"]
    rows = np.concatenate([g["means"][vis], g["scales"][vis], g["rotations"][vis], gr["means2d"][vis],
                           gr["conics"][vis], gr["invd"][vis, None]], 1).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(cam + struct.pack("<I", len(vis)) + rows.tobytes())
    r = subprocess.run([project_backward_depth_bin, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 10)
    assert np.isfinite(out).all()
    failed = []
    for k, sl in (("means", slice(0, 3)), ("scales", slice(3, 6)), ("rotations", slice(6, 10))):
        full = np.zeros(gr[k].shape, np.float64)
        full[vis] = out[:, sl]
        failed += R.check_bounds(c, k, full, f"host projection backward, {which}")
    assert not failed, failed


# ---------------------------------------------------------------------------------------------------------
# the frame cases (splat_grad_ref.FRAME_CASES): both upstream gradients are exactly 0 on the borderline pixels
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=sorted(R.FRAME_CASES))
def frame_case(request, oracle_lib):
    return Z.frame_case_reference(request.param, oracle_lib)


def test_frame_case_mask(frame_case):
    """This module's evaluate() marks the pixels splat_grad_ref masked; dL and dinv are exactly 0 there and
    nowhere else; the share is at most 1%; no borderline decision is left on a pixel with a non-zero gradient."""
    c = frame_case
    base = R.frame_case_reference(c["name"], None)  # (cached by the fixture)
    assert np.array_equal(c["r64"]["border_pixels"], c["mask"]) and np.array_equal(c["mask"], base["mask"])
    assert float(c["mask"].mean()) <= R.MASK_CAP
    assert not np.any(c["dL"][c["mask"]]) and not np.any(c["dinv"][c["mask"]])
    live = np.any(c["dL"] != 0.0, -1) | (c["dinv"] != 0.0)
    assert np.array_equal(live, ~c["mask"]) and not np.any(c["r64"]["border_pixels"] & live)
    assert c["r64"]["borderline"] == base["r64"]["borderline"]
    assert c["r64"]["clamped"] == base["r64"]["clamped"] and c["r64"]["stopped"] == base["r64"]["stopped"]


def test_frame_reference_maps(frame_case):
    """Outside the mask the colour image is the oracle's (< 1e-4) and splat_grad_ref's; D is non-zero; the
    colour-only gradients are splat_grad_ref's and the depth-only ones are not hidden by them."""
    c = frame_case
    base = R.frame_case_reference(c["name"], None)
    keep = ~c["mask"]
    err = R.rel_l2(c["r64"]["image"][keep], c["frame"]["image"][keep])
    print(f"{c['name']}: float64 reference vs oracle image outside the mask rel L2 {err:.2e}")
    assert err < 1e-4 and np.abs(c["r64"]["image"] - base["r64"]["image"]).max() < 1e-12
    assert c["r64"]["invdepth"].max() > 0.05 and not np.any(c["r64"]["invdepth"][c["r64"]["empty"]])
    gc, gd = c["r64"]["grads_color"], c["r64"]["grads_depth"]
    ratio = np.linalg.norm(gd["means"]) / np.linalg.norm(gc["means"])
    print(f"{c['name']}: |d means| depth / colour {ratio:.3f}")
    assert 0.1 < ratio < 10.0
    for k in R.GRAD_KEYS:
        assert R.rel_l2(gc[k], base["r64"]["grads"][k]) < 1e-12, k
        assert R.rel_l2(gc[k] + gd[k], c["r64"]["grads"][k]) < 1e-12, k


def test_frame_float32_reference_error(frame_case):
    """e32 of the full and of the depth-only gradients, per key: printed (the GPU bound follows it)."""
    for which in ("grads", "grads_depth"):
        for k in R.GRAD_KEYS:
            if which == "grads_depth" and k == "colors":
                continue
            ref = frame_case["r64"][which][k]
            assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
            assert np.isfinite(frame_case["r32"][which][k]).all()
            print(f"{frame_case['name']} {which} {k}: e32 {R.rel_l2(frame_case['r32'][which][k], ref):.2e}")


@pytest.mark.parametrize("which", ["grads", "grads_depth"])
def test_projection_backward_depth_on_the_host_frames(frame_case, project_backward_depth_bin, tmp_path, which):
    """test_projection_backward_depth_on_the_host on the frame cases."""
    _host_projection_backward_depth(frame_case, project_backward_depth_bin, tmp_path, which)


def test_depth_entry_points_are_exported(native_lib):
    for name in ("ptgs_splat_gaussians_invdepth", "ptgs_splat_gaussians_backward_depth",
                 "ptgs_image_loss_invdepth_l1"):
        assert hasattr(native_lib, name)
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_splat_gaussians_invdepth(None, 1, 1, None, None) == -1
    assert native_lib.ptgs_splat_gaussians_backward_depth(None, None, None, 1, 1, None, None, None, None, None) == -1
    assert native_lib.ptgs_image_loss_invdepth_l1(None, None, None, 1, 1, 1.0, 1.0, None, None, None) == -1
