"""The camera-pose gradient's reference (tests/splat_pose_grad_ref.py), checked without a GPU: the chain (blend
cotangents through the projection's VJP) against finite differences of the whole frame, the kernel's per-Gaussian
math built for the host against the reference on every case and block, what the EWA clamp switches off, the depth
part not hidden by the colour part, se3_view, the reference pose descent, and the exported entry points; the same
chain and host math on the forward's hard cases (splat_hard_grad_ref); and the conditions on the inputs of
tests/test_splat_pose_rows_gpu.py: every occupied row, lane and row class of the second-stage sums carries a share of
the reference that the tolerance cannot hide."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sh_grad_ref as S
import splat_grad_ref as R
import splat_hard_grad_ref as HG
import splat_pose_grad_ref as P

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FD_CASES = ("posed", "clamp", "edges", "deep_stop")
FD_HARD_CASES = ("near", "needles")  # splat_hard_grad_ref's: Gaussians cut by the near plane, scale ratios above 200
FD_STEPS = (1e-6, 5e-7)
FD_BOUND = 1e-6  # three decades above what the chain measures against central differences, three below a missing term


@pytest.fixture(scope="module", params=sorted(R.CASES))
def case(request, oracle_lib):
    return P.case_reference(request.param, oracle_lib)


@pytest.fixture(scope="module", params=HG.CASES)
def hard_case(request):
    return P.hard_case_reference(request.param)


@pytest.mark.parametrize("name", FD_CASES + FD_HARD_CASES)
def test_reference_against_finite_differences(oracle_lib, name):
    c = P.hard_case_reference(name) if name in FD_HARD_CASES else P.case_reference(name, oracle_lib)
    ref = c["pose"]["grads"]["r64"]
    assert np.isfinite(ref).all() and np.all(ref != 0.0)  # every entry of the 3x4 takes part
    for step in FD_STEPS:
        fd, border = P.fd_view_grad(c, step)
        err = R.rel_l2(ref, fd)
        print(f"{name}: chain vs central differences at {step:g}: rel L2 {err:.2e}, borderline decisions {border}")
        assert border == 0  # no decision came near its threshold under the perturbation
        assert err <= FD_BOUND


def test_float32_reference_error(case):
    """e32 per part and block: printed, and small enough for the bound max(1e-4, 8 e32) to mean something."""
    for which in P.PARTS:
        for name, idx in P.BLOCKS.items():
            ref = case["pose"][which]["r64"][idx]
            e32 = R.rel_l2(case["pose"][which]["r32"][idx], ref)
            print(f"{case['name']} {which} {name}: |ref| {np.linalg.norm(ref):.3e} e32 {e32:.2e}")
            assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0 and e32 < 1e-4
    full = case["pose"]["grads"]["r64"]
    assert R.rel_l2(case["pose"]["grads_color"]["r64"] + case["pose"]["grads_depth"]["r64"], full) < 1e-12


def test_float32_reference_error_on_the_hard_cases(hard_case):
    """The same on the forward's hard cases: every part and block of the reference is finite and non-zero, and 8 e32
    does not exceed splat_hard_grad_ref.BOUND_CAP (a blown-up float32 yardstick must not hide a failure)."""
    c = hard_case
    for which in P.PARTS:
        for name, idx in P.BLOCKS.items():
            ref, r32 = c["pose"][which]["r64"][idx], c["pose"][which]["r32"][idx]
            e32 = R.rel_l2(r32, ref)
            print(f"{c['name']} {which} {name}: |ref| {np.linalg.norm(ref):.3e} e32 {e32:.2e}")
            assert np.isfinite(ref).all() and np.isfinite(r32).all() and np.linalg.norm(ref) > 0
            assert 8.0 * e32 <= HG.BOUND_CAP
    full = c["pose"]["grads"]["r64"]
    assert R.rel_l2(c["pose"]["grads_color"]["r64"] + c["pose"]["grads_depth"]["r64"], full) < 1e-12


def test_depth_part_is_not_hidden_by_the_colour(case):
    ratio = np.linalg.norm(case["pose"]["grads_depth"]["r64"]) / np.linalg.norm(case["pose"]["grads_color"]["r64"])
    print(f"{case['name']}: |d view| depth / colour {ratio:.3f}")
    assert 0.1 < ratio < 10.0


@pytest.fixture(scope="module")
def project_backward_pose_bin(tmp_path_factory):
    """csrc/splat_backward_math.h with DEPTH and POSE compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("pbph") / "project_backward_pose_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "project_backward_pose_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _host_shares(case, exe, tmp_path, cot):
    """The driver on the case's visible Gaussians with the cotangents `cot`: (vis, [len(vis), 22] float32, the
    printed shares [len(vis), 12] float64)."""
    g, W, H, u = case["g"], case["W"], case["H"], case["ubo"]
    view, proj = np.array(u.view, np.float32), np.array(u.proj, np.float32)
    mvp = (proj.reshape(4, 4).T @ view.reshape(4, 4).T).T.reshape(-1).astype(np.float32)
    p00, p11 = float(proj[0]), float(proj[5])
    cam = view.tobytes() + mvp.tobytes() + struct.pack("<ffffIII", p00 * W * 0.5, p11 * H * 0.5, 1.3 / p00,
                                                       1.3 / abs(p11), W, H, (W + 15) // 16)
    vis = np.flatnonzero(case["frame"]["radii"] > 0)
    rows = np.concatenate([g["means"][vis], g["scales"][vis], g["rotations"][vis], cot["means2d"][vis],
                           cot["conics"][vis], cot["invd"][vis, None]], 1).astype(np.float32)
    (tmp_path / "in.bin").write_bytes(cam + proj.tobytes() + struct.pack("<I", len(vis)) + rows.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", np.float32).reshape(-1, 22)
    printed = np.array([[float(v) for v in line.split()] for line in r.stdout.splitlines()], np.float64)
    assert printed.shape == (len(vis), 12) and np.isfinite(out).all()
    assert np.array_equal(printed.astype(np.float32), out[:, 10:])  # (%.9g round-trips a float32)
    return vis, out, printed


@pytest.mark.parametrize("which", P.PARTS)
def test_projection_backward_pose_on_the_host(case, project_backward_pose_bin, tmp_path, which):
    """gs_project_backward_one<true, true> on the host, fed the reference's cotangents: the float64 sum of the
    Gaussians' twelve shares is dL/d view within max(1e-4, 8 e32) on the whole 3x4, the rotation block and the
    translation column, for the full loss, its colour part and its depth part; dL/d(means, scales, rotations) of
    the same call are those of the DEPTH form."""
    vis, out, printed = _host_shares(case, project_backward_pose_bin, tmp_path, case["r64"][which])
    got = printed.sum(0).reshape(3, 4)
    ref = case["pose"][which]
    failed = P.check_blocks(ref["r64"], ref["r32"], got, f"{case['name']} host projection backward, {which}")
    assert not failed, failed
    import splat_depth_ref as Z
    cz = Z.part(case, which)
    for k, sl in (("means", slice(0, 3)), ("scales", slice(3, 6)), ("rotations", slice(6, 10))):
        full = np.zeros(cz["r64"]["grads"][k].shape, np.float64)
        full[vis] = out[:, sl]
        failed += R.check_bounds(cz, k, full, f"host projection backward with POSE, {which}")
    assert not failed, failed


@pytest.mark.parametrize("which", P.PARTS)
def test_projection_backward_pose_on_the_host_on_the_hard_cases(hard_case, project_backward_pose_bin, tmp_path, which):
    """The same host build on the forward's hard cases (needles, giants, near-plane, sub-pixel, tied and
    opacity-edge Gaussians, 1x1 to 130x9 frames): finite shares (asserted by _host_shares), dL/d view within
    max(1e-4, 8 e32) with 8 e32 capped at BOUND_CAP, the other gradients through check_bounds."""
    import splat_depth_ref as Z
    c = hard_case
    vis, out, printed = _host_shares(c, project_backward_pose_bin, tmp_path, c["r64"][which])
    ref = c["pose"][which]
    failed = P.check_blocks(ref["r64"], ref["r32"], printed.sum(0).reshape(3, 4),
                            f"{c['name']} host projection backward, {which}", cap=HG.BOUND_CAP)
    cz = Z.part(c, which)
    for k, sl in (("means", slice(0, 3)), ("scales", slice(3, 6)), ("rotations", slice(6, 10))):
        full = np.zeros(cz["r64"]["grads"][k].shape, np.float64)
        full[vis] = out[:, sl]
        failed += R.check_bounds(cz, k, full, f"host projection backward with POSE, {which}")
    assert not failed, failed


def test_clamped_gaussians_leave_the_tangent_path(oracle_lib, project_backward_pose_bin, tmp_path):
    """In `clamp`, a Gaussian beyond the EWA clamp in x contributes nothing to view[0][c] through J02 (tx no longer
    depends on x), one beyond it in y nothing to view[1][c] through J12. With the conic's cotangent alone the share
    of view[0][3] (view[1][3]) is exactly that path, dL/d x (dL/d y) of the camera-space point: exactly 0 for the
    clamped Gaussians, in the reference and in the kernel's math, and non-zero for the others."""
    c = P.case_reference("clamp", oracle_lib)
    cx, cy = R.ewa_clamped(c["g"], c["ubo"], c["frame"])
    assert cx.sum() == 4 and cy.sum() == 4 and (cx | cy).sum() == R.CLAMP_WIDE
    vis = np.flatnonzero(c["frame"]["radii"] > 0)
    cot = {"means2d": np.zeros_like(c["r64"]["grads"]["means2d"]), "conics": c["r64"]["grads"]["conics"],
           "invd": np.zeros_like(c["r64"]["grads"]["invd"])}
    assert np.all(np.abs(cot["conics"][cx | cy]).sum(1) > 0)  # the clamped Gaussians do take part in the image
    _, dpv = P.view_grad(c["g"], P.view_matrix(c["ubo"]), c["ubo"].proj, c["W"], c["H"], vis, cot, per_gaussian=True)
    vis2, _, shares = _host_shares(c, project_backward_pose_bin, tmp_path, cot)
    assert np.array_equal(vis, vis2)
    live = np.abs(cot["conics"][vis]).sum(1) > 0
    for axis, clamped in ((0, cx[vis]), (1, cy[vis])):
        assert not np.any(dpv[clamped, axis]) and np.all(dpv[live & ~clamped, axis] != 0.0)
        assert not np.any(shares[clamped, 4 * axis + 3]) and np.all(shares[live & ~clamped, 4 * axis + 3] != 0.0)
        # the rest of that row is the same dL/d x times the mean: the clamped Gaussians keep only J00 dT (J11 dT)
        assert R.rel_l2(shares[~clamped, 4 * axis + 3], dpv[~clamped, axis]) < 1e-4


def test_se3_view():
    from pathtracer_gaussiansplatting_amd import autograd
    rng = np.random.default_rng(5)
    view0 = P.view_matrix(R.make_ubo(44, 40, *R.POSE))
    for dt in (torch.float32, torch.float64):
        v0 = torch.tensor(view0, dtype=dt)
        out = autograd.se3_view(v0, torch.zeros(6, dtype=dt, requires_grad=True))
        assert out.dtype == dt and torch.equal(out, v0)  # the identity at xi = 0, bit for bit
    xi = rng.normal(size=6) * np.array([0.3, 0.3, 0.3, 0.2, 0.2, 0.2])
    got = autograd.se3_view(torch.tensor(view0), torch.tensor(xi)).numpy()
    assert np.abs(got - P.se3_exp(xi) @ view0).max() < 1e-13
    E = P.se3_exp(xi)  # (a rigid motion: the restatement's own check)
    assert np.abs(E[:3, :3] @ E[:3, :3].T - np.eye(3)).max() < 1e-12 and np.array_equal(got[3], [0, 0, 0, 1])
    # a pure translation adds to the view's translation (camera space) and leaves the rotation alone
    shift = torch.tensor([0.1, -0.2, 0.3, 0.0, 0.0, 0.0], dtype=torch.float64)
    t = autograd.se3_view(torch.tensor(view0), shift).numpy()
    assert np.abs(t[:3, 3] - view0[:3, 3] - [0.1, -0.2, 0.3]).max() < 1e-15 and np.array_equal(t[:3, :3], view0[:3, :3])
    # its torch gradient against central differences, float64
    w = rng.normal(size=(4, 4))
    x = torch.tensor(xi, requires_grad=True)
    (autograd.se3_view(torch.tensor(view0), x) * torch.tensor(w)).sum().backward()
    fd = np.zeros(6)
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-6
        fd[k] = ((P.se3_exp(xi + e) @ view0 * w).sum() - (P.se3_exp(xi - e) @ view0 * w).sum()) / 2e-6
    assert R.rel_l2(x.grad.numpy(), fd) < 1e-8
    assert R.rel_l2(P.descent_xi_grad(w[:3], view0, xi), fd) < 1e-8  # (row 3 does not depend on xi)


def test_reference_pose_descent(oracle_lib, capsys):
    """Plain gradient steps with the float64 reference gradient bring `posed` from XI0 to at most 0.25 of the
    initial pose error (the GPU run of the same constants is asked for 0.5)."""
    c = P.case_reference("posed", oracle_lib)
    errs = P.reference_descent(c, oracle_lib, log=print)
    print(f"pose error {errs[0]:.5f} -> {errs[-1]:.5f} ({errs[-1] / errs[0]:.3f}) in {P.STEPS} steps")
    assert len(errs) == P.STEPS + 1 and errs[0] > 0.1
    assert errs[-1] <= 0.25 * errs[0]


def test_pose_entry_points_are_exported(native_lib):
    for name in ("ptgs_splat_gaussians_backward_pose", "ptgs_gaussians_sh_colors_backward_eye"):
        assert hasattr(native_lib, name)
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_splat_gaussians_backward_pose(None, None, None, 1, 1, None, None, None, None, None,
                                                         None) == -1
    assert native_lib.ptgs_gaussians_sh_colors_backward_eye(None, None, None, 1, 0, 0, None, None, None, None, None,
                                                            None) == -1
    assert native_lib.ptgs_abi_version() == 4


# ---- the inputs of tests/test_splat_pose_rows_gpu.py: conditions on the reference alone
def _row_groups(c):
    rows = c["vis"] // 256
    return [np.flatnonzero(rows == r) for r in np.unique(rows)]


@pytest.mark.parametrize("n", (P.ROWS_N,) + P.ROWS_PREFIXES)
def test_rows_every_occupied_row_counts(oracle_lib, n):
    """ROWS and its prefixes: the visible set is the layout and no decision is borderline (rows_reference asserts
    both), and every occupied row's own share of |dL/d view| is at least 1% on each block, so a dropped or doubled
    row is a hundred times the bound."""
    c = P.rows_prefix(n, oracle_lib)
    assert len(c["g"]["means"]) == n and c["borderline"] == 0
    want = [r for r in P.ROWS_AT if r * 256 < n]
    assert np.array_equal(np.unique(c["vis"] // 256), want)
    if n == P.ROWS_N:
        assert len(c["vis"]) == 98 and (n + 255) // 256 == 1281 and n % 256 == 56
    shares = P.block_shares(c, _row_groups(c))
    for name, v in shares.items():
        print(f"{c['name']} {name}: rows' own shares {v.min():.3f} .. {v.max():.3f}")
        assert v.min() >= P.ROW_SHARE_MIN, (name, v)
    for which in P.PARTS:  # the yardstick of the GPU comparison
        for name, idx in P.BLOCKS.items():
            e32 = R.rel_l2(c["pose"][which]["r32"][idx], c["pose"][which]["r64"][idx])
            assert np.linalg.norm(c["pose"][which]["r64"][idx]) > 0 and e32 < 1e-4, (which, name, e32)


def test_rows_reference_is_the_compact_cases(oracle_lib):
    """The culled Gaussians change nothing: the float64 reference of ROWS is that of its 98 visible Gaussians alone."""
    c = P.rows_prefix(P.ROWS_N, oracle_lib)
    k = P.compact_of(c, oracle_lib)
    assert len(k["g"]["means"]) == 98 and np.array_equal(k["g"]["means"], c["g"]["means"][c["vis"]])
    for which in P.PARTS:
        err = R.rel_l2(c["pose"][which]["r64"], k["pose"][which]["r64"])
        print(f"ROWS vs its compact case, {which}: {err:.1e}")
        assert err <= 1e-12


def test_lanes_every_gaussian_counts(oracle_lib):
    """LANES: one visible Gaussian per row, at row j, lane j; each one's own share of |dL/d view| is at least ten
    times the block's bound max(1e-4, 8 e32)."""
    c = P.lanes_reference(oracle_lib)
    assert len(c["g"]["means"]) == P.LANES_N == 256 * 256
    assert np.array_equal(c["vis"] // 256, np.arange(256)) and np.array_equal(c["vis"] % 256, np.arange(256))
    shares = P.block_shares(c, [[i] for i in range(256)])
    for name, idx in P.BLOCKS.items():
        e32 = R.rel_l2(c["pose"]["grads"]["r32"][idx], c["pose"]["grads"]["r64"][idx])
        need = P.LANE_SHARE_FACTOR * max(1e-4, 8.0 * e32)
        print(f"LANES {name}: smallest own share {shares[name].min():.2e}, asked {need:.1e} (e32 {e32:.2e})")
        assert shares[name].min() >= need


@pytest.mark.parametrize("deg,n", sorted(P.EYE_DENSE))
def test_eye_every_row_class_counts(deg, n):
    """The dense eye inputs: every class of rows (row // 1024) has at least EYE_SHARE_MIN of |dL/d eye| with
    EYE_DENSE's factors. A class's share is eye_grad of its Gaussians alone (the others' dcol zeroed: they add exact
    zeros, so they are left out of the evaluation)."""
    means, sh, dcol = P.eye_dense_inputs(deg, n)
    classes = P.eye_classes(n)
    assert len(classes) == ((n + 255) // 256 + 1023) // 1024 and classes[-1][1].stop == n
    total = P.eye_grad(means, sh, S.CAM, deg, dcol)
    parts = [P.eye_grad(means[sl], sh[sl], S.CAM, deg, dcol[sl]) for _, sl in classes]
    assert R.rel_l2(np.sum(parts, 0), total) < 1e-12
    shares = [float(np.linalg.norm(p) / np.linalg.norm(total)) for p in parts]
    print(f"degree {deg}, n {n}: classes' shares " + " ".join(f"{v:.3f}" for v in shares))
    assert min(shares) >= P.EYE_SHARE_MIN


def test_eye_sparse_inputs():
    """One Gaussian per workgroup, at lane row % 256: 4097 of them, every lane used, the last row's inside n."""
    dcol, at = P.eye_sparse_dcol(1, P.EYE_N_STEP)
    assert len(at) == 4097 and np.array_equal(at // 256, np.arange(4097)) and set(at % 256) == set(range(256))
    assert at[-1] < P.EYE_N_STEP and int(np.any(dcol != 0, axis=1).sum()) == 4097
