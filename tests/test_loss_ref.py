"""The float64 reference of the L1 + D-SSIM training loss (tests/loss_ref.py) against torch autograd and central
differences, and csrc/splat_loss_math.h on the host (f32, separable, ASan + UBSan) against the reference. No GPU.

Tolerance of the host restatement (the rule tests/test_loss_gpu.py applies to the kernels): e32 is the error of
the float32 F.conv2d formulation on the CPU against the float64 reference, relative L2 for the gradient and
relative for each term, computed here per case; the restatement must be within 4 * e32 + 1e-7 (the factor for
the separable summation order against the direct one, the floor for cases whose e32 happens to be near zero)."""
import os
import subprocess

import numpy as np
import pytest

import loss_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


@pytest.fixture(scope="module")
def loss_bin(tmp_path_factory):
    """csrc/splat_loss_math.h compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("ls") / "loss_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "loss_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_reference_gradient_against_autograd():
    torch = pytest.importorskip("torch")
    for (H, W), lam in (((13, 17), 0.2), ((3, 7), 1.0), ((24, 12), 0.5)):
        image, target = L.make_inputs(H, W, 3, seed=1)
        loss, l1, ssim, grad = L.loss_and_grad(image, target, lam, 1.5)
        eloss, el1, essim, egrad = L.eager(image, target, lam, 1.5, "float64")
        assert L.rel_l2(grad, egrad) < 1e-12
        assert L.rel(loss, eloss) < 1e-12 and L.rel(l1, el1) < 1e-12 and L.rel(ssim, essim) < 1e-12
        assert not grad[..., 3].any()


def test_reference_gradient_against_central_differences():
    """20 pixels of a 12 x 14 image away from the kink of |a - b|; step 1e-5 in float64: the truncation error is
    O(1e-10) relative and the rounding error 1e-16 / 1e-5 absolute, so 1e-5 relative + 1e-10 absolute is ample."""
    H, W = 12, 14
    image, target = L.make_inputs(H, W, 3, seed=2)
    _, _, _, grad = L.loss_and_grad(image, target, 0.2)
    a, b = image.astype(np.float64), target.astype(np.float64)
    rng = np.random.default_rng(5)
    cand = np.argwhere(np.abs(a[..., :3] - b) > 1e-3)
    h = 1e-5
    for y, x, c in cand[rng.choice(len(cand), 20, replace=False)]:
        hi, lo = a.copy(), a.copy()
        hi[y, x, c] += h
        lo[y, x, c] -= h
        fd = (L.loss_only(hi, b) - L.loss_only(lo, b)) / (2 * h)
        assert abs(fd - grad[y, x, c]) <= 1e-5 * abs(grad[y, x, c]) + 1e-10, (y, x, c, fd, grad[y, x, c])


def test_equal_images():
    """image == target: loss 0, ssim 1, and a gradient that is zero up to the rounding of terms that cancel
    (each O(100 / n) before the cancellation)."""
    image, _ = L.make_inputs(19, 23, 3, seed=3)
    loss, l1, ssim, grad = L.loss_and_grad(image, image[..., :3].copy(), 0.2)
    assert l1 == 0.0 and ssim == 1.0 and loss == 0.0
    assert np.abs(grad).max() < 1e-13


def test_window_literals(loss_bin):
    r = subprocess.run([loss_bin, "window"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([float.fromhex(s) for s in r.stdout.split()])
    assert got.shape == (11,)
    assert np.array_equal(got.astype(F), L.window().astype(F)) and np.array_equal(got, got.astype(F).astype(np.float64))


def _run_host(exe, tmp_path, image, target, lam, grad_scale):
    H, W, C = target.shape
    blob = np.array([H, W, C], np.uint32).tobytes() + np.array([lam, grad_scale], F).tobytes()
    (tmp_path / "in.bin").write_bytes(blob + image.tobytes() + target.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", F)
    assert raw.size == 4 + H * W * 4
    return raw[:4].astype(np.float64), raw[4:].reshape(H, W, 4).astype(np.float64)


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (16, 16), (35, 67)])
@pytest.mark.parametrize("C", [3, 4])
def test_host_math_against_the_reference(loss_bin, tmp_path, shape, C):
    pytest.importorskip("torch")
    image, target = L.make_inputs(*shape, C, seed=4)
    p = L.parts(image, target)
    for lam, gs in ((0.2, 1.0), (1.0, 2.5), (0.0, 1.0)):
        lam = float(F(lam))  # (the value the f32 argument carries)
        ref = L.combine(p, lam, gs)
        e32 = L.eager(image, target, lam, gs, "float32")
        terms, grad = _run_host(loss_bin, tmp_path, image, target, lam, gs)
        assert terms[3] == 0.0 and not grad[..., 3].any()
        for k, name in enumerate(("loss", "l1", "ssim")):
            err, bound = L.rel(terms[k], ref[k]), 4 * L.rel(e32[k], ref[k]) + 1e-7
            print(f"{shape} C={C} lam={lam:.1f} {name}: {err:.2e} (bound {bound:.2e})")
            assert err <= bound, (name, err, bound)
        err, bound = L.rel_l2(grad, ref[3]), 4 * L.rel_l2(e32[3], ref[3]) + 1e-7
        print(f"{shape} C={C} lam={lam:.1f} grad: {err:.2e} (bound {bound:.2e})")
        assert err <= bound, (err, bound)


def test_loss_entry_point_is_exported(native_lib):
    assert hasattr(native_lib, "ptgs_image_loss_l1_dssim")
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_image_loss_l1_dssim(None, None, None, 3, 1, 1, 0.2, 1.0, None, None, None) == -1


def test_python_layer_is_exported():
    import pathtracer_gaussiansplatting_amd as P
    assert callable(P.Renderer.l1_dssim_loss) and callable(P.autograd.l1_dssim) and P.l1_dssim is P.autograd.l1_dssim
    assert "l1_dssim" in P.__all__
