"""The reference of the SH colour's backward (tests/sh_grad_ref.py) and its cases, checked without a GPU: the
float32 run of the torch restatement is the forward's numpy restatement bit for bit, the cases decide their
clamps alike in float64 and float32 and far from the threshold, csrc/splat_sh_math.h built for the host matches
the bit-exact part of the contract and the float64 reference, and the native library exports the entry points."""
import os
import struct
import subprocess

import numpy as np
import pytest

import sh_grad_ref as S
import test_splat_sh_gpu as T

torch = pytest.importorskip("torch")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
IDS = [f"d{d}-n{n}-a{a}" for d, n, a in S.CASES]


@pytest.fixture(scope="module", params=S.CASES, ids=IDS)
def case(request):
    return S.case_reference(request.param)


def test_float32_reference_is_the_forward_restatement(case):
    deg, count, active = case["case"]
    ref = T.ref_sh_colors(case["means"], case["sh"][:, :(active + 1) ** 2, :], S.CAM, active)
    assert np.array_equal(case["r32"]["colors"].astype(F), ref)
    # and so is the numpy restatement the bit-exact checks are built on
    res = S.np_res(case["sh"], S.np_factors(case["means"], S.CAM, active, (deg + 1) ** 2))
    assert np.array_equal(np.where(res < 0, F(0), res), ref)
    assert np.array_equal(case["np_clamped"], case["r32"]["res"] < 0)


def test_clamp_decisions_are_not_borderline(case):
    """Conditions on the seeds, not tolerances."""
    deg, count, active = case["case"]
    c64, c32 = case["r64"]["res"] < 0, case["r32"]["res"] < 0
    margin = float(np.abs(case["r64"]["res"]).min())
    print(f"{case['case']}: {int(c64.sum())} clamped of {c64.size}, {int((c64 != c32).sum())} flips, "
          f"min |res + 0.5| {margin:.2e}")
    assert np.array_equal(c64, c32)
    assert margin > 1e-5
    if deg >= 1:
        assert c64.any() and not c64.all()
    all3 = c64.all(axis=1)
    if active >= 2:
        assert all3.any()  # Gaussians with every channel clamped: an exactly zero means gradient
    assert not np.any(case["r64"]["dmeans"][all3]) and not np.any(case["r64"]["dsh"][all3])


def test_float32_reference_error(case):
    """e32 of the float32 run against the float64 run: the bound of the host and GPU tests is max(1e-4, 8 e32)."""
    deg, count, active = case["case"]
    e = S.rel_l2(case["r32"]["dsh"], case["r64"]["dsh"])
    print(f"{case['case']} dsh: e32 {e:.2e}")
    assert e < 1e-6
    assert not np.any(case["r64"]["dsh"][:, (active + 1) ** 2:, :])  # the bands above the active degree
    if active >= 1:
        ref = case["r64"]["dmeans"]
        assert np.isfinite(ref).all() and np.linalg.norm(ref) > 0
        for name, idx in [("all", np.arange(count))] + S.quarters(ref):
            if np.any(ref[idx]):
                e = S.rel_l2(case["r32"]["dmeans"][idx], ref[idx])
                print(f"{case['case']} dmeans {name}: e32 {e:.2e}")
                assert e < 1e-5
    else:
        assert not np.any(case["r64"]["dmeans"])  # the DC band does not see the direction


@pytest.fixture(scope="module")
def sh_backward_bin(tmp_path_factory):
    """csrc/splat_sh_math.h compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("shb") / "sh_backward_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "sh_backward_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run_host(exe, tmp_path, c, in_place):
    deg, count, active = c["case"]
    blob = struct.pack("<IIII", count, deg, active, int(in_place)) + np.asarray(S.CAM, F).tobytes()
    blob += c["means"].tobytes() + c["sh"].tobytes() + c["dcol"].tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / "out.bin", F)
    K = (deg + 1) ** 2
    assert out.size == count * (3 * K + 6)
    return (out[:count * K * 3].reshape(count, K, 3), out[count * K * 3:count * (K * 3 + 3)].reshape(count, 3),
            out[count * (K * 3 + 3):].reshape(count, 3))


def _check_host(c, dsh, dmeans, colors):
    deg, count, active = c["case"]
    assert np.isfinite(dsh).all() and np.isfinite(dmeans).all()
    assert np.array_equal(colors, T.ref_sh_colors(c["means"], c["sh"][:, :(active + 1) ** 2, :], S.CAM, active))
    assert np.array_equal(dsh, c["np_dsh"]), int((dsh != c["np_dsh"]).sum())  # bit for bit
    failed = S.check_bounds(c["r64"]["dmeans"], c["r32"]["dmeans"], dmeans, f"{c['case']} host dmeans")
    assert not failed, failed


@pytest.mark.parametrize("in_place", [False, True])
def test_sh_backward_on_the_host(case, sh_backward_bin, tmp_path, in_place):
    """sh_backward_one (the function the GPU kernel calls), built for the host: dL_dsh equals the numpy float32
    restatement of the contract bit for bit, dL_dmeans is within max(1e-4, 8 e32) of the float64 reference per
    array and per quarter of the Gaussians ranked by gradient norm; writing the row over its own coefficients (as
    the kernel does in LDS) changes nothing."""
    _check_host(case, *_run_host(sh_backward_bin, tmp_path, case, in_place))


def test_sh_backward_on_the_host_at_the_eye(sh_backward_bin, tmp_path):
    c = S.case_reference(S.EYE_CASE, eye=True)
    i = S.EYE_INDEX
    assert np.array_equal(c["means"][i], np.asarray(S.CAM, F))
    dsh, dmeans, colors = _run_host(sh_backward_bin, tmp_path, c, False)
    _check_host(c, dsh, dmeans, colors)
    assert not np.any(c["r64"]["dmeans"][i])  # the select is held fixed: the reference has no gradient there
    assert not np.any(dmeans[i])  # exactly 0 is added
    dres = np.where(c["np_clamped"][i], F(0), c["dcol"][i])
    assert np.array_equal(dsh[i, 0], T.C0 * dres) and np.any(dsh[i, 0])  # the DC row gets its gradient
    assert not np.any(dsh[i, 1:])  # (every other factor is a multiple of x, y or z = 0)


def test_sh_backward_on_the_host_degree0_clamp(sh_backward_bin, tmp_path):
    """The clamp at degree 0, which N(0, 0.5) coefficients do not reach: the same inputs times 8."""
    means, sh, dcol = S.inputs(0, 257)
    sh = sh * F(8)
    want, clamped = S.np_dsh(means, sh, S.CAM, 0, dcol)
    assert clamped.any() and not clamped.all()
    dsh, dmeans, _ = _run_host(sh_backward_bin, tmp_path, {"case": (0, 257, 0), "means": means, "sh": sh, "dcol": dcol},
                               False)
    assert np.array_equal(dsh, want) and not np.any(dmeans)
    assert np.array_equal(dsh[:, 0, :] == 0, clamped)


def test_activation_derivatives_are_those_of_exp_and_sigmoid():
    """The backward uses d exp = exp and d sigmoid = o (1 - o) on the forward's outputs; the forward's expx is
    an exp to about 1e-7 max(1, |x|) relative (its polynomial, plus the rounding of x * log2(e): half an ulp of up
    to 17.3 = 9.5e-7 absolute in the exponent at x = -12, times ln 2), so these differentiate what it computes to
    that accuracy."""
    x = np.linspace(-12.0, 4.0, 4001).astype(F)
    err = np.abs(T.ref_expx(x) / np.exp(x.astype(np.float64)) - 1.0)
    assert (err <= 2e-7 + 7e-8 * np.abs(x)).all(), float(err.max())
    lo = np.linspace(-15.0, 15.0, 4001).astype(F)
    o = (F(1) / (F(1) + T.ref_expx(-lo))).astype(np.float64)
    t = torch.tensor(lo.astype(np.float64), requires_grad=True)
    torch.sigmoid(t).sum().backward()
    # relative to the derivative's scale; near o = 1 the float32 opacity itself limits 1 - o
    np.testing.assert_allclose(o * (1 - o), t.grad.numpy(), rtol=1e-5, atol=1e-7)


def test_backward_entry_points_are_exported(native_lib):
    assert hasattr(native_lib, "ptgs_gaussians_sh_colors_backward")
    assert hasattr(native_lib, "ptgs_gaussians_activate_backward")
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_gaussians_sh_colors_backward(None, None, None, 1, 3, 3, None, None, None, None, None) == -1
    assert native_lib.ptgs_gaussians_activate_backward(None, None, None, 1, None, None, None, None, None) == -1
