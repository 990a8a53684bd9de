"""Reference for the backward of the SH colour (ptgs_gaussians_sh_colors_backward) and of the activations,
independent of the code under test.

torch_colors() restates the colour contract of include/ptgs/ptgs.h in torch, parametrised on the dtype: the same
expressions in the same order, the constants rounded to float32 in either dtype, the two selects (len > 0 and
res + 0.5 < 0) as torch.where on detached conditions. torch.autograd in float64 gives the reference gradients; the
float32 run of the same code gives e32, the error float32 itself makes, from which the bound max(1e-4, 8 e32) of
the GPU and host tests is taken (the pattern of splat_grad_ref.py). np_factors / np_dsh restate the bit-exact part
of the backward contract (dL_dsh = f_k * dL_dres, one float32 multiply) in numpy float32.

Inputs are those of test_splat_sh_gpu._inputs (means ~ N(0, 3), coefficients ~ N(0, 0.5), seed 1000 deg + count,
camera CAM) and an N(0, 1) upstream gradient.
"""
import numpy as np
import torch

import test_splat_sh_gpu as T  # (imports without a GPU: the forward's numpy restatement and its inputs)

F = np.float32
CAM = T.CAM
# (stored degree, count, active degree): the wave (63, 65) and workgroup (257) boundaries, a partial last block
# (1000 = 3 * 256 + 232), every stored degree, fewer active bands than stored
CASES = [(0, 257, 0), (1, 63, 1), (1, 257, 1), (2, 257, 2), (3, 65, 3), (3, 257, 3), (3, 257, 1), (3, 1000, 3)]
EYE_CASE, EYE_INDEX = (3, 65, 3), 7  # the case repeated with Gaussian 7 exactly at the eye

C0, C1 = float(T.C0), float(T.C1)
C2 = [float(v) for v in T.C2]
C3 = [float(v) for v in T.C3]


def inputs(deg, count, eye=False):
    """(means, sh, dL_dcolors) float32, read-only."""
    means, sh = T._inputs(deg, count)
    if eye:
        means = means.copy()
        means[EYE_INDEX] = np.asarray(CAM, F)
        means.setflags(write=False)
    dcol = np.random.default_rng(770000 + 1000 * deg + count).normal(0.0, 1.0, (count, 3)).astype(F)
    dcol.setflags(write=False)
    return means, sh, dcol


class _Sqrt(torch.autograd.Function):
    """A correctly rounded square root in either dtype (numpy's; torch's vectorised float32 sqrt on the CPU is
    not, and the float32 run has to be the contract's IEEE sqrt), with the derivative 1 / (2 sqrt)."""

    @staticmethod
    def forward(ctx, v):
        r = torch.from_numpy(np.sqrt(v.detach().numpy()))
        ctx.save_for_backward(r)
        return r

    @staticmethod
    def backward(ctx, g):
        (r,) = ctx.saved_tensors
        pos = r > 0  # (at 0 the forward's select takes the other branch: no gradient reaches here, and 0 / 0 must not)
        return torch.where(pos, g / (2 * torch.where(pos, r, torch.ones_like(r))), torch.zeros_like(r))


def _direction(means, cam):
    d = means - cam[None, :]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ln = _Sqrt.apply((dx * dx + dy * dy) + dz * dz)
    pos = (ln > 0).detach()
    safe = torch.where(pos, ln, torch.ones_like(ln))
    zero = torch.zeros_like(ln)
    return [torch.where(pos, c / safe, zero) for c in (dx, dy, dz)]


def torch_colors(means, sh, cam, active):
    """(res + 0.5 before the clamp, colour): the contract, term by term, in the tensors' dtype."""
    x, y, z = _direction(means, cam)
    s = lambda k: sh[:, k, :]  # noqa: E731
    col = lambda w: w[:, None]  # noqa: E731
    res = C0 * s(0)
    if active >= 1:
        res = res - col(C1 * y) * s(1) + col(C1 * z) * s(2) - col(C1 * x) * s(3)
    if active >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        res = (res + col(C2[0] * xy) * s(4) + col(C2[1] * yz) * s(5) + col(C2[2] * (2 * zz - xx - yy)) * s(6)
               + col(C2[3] * xz) * s(7) + col(C2[4] * (xx - yy)) * s(8))
    if active >= 3:
        res = (res + col(C3[0] * y * (3 * xx - yy)) * s(9) + col(C3[1] * xy * z) * s(10)
               + col(C3[2] * y * (4 * zz - xx - yy)) * s(11) + col(C3[3] * z * (2 * zz - 3 * xx - 3 * yy)) * s(12)
               + col(C3[4] * x * (4 * zz - xx - yy)) * s(13) + col(C3[5] * z * (xx - yy)) * s(14)
               + col(C3[6] * x * (3 * xx - yy)) * s(15))
    res = res + 0.5
    return res, torch.where((res < 0).detach(), torch.zeros_like(res), res)


def evaluate(means, sh, cam, active, dcol, dtype=torch.float64):
    """{"res", "colors", "dsh", "dmeans"} (numpy float64) of the colour and its gradients given dL_dcolors, with
    every tensor in `dtype`. Coefficient rows above the active bands get gradient 0."""
    m = torch.tensor(np.asarray(means, np.float64), dtype=dtype, requires_grad=True)
    s = torch.tensor(np.asarray(sh, np.float64), dtype=dtype, requires_grad=True)
    c = torch.tensor(np.asarray(cam, F).astype(np.float64), dtype=dtype)  # (the camera is float32 data)
    g = torch.tensor(np.asarray(dcol, np.float64), dtype=dtype)
    res, colors = torch_colors(m, s, c, active)
    (colors * g).sum().backward()
    dm = m.grad if m.grad is not None else torch.zeros_like(m)
    return {"res": res.detach().double().numpy(), "colors": colors.detach().double().numpy(),
            "dsh": s.grad.double().numpy().copy(), "dmeans": dm.double().numpy().copy()}


def np_factors(means, cam, active, K):
    """f [N, K] float32: the factor the forward forms in front of sh[k], each expression as the contract writes
    it (negation is exact); 0 for the bands above `active`."""
    means, cam = np.asarray(means, F), np.asarray(cam, F)
    d = means - cam[None, :]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    ln = np.sqrt((dx * dx + dy * dy) + dz * dz)
    pos = ln > 0
    safe = np.where(pos, ln, F(1))
    x, y, z = (np.where(pos, c / safe, F(0)) for c in (dx, dy, dz))
    f = np.zeros((len(means), K), F)
    c2, c3 = T.C2, T.C3
    f[:, 0] = T.C0
    if active >= 1:
        f[:, 1], f[:, 2], f[:, 3] = -(T.C1 * y), T.C1 * z, -(T.C1 * x)
    if active >= 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        f[:, 4], f[:, 5], f[:, 6] = c2[0] * xy, c2[1] * yz, c2[2] * (F(2) * zz - xx - yy)
        f[:, 7], f[:, 8] = c2[3] * xz, c2[4] * (xx - yy)
    if active >= 3:
        f[:, 9], f[:, 10] = c3[0] * y * (F(3) * xx - yy), c3[1] * xy * z
        f[:, 11] = c3[2] * y * (F(4) * zz - xx - yy)
        f[:, 12] = c3[3] * z * (F(2) * zz - F(3) * xx - F(3) * yy)
        f[:, 13], f[:, 14] = c3[4] * x * (F(4) * zz - xx - yy), c3[5] * z * (xx - yy)
        f[:, 15] = c3[6] * x * (F(3) * xx - yy)
    return f


def np_res(sh, f):
    """res + 0.5 in float32 from the factors: res + f_k sh[k] term by term rounds like the forward's res - w sh[k]
    (the product's sign is exact), so this equals the forward bit for bit (tests/test_sh_grad_ref.py checks it)."""
    sh = np.asarray(sh, F)
    res = f[:, 0, None] * sh[:, 0, :]
    for k in range(1, f.shape[1]):
        if f[:, k].any():
            res = res + f[:, k, None] * sh[:, k, :]
    res = res + F(0.5)
    assert res.dtype == F
    return res


def np_dsh(means, sh, cam, active, dcol):
    """(dL_dsh float32 [N, K, 3], clamped [N, 3] bool): the bit-exact part of the backward contract."""
    sh = np.asarray(sh, F)
    f = np_factors(means, cam, active, sh.shape[1])
    clamped = np_res(sh, f) < 0
    dres = np.where(clamped, F(0), np.asarray(dcol, F))
    out = f[:, :, None] * dres[:, None, :]
    assert out.dtype == F
    return out, clamped


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def quarters(ref, rows=None):
    """[(label, indices)]: each quarter of the rows (default: all) ranked by the norm of the float64 reference
    (q1: the smallest)."""
    rows = np.arange(len(ref)) if rows is None else np.asarray(rows)
    order = rows[np.argsort(np.linalg.norm(ref[rows].reshape(len(rows), -1), axis=1), kind="stable")]
    return [(f"q{i + 1}", part) for i, part in enumerate(np.array_split(order, 4))]


def check_bounds(ref, r32, got, label, rows=None):
    """Relative L2 of `got` against the float64 reference `ref`, on the whole array and on each quarter (of
    `rows`, e.g. the visible Gaussians; default: of all), each
    against max(1e-4, 8 e32) with e32 the float32 reference's error on the same rows. Prints every value; returns
    the failures."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    failed = []
    for name, idx in [("all", np.arange(len(ref)))] + quarters(ref, rows):
        if not np.any(ref[idx]):  # (rows whose reference is exactly zero: so must the result be)
            if np.any(got[idx]):
                failed.append((label, name, "nonzero where the reference is exactly 0"))
            continue
        e32 = rel_l2(r32[idx], ref[idx])
        bound = max(1e-4, 8.0 * e32)
        err = rel_l2(got[idx], ref[idx])
        print(f"{label} {name} ({len(idx)}): rel L2 {err:.2e}  e32 {e32:.2e}  bound {bound:.1e}")
        if not err <= bound:
            failed.append((label, name, err, bound))
    return failed


_CACHE = {}


def case_reference(case, eye=False):
    """The case's inputs, its float64 / float32 reference runs and the numpy restatement (computed once)."""
    key = (tuple(case), eye)
    if key not in _CACHE:
        deg, count, active = case
        means, sh, dcol = inputs(deg, count, eye)
        dsh32, clamped = np_dsh(means, sh, CAM, active, dcol)
        _CACHE[key] = {"case": tuple(case), "means": means, "sh": sh, "dcol": dcol, "np_dsh": dsh32,
                       "np_clamped": clamped,
                       "r64": evaluate(means, sh, CAM, active, dcol, torch.float64),
                       "r32": evaluate(means, sh, CAM, active, dcol, torch.float32)}
    return _CACHE[key]
