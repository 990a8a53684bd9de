"""The camera-pose gradient on the GPU: ptgs_splat_gaussians_backward_pose and ptgs_gaussians_sh_colors_backward_eye
against the float64 references of tests/splat_pose_grad_ref.py, the reduction's boundaries, culled and empty frames,
the error paths, and torch.autograd through view= and se3_view.

Tolerances are the project's: max(1e-4, 8 e32) relative L2 per block of dL/d view (the whole 3x4, the rotation
block, the translation column; e32 from the float32 run of the reference) and per gradient array and subset
(splat_grad_ref.check_bounds). The cases hold no borderline decision, or have a zero upstream gradient where the
float64 reference counts one, so the GPU takes the reference's decisions."""
import ctypes as C

import numpy as np
import pytest

import sh_grad_ref as S
import splat_depth_ref as Z
import splat_grad_ref as R
import splat_pose_grad_ref as P
from pathtracer_gaussiansplatting_amd import PtgsError, _abi, autograd
from pathtracer_gaussiansplatting_amd.renderer import _gaussians, _ptr, _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: shared inputs may be read-only)


def _forward(renderer, c, dg=None, ubo=None):
    dg = {k: _dev(v) for k, v in c["g"].items()} if dg is None else dg
    out = torch.zeros((c["H"], c["W"], 4), dtype=torch.float32, device="cuda")
    renderer.splat_gaussians(dg, c["ubo"] if ubo is None else ubo, c["W"], c["H"], out, bg=c["bg"], want_stats=True)
    return dg, out


def _raw_pose(renderer, dg, ubo, W, H, dL, dinv, dview, n=None, bg=(0.0, 0.0, 0.0)):
    """The C call with NaN-filled gradient arrays: (rc, the arrays after a synchronise)."""
    n = int(dg["means"].shape[0]) if n is None else n
    arrs = {"means": 3, "scales": 3, "rotations": 4, "opacities": 1, "colors": 3, "means2d": 2, "conics": 3}
    t = {k: torch.full((max(n, 1) * w,), float("nan"), dtype=torch.float32, device="cuda") for k, w in arrs.items()}
    gr = _abi.GaussianGrads()
    for k, v in t.items():
        setattr(gr, k, _ptr(v))
    bgc = np.asarray(bg, np.float32)
    rc = renderer.lib.ptgs_splat_gaussians_backward_pose(renderer._h, C.byref(_gaussians(dg)), C.byref(ubo), W, H,
                                                         _abi.fptr(bgc), _ptr(dL), _ptr(dinv) or None, C.byref(gr),
                                                         dview if isinstance(dview, int) else (_ptr(dview) or None),
                                                         _stream(None))
    torch.cuda.synchronize()
    return rc, t


def _pose_call(renderer, c, dg, dL, dinv):
    """backward_pose through the C call with dL_dview pre-filled with NaN: ({key: numpy}, view [4, 4] math indexing)."""
    raw = torch.full((16,), float("nan"), dtype=torch.float32, device="cuda")
    rc, t = _raw_pose(renderer, dg, c["ubo"], c["W"], c["H"], dL, dinv, raw, bg=c["bg"])
    assert rc == 0, renderer._err()
    n = len(c["g"]["means"])
    shapes = {"means": (n, 3), "scales": (n, 3), "rotations": (n, 4), "opacities": (n,), "colors": (n, 3),
              "means2d": (n, 2), "conics": (n, 3)}
    got = {k: v.cpu().numpy().reshape(shapes[k]) for k, v in t.items()}
    return got, raw.cpu().numpy().reshape(4, 4).T


def _check_view(c, which, view, label):
    assert np.isfinite(view).all(), view
    assert np.array_equal(view[3], np.zeros(4, F)) and not np.signbit(view[3]).any()  # row 3: exactly 0
    ref = c["pose"][which]
    return P.check_blocks(ref["r64"], ref["r32"], view[:3], f"{c['name']} GPU {label}")


# ---- 1. every case, colour only and with dL_dinvdepth
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_pose_matches_reference(renderer, oracle_lib, name, depth):
    c = P.case_reference(name, oracle_lib)
    assert c["r64"]["borderline"] == 0
    which = "grads" if depth else "grads_color"
    dg, out = _forward(renderer, c)
    got, view = _pose_call(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]) if depth else None)
    assert R.rel_l2(out.cpu().numpy(), c["frame"]["image"]) < 1e-4  # (the frame differentiated is the oracle's)
    failed = _check_view(c, which, view, f"backward_pose ({which})")
    cz = Z.part(c, which)
    for k in R.GRAD_KEYS:  # the other gradients of the same call, as the plain backward's are checked
        assert np.isfinite(got[k]).all(), k
        failed += R.check_bounds(cz, k, got[k].astype(np.float64), f"GPU backward_pose ({which})")
    assert not failed, failed
    # the Renderer method: the same call, "view" in math indexing beside the usual keys
    m = renderer.splat_gaussians_backward(dg, c["ubo"], c["W"], c["H"], _dev(c["dL"]), bg=c["bg"], want_view=True,
                                          dL_dinvdepth=_dev(c["dinv"]) if depth else None)
    torch.cuda.synchronize()
    assert tuple(m["view"].shape) == (4, 4) and m["view"].dtype == torch.float32 and m["view"].is_cuda
    assert R.rel_l2(m["view"].cpu().numpy(), view) < 1e-5  # (two runs of the same kernels: the atomics' order)
    assert set(m) == {"means", "scales", "rotations", "opacities", "colors", "view"}


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_pose_depth_only(renderer, oracle_lib, name):
    c = P.case_reference(name, oracle_lib)
    dg, _ = _forward(renderer, c)
    zero = torch.zeros((c["H"], c["W"], 4), dtype=torch.float32, device="cuda")
    _, view = _pose_call(renderer, c, dg, zero, _dev(c["dinv"]))
    failed = _check_view(c, "grads_depth", view, "backward_pose (depth only)")
    assert not failed, failed


# ---- 2. the reduction's boundaries
# posed has 150 Gaussians: its n = 255, 256, 257 are the whole case. The workgroup boundary itself is met on the
# first 255 / 256 / 257 Gaussians of `chunks` (642 at the same pose, each in its own tile, all of them visible).
BOUNDARY = [("posed", n) for n in (1, 63, 64, 65, 255, 256, 257)] + [("chunks", n) for n in (255, 256, 257)]


@pytest.mark.parametrize("name,n", BOUNDARY, ids=[f"{a}-{b}" for a, b in BOUNDARY])
def test_reduction_boundaries(renderer, oracle_lib, name, n):
    """The first n Gaussians: a partial wave, a full wave, a wave and one, a partial last workgroup, a full one, a
    workgroup and one."""
    c = P.subset_reference(name, n, oracle_lib)
    assert c["r64"]["borderline"] == 0 and c["r32"]["borderline"] == 0
    if name == "chunks":
        assert len(c["g"]["means"]) == n and int((c["frame"]["radii"] > 0).sum()) == n
    dg, _ = _forward(renderer, c)
    _, view = _pose_call(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]))
    failed = _check_view(c, "grads", view, f"backward_pose, first {n}")
    assert not failed, failed


def test_frame_cases_and_no_stale_partials(renderer, oracle_lib):
    """field (20000 = 78 * 256 + 32 Gaussians: 79 partials) and layers (8000) with their masked gradients, then
    posed (150: one partial) on the same renderer straight after field: a finish that read beyond this call's
    rows would add field's."""
    failed = []
    for name in ("layers", "field"):
        c = P.frame_case_reference(name, oracle_lib)
        dg, _ = _forward(renderer, c)
        _, view = _pose_call(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]))
        failed += _check_view(c, "grads", view, "backward_pose (frame)")
    assert len(c["g"]["means"]) == 20000
    p = P.case_reference("posed", oracle_lib)
    dg, _ = _forward(renderer, p)
    _, view = _pose_call(renderer, p, dg, _dev(p["dL"]), _dev(p["dinv"]))
    failed += _check_view(p, "grads", view, "backward_pose (posed after field)")
    assert not failed, failed


# ---- 3. culled frames, count == 0, a null dL_dview
def test_culled_empty_and_null(renderer, oracle_lib):
    c = P.case_reference("posed", oracle_lib)
    W, H = c["W"], c["H"]
    eye, centre, up = R.POSE
    away = R.make_ubo(W, H, eye, tuple(2.0 * e - t for e, t in zip(eye, centre)), up)  # the scene behind the camera
    assert not np.any(oracle_lib.splat_gaussians(c["g"], away, W, H, bg=c["bg"])["radii"])
    dg, _ = _forward(renderer, c, ubo=away)
    raw = torch.full((16,), float("nan"), dtype=torch.float32, device="cuda")
    rc, t = _raw_pose(renderer, dg, away, W, H, _dev(c["dL"]), _dev(c["dinv"]), raw, bg=c["bg"])
    assert rc == 0, renderer._err()
    for k, v in t.items():  # every Gaussian is culled: every gradient is exactly 0
        assert not bool(v.any()) and bool(torch.isfinite(v).all()), k
    assert np.array_equal(raw.cpu().numpy(), np.zeros(16, F))  # sixteen exact zeros
    # count == 0: zeros and PTGS_OK, the gradient arrays untouched
    empty = {k: v[:0].contiguous() for k, v in dg.items()}
    raw.fill_(float("nan"))
    rc, t = _raw_pose(renderer, empty, c["ubo"], W, H, _dev(c["dL"]), None, raw, n=0)
    assert rc == 0 and np.array_equal(raw.cpu().numpy(), np.zeros(16, F))
    assert all(bool(torch.isnan(v).all()) for v in t.values())
    got = renderer.splat_gaussians_backward(empty, c["ubo"], W, H, _dev(c["dL"]), want_view=True)
    assert got["means"].shape == (0, 3) and not bool(got["view"].any())
    # a null or non-device dL_dview: PTGS_EINVAL, nothing enqueued
    _forward(renderer, c, dg)
    host = np.zeros(16, F)
    for bad in (None, host.ctypes.data):
        rc, t = _raw_pose(renderer, dg, c["ubo"], W, H, _dev(c["dL"]), _dev(c["dinv"]), bad if bad else 0, bg=c["bg"])
        assert rc == _abi.PTGS_EINVAL and renderer._err()
        assert all(bool(torch.isnan(v).all()) for v in t.values())
        with pytest.raises(PtgsError):
            renderer._chk(rc, "ptgs_splat_gaussians_backward_pose")
    rc, _ = _raw_pose(renderer, empty, c["ubo"], W, H, _dev(c["dL"]), None, 0, n=0)
    assert rc == _abi.PTGS_EINVAL
    # the frame is still the latest one: the rejected calls changed nothing
    ok = renderer.splat_gaussians_backward(dg, c["ubo"], W, H, _dev(c["dL"]), bg=c["bg"], want_view=True)
    torch.cuda.synchronize()
    assert not P.check_blocks(c["pose"]["grads_color"]["r64"], c["pose"]["grads_color"]["r32"],
                              ok["view"].cpu().numpy()[:3], "after the rejected calls")


# ---- 4. the SH eye
EYE_CASES = [(case, False) for case in S.CASES] + [(S.EYE_CASE, True)]
EYE_IDS = [f"d{d}-n{n}-a{a}" + ("-eye" if e else "") for (d, n, a), e in EYE_CASES]


@pytest.mark.parametrize("case,at_eye", EYE_CASES, ids=EYE_IDS)
def test_sh_eye_gradient(renderer, case, at_eye):
    deg, count, active = case
    c = S.case_reference(case, eye=at_eye)
    dm, dsh_in, dcol = _dev(c["means"]), _dev(c["sh"]), _dev(c["dcol"])
    start = _dev(np.random.default_rng(3).normal(size=(count, 3)).astype(F))
    a_means, b_means, c_means = start.clone(), start.clone(), start.clone()
    dsh0, dmeans0 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dcol, active_degree=active, dL_dmeans=a_means)
    dsh1, dmeans1, eye1 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dcol, active_degree=active,
                                                      dL_dmeans=b_means, want_eye=True)
    dsh2, dmeans2, eye2 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dcol, active_degree=active,
                                                      dL_dmeans=c_means, want_eye=True)
    dsh3, none, eye3 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dcol, active_degree=active, want_means=False,
                                                   want_eye=True)
    torch.cuda.synchronize()
    assert dmeans1 is b_means and none is None and tuple(eye1.shape) == (3,) and eye1.dtype == torch.float32
    # the same dL_dsh and the same addition into dL_dmeans as the existing call, bit for bit
    assert torch.equal(dsh1, dsh0) and torch.equal(dmeans1, dmeans0) and torch.equal(dsh3, dsh0)
    # no atomics: two runs give the same bits; the sum does not need dL_dmeans
    assert torch.equal(eye1, eye2) and torch.equal(eye3, eye1) and torch.equal(dmeans2, dmeans1)
    got = eye1.cpu().numpy().astype(np.float64)
    ref = P.eye_grad(c["means"], c["sh"], S.CAM, active, c["dcol"], torch.float64)
    if deg == 0 or active == 0:
        assert not np.any(ref) and np.array_equal(eye1.cpu().numpy(), np.zeros(3, F))  # exact zeros
        return
    r32 = P.eye_grad(c["means"], c["sh"], S.CAM, active, c["dcol"], torch.float32)
    e32 = R.rel_l2(r32, ref)
    err = R.rel_l2(got, ref)
    print(f"{case} eye={at_eye}: dL/d eye rel L2 {err:.2e}  e32 {e32:.2e}  bound {max(1e-4, 8 * e32):.1e}")
    assert np.linalg.norm(ref) > 0 and err <= max(1e-4, 8.0 * e32)
    # it is the negative of the sum of what the call adds to dL_dmeans
    added = (dmeans0 - start).double().sum(0).cpu().numpy()
    assert R.rel_l2(-added, ref) < 1e-4
    if at_eye:
        assert not bool((dmeans0 - start)[S.EYE_INDEX].any())  # a Gaussian at the eye adds nothing


def test_sh_eye_error_paths(renderer):
    c = S.case_reference((1, 63, 1))
    dm, dsh_in, dcol = _dev(c["means"]), _dev(c["sh"]), _dev(c["dcol"])
    dsh = torch.full((63, 4, 3), 7.0, dtype=torch.float32, device="cuda")
    cam = np.asarray(S.CAM, F)
    fn, h = renderer.lib.ptgs_gaussians_sh_colors_backward_eye, renderer._h
    host = np.zeros(3, F)
    for bad in (None, host.ctypes.data):
        rc = fn(h, _ptr(dm), _ptr(dsh_in), 63, 1, 1, _abi.fptr(cam), _ptr(dcol), _ptr(dsh), None, bad, _stream(None))
        torch.cuda.synchronize()
        assert rc == _abi.PTGS_EINVAL and renderer._err() and bool((dsh == 7.0).all())
    eye = torch.full((3,), float("nan"), dtype=torch.float32, device="cuda")
    assert fn(h, None, None, 0, 3, 3, None, None, None, None, _ptr(eye), _stream(None)) == 0  # count == 0: zeros
    torch.cuda.synchronize()
    assert np.array_equal(eye.cpu().numpy(), np.zeros(3, F))


# ---- 5. end to end: splat_sh_depth(view=se3_view(view0, xi)), a loss on both outputs
def test_autograd_pose_end_to_end(renderer, oracle_lib):
    c = P.case_reference("posed", oracle_lib)
    W, H = c["W"], c["H"]
    params = P.e2e_params(c)
    view0 = P.view_matrix(c["ubo"])
    xi = torch.tensor(P.E2E_XI, dtype=torch.float32, requires_grad=True)  # (a host leaf: the gradient comes back here)
    view0_t = torch.tensor(view0, dtype=torch.float32)
    view = autograd.se3_view(view0_t, xi)
    view32 = view.detach().numpy().copy()
    dL, dinv, mask = P.e2e_upstream(c, oracle_lib, params, view32)
    assert float(mask.mean()) <= R.MASK_CAP
    leaves = {k: _dev(v) for k, v in params.items()}
    before = [float(v) for v in c["ubo"].view]
    img, inv = autograd.splat_sh_depth(renderer, leaves["means"], leaves["log_scales"], leaves["rotations"],
                                       leaves["opacity_logits"], leaves["sh"], c["ubo"], W, H, bg=c["bg"], view=view)
    ((img * _dev(dL)).sum() + (inv * _dev(dinv)).sum()).backward()
    torch.cuda.synchronize()
    assert [float(v) for v in c["ubo"].view] == before  # the caller's ubo is not modified
    xi64 = np.asarray(P.E2E_XI, np.float32).astype(np.float64)
    r64 = P.e2e_reference(c, oracle_lib, params, view32, view0, xi64, dL, dinv, torch.float64)
    r32 = P.e2e_reference(c, oracle_lib, params, view32, view0, xi64, dL, dinv, torch.float32)
    keep = ~mask
    assert R.rel_l2(img.detach().cpu().numpy()[keep], r64["image"][keep]) < 1e-4
    assert R.rel_l2(inv.detach().cpu().numpy()[keep], r64["invdepth"][keep]) < 1e-4
    assert xi.grad is not None and not xi.grad.is_cuda and tuple(xi.grad.shape) == (6,)
    e32 = R.rel_l2(r32["xi"], r64["xi"])
    err = R.rel_l2(xi.grad.numpy(), r64["xi"])
    share = np.linalg.norm(r64["total"] - r64["view"]) / np.linalg.norm(r64["total"])
    print(f"end to end: dL/dxi rel L2 {err:.2e}  e32 {e32:.2e}  bound {max(1e-4, 8 * e32):.1e}; "
          f"the eye's share of dL/d view {share:.2e}")
    assert np.all(r64["eye"] != 0.0) and err <= max(1e-4, 8.0 * e32)
    # a device leaf receives its gradient on the device; a tensor camera_pos receives the eye's own gradient
    vdev = torch.tensor(view32, device="cuda", requires_grad=True)
    cam = torch.tensor(-(view32[:3, :3].T @ view32[:3, 3]), requires_grad=True)
    img, inv = autograd.splat_sh_depth(renderer, leaves["means"], leaves["log_scales"], leaves["rotations"],
                                       leaves["opacity_logits"], leaves["sh"], c["ubo"], W, H, bg=c["bg"], view=vdev,
                                       camera_pos=cam)
    ((img * _dev(dL)).sum() + (inv * _dev(dinv)).sum()).backward()
    torch.cuda.synchronize()
    assert vdev.grad.is_cuda and tuple(vdev.grad.shape) == (4, 4) and not bool(vdev.grad[3].any())
    assert not cam.grad.is_cuda
    e32v = R.rel_l2(r32["view"], r64["view"])
    assert R.rel_l2(vdev.grad.cpu().numpy()[:3], r64["view"]) <= max(1e-4, 8.0 * e32v)
    assert R.rel_l2(cam.grad.numpy(), r64["eye"]) <= max(1e-4, 8.0 * R.rel_l2(r32["eye"], r64["eye"]))


# ---- 6. without view= nothing changes: the calls and their keywords are today's
class _Recording:
    """The renderer with every method call recorded as (name, sorted keyword names)."""

    def __init__(self, renderer):
        object.__setattr__(self, "_r", renderer)
        object.__setattr__(self, "calls", [])

    def __getattr__(self, name):
        v = getattr(self._r, name)
        if not callable(v) or name.startswith("_"):
            return v

        def call(*a, **kw):
            self.calls.append((name, tuple(sorted(kw))))
            return v(*a, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self._r, name, value)


PLAIN = {
    "splat": [("splat_gaussians", ("bg", "want_stats")), ("splat_gaussians_backward", ("bg",))],
    "splat_depth": [("splat_gaussians", ("bg", "want_stats")), ("splat_gaussians_invdepth", ()),
                    ("splat_gaussians_backward", ("bg", "dL_dinvdepth"))],
    "splat_sh": [("activate_gaussians", ()), ("sh_colors", ("active_degree",)),
                 ("splat_gaussians", ("bg", "want_stats")), ("splat_gaussians_backward", ("bg", "want_means2d")),
                 ("sh_colors_backward", ("active_degree", "dL_dmeans", "want_means")),
                 ("activate_gaussians_backward", ("out",))],
    "splat_sh_depth": [("activate_gaussians", ()), ("sh_colors", ("active_degree",)),
                       ("splat_gaussians", ("bg", "want_stats")), ("splat_gaussians_invdepth", ()),
                       ("splat_gaussians_backward", ("bg", "dL_dinvdepth", "want_means2d")),
                       ("sh_colors_backward", ("active_degree", "dL_dmeans", "want_means")),
                       ("activate_gaussians_backward", ("out",))],
}


@pytest.mark.parametrize("fn", sorted(PLAIN))
def test_calls_without_view_are_unchanged(renderer, oracle_lib, fn):
    c = P.case_reference("posed", oracle_lib)
    W, H = c["W"], c["H"]
    params = P.e2e_params(c)
    sh_form = "sh" in fn
    src = params if sh_form else c["g"]
    keys = ("means", "log_scales", "rotations", "opacity_logits", "sh") if sh_form else \
        ("means", "scales", "rotations", "opacities", "colors")
    dL, dinv = _dev(c["dL"]), _dev(c["dinv"])

    def run(**kw):
        rec = _Recording(renderer)
        leaves = [_dev(src[k]).requires_grad_(True) for k in keys]
        out = getattr(autograd, fn)(rec, *leaves, c["ubo"], W, H, bg=c["bg"], **kw)
        loss = (out * dL).sum() if not isinstance(out, tuple) else (out[0] * dL).sum() + (out[1] * dinv).sum()
        loss.backward()
        torch.cuda.synchronize()
        return rec.calls, leaves

    calls, leaves = run()
    assert calls == PLAIN[fn], calls
    # with view= the backward asks for the view (and, for the SH forms, the eye): the wrapper does see the difference
    view = torch.tensor(P.view_matrix(c["ubo"]), dtype=torch.float32, requires_grad=True)
    kw = {"view": view}
    if sh_form:  # (the eye of the plain run, as a leaf: by default it would be the view's own)
        kw["camera_pos"] = torch.tensor([float(v) for v in c["ubo"].camera_pos][:3], requires_grad=True)
    posed_calls, posed_leaves = run(**kw)
    if sh_form:
        assert kw["camera_pos"].grad is not None and float(kw["camera_pos"].grad.abs().max()) > 0
    want = [(n, tuple(sorted(k + (("want_view",) if n == "splat_gaussians_backward" else ()) +
                             (("want_eye",) if n == "sh_colors_backward" else ())))) for n, k in PLAIN[fn]]
    assert posed_calls == want, posed_calls
    assert view.grad is not None and tuple(view.grad.shape) == (4, 4) and float(view.grad.abs().max()) > 0
    for a, b in zip(leaves, posed_leaves):  # the same view: the same gradients for the Gaussians
        assert R.rel_l2(b.grad.cpu().numpy(), a.grad.cpu().numpy()) < 1e-5


# ---- 7. pose recovery
def test_pose_recovery(renderer, oracle_lib):
    """The reference descent's constants with the GPU's gradient: plain steps on xi from XI0 end at <= 0.5 of the
    initial pose error (the float64 reference run ends at <= 0.25: tests/test_splat_pose_grad_ref.py)."""
    c = P.case_reference("posed", oracle_lib)
    W, H = c["W"], c["H"]
    dg = {k: _dev(v) for k, v in c["g"].items()}
    target_img, target_inv = _dev(c["r64"]["image"].astype(F)), _dev(c["r64"]["invdepth"].astype(F))
    view0 = torch.tensor(P.view_matrix(c["ubo"]), dtype=torch.float32)
    xi = torch.tensor(P.XI0, dtype=torch.float32, requires_grad=True)
    lr = torch.tensor([P.LR[0]] * 3 + [P.LR[1]] * 3, dtype=torch.float32)
    errs = [P.pose_error(c, xi.detach().numpy().astype(np.float64))]
    for _ in range(P.STEPS):
        img, inv = autograd.splat_depth(renderer, dg["means"], dg["scales"], dg["rotations"], dg["opacities"],
                                        dg["colors"], c["ubo"], W, H, bg=c["bg"], view=autograd.se3_view(view0, xi))
        loss = 0.5 * ((img - target_img) ** 2).sum() + 0.5 * P.DEPTH_WEIGHT * ((inv - target_inv) ** 2).sum()
        loss.backward()
        with torch.no_grad():
            xi -= lr * xi.grad
        xi.grad = None
        errs.append(P.pose_error(c, xi.detach().numpy().astype(np.float64)))
    print("pose error per step: " + " ".join(f"{e:.4f}" for e in errs) + f"  ({errs[-1] / errs[0]:.3f})")
    assert errs[0] > 0.1 and errs[-1] <= 0.5 * errs[0]
