"""3DGS depth supervision on the GPU: ptgs_splat_gaussians_invdepth, ptgs_splat_gaussians_backward_depth and
ptgs_image_loss_invdepth_l1 against the float64 reference of tests/splat_depth_ref.py, their error paths, and
torch.autograd through autograd.splat_depth / splat_sh_depth / invdepth_l1.

Tolerances are the project's existing ones: 1e-4 relative L2 for a blended map (the allowance for the blend's
hardware exp2), max(1e-4, 8 e32) per gradient array and subset (splat_grad_ref.check_bounds, with e32 from the new
reference), 1e-5 between two runs of the same atomics. The cases hold no borderline decision
(tests/test_splat_depth_ref.py), so the GPU takes the reference's decisions."""
import ctypes as C

import numpy as np
import pytest

import splat_depth_ref as Z
import splat_grad_ref as R
from pathtracer_gaussiansplatting_amd import PtgsError, Renderer, _abi, autograd
from pathtracer_gaussiansplatting_amd.renderer import _gaussians, _ptr, _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SAME_KERNELS = 1e-5  # relative L2 between two runs of the same kernels: only the atomics' order differs
DEPTH_KEYS = ("opacities", "means2d", "conics", "means", "scales", "rotations")  # what D passes gradient to


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(renderer, c, dg=None, bg=None, **kw):
    dg = {k: _dev(v) for k, v in c["g"].items()} if dg is None else dg
    out = torch.zeros((c["H"], c["W"], 4), dtype=torch.float32, device="cuda")
    kw.setdefault("want_stats", True)
    renderer.splat_gaussians(dg, c["ubo"], c["W"], c["H"], out, bg=c["bg"] if bg is None else bg, **kw)
    return dg, out


def _backward(renderer, c, dg, dL, dinv=None):
    got = renderer.splat_gaussians_backward(dg, c["ubo"], c["W"], c["H"], dL, bg=c["bg"], want_means2d=True,
                                            want_conics=True, dL_dinvdepth=dinv)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _exact_zeros(c, got, keys):
    culled = c["frame"]["radii"] == 0
    if c["name"] == "edges":
        assert culled.any()
    if c["name"] == "posed":
        assert np.count_nonzero(c["g"]["opacities"] == 0.0) == 1
    for k in keys:  # culled Gaussians and a listed Gaussian of opacity 0.0: exactly zero
        assert not np.any(got[k][culled]), k
        for i in np.flatnonzero(c["g"]["opacities"] == 0.0):
            assert not np.any(got[k][i]), (k, i)


# ---- 1. the inverse-depth render against the reference
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_invdepth_matches_reference(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    assert c["r64"]["borderline"] == 0
    _forward(renderer, c)
    a = torch.full((c["H"], c["W"]), 7.0, dtype=torch.float32, device="cuda")
    assert renderer.splat_gaussians_invdepth(c["W"], c["H"], a) is a
    b = renderer.splat_gaussians_invdepth(c["W"], c["H"])
    torch.cuda.synchronize()
    got = a.cpu().numpy()
    err = R.rel_l2(got, c["r64"]["invdepth"])
    print(f"{name}: invdepth rel L2 {err:.2e}")
    assert np.isfinite(got).all() and np.linalg.norm(c["r64"]["invdepth"]) > 0 and err < 1e-4
    assert not np.any(got[c["r64"]["empty"]])  # a pixel of an empty tile: exactly 0 (the sentinel overwritten)
    if name == "edges":
        assert c["r64"]["empty"].any()
    assert torch.equal(a, b)  # no atomics: two runs are bit-equal


# ---- 2. independent of the reference: D is the forward's blend of the colour 1 / d over a zero background
@pytest.mark.parametrize("name", ["posed", "batches", "opaque"])
def test_invdepth_is_the_forward_blend_of_inverse_depth(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    view = np.asarray(c["ubo"].view, np.float32).reshape(4, 4).T  # row-major
    m = c["g"]["means"]
    d = -(((view[2, 0] * m[:, 0] + view[2, 1] * m[:, 1]) + view[2, 2] * m[:, 2]) + view[2, 3])  # f32, the kernel's order
    assert d.dtype == np.float32
    vis = c["frame"]["radii"] > 0
    cols = np.zeros((len(d), 3), np.float32)
    cols[vis] = (np.float32(1.0) / d[vis])[:, None]
    dg = {k: _dev(v) for k, v in dict(c["g"], colors=cols).items()}
    _, img = _forward(renderer, c, dg, bg=(0.0, 0.0, 0.0))
    inv = renderer.splat_gaussians_invdepth(c["W"], c["H"])
    torch.cuda.synchronize()
    rgb = img.cpu().numpy()[..., :3]
    for ch in range(3):
        err = R.rel_l2(inv.cpu().numpy(), rgb[..., ch])
        print(f"{name}: invdepth vs forward channel {ch}: {err:.2e}")
        assert np.linalg.norm(rgb[..., ch]) > 0 and err < 1e-4


# ---- 3. the frame stays valid; 4. a zero depth gradient
@pytest.mark.parametrize("name", ["clamp", "chunks"])
def test_invdepth_leaves_the_frame_and_zero_depth_gradient(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    dg, _ = _forward(renderer, c)
    dL = _dev(c["dL"])
    before = _backward(renderer, c, dg, dL)
    renderer.splat_gaussians_invdepth(c["W"], c["H"])
    after = _backward(renderer, c, dg, dL)  # (no forward in between: the same frame)
    zero = _backward(renderer, c, dg, dL, torch.zeros((c["H"], c["W"]), dtype=torch.float32, device="cuda"))
    for k in R.GRAD_KEYS:
        e1, e2 = R.rel_l2(after[k], before[k]), R.rel_l2(zero[k], before[k])
        print(f"{name} {k}: after invdepth {e1:.2e}, backward_depth with a zero gradient {e2:.2e}")
        assert np.linalg.norm(before[k]) > 0 and e1 < SAME_KERNELS and e2 < SAME_KERNELS, (k, e1, e2)


# ---- 5. full gradients
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_depth_matches_reference(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    assert c["r64"]["borderline"] == 0
    dg, out = _forward(renderer, c)
    got = _backward(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]))
    assert R.rel_l2(out.cpu().numpy(), c["frame"]["image"]) < 1e-4  # (the frame differentiated is the oracle's)
    failed = []
    for k in R.GRAD_KEYS:
        assert np.isfinite(got[k]).all(), k
        failed += R.check_bounds(c, k, got[k].astype(np.float64), "GPU backward_depth")
    assert not failed, failed
    _exact_zeros(c, got, R.GRAD_KEYS)


# ---- 6. depth only
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_depth_only(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    dg, _ = _forward(renderer, c)
    got = _backward(renderer, c, dg, torch.zeros((c["H"], c["W"], 4), dtype=torch.float32, device="cuda"),
                    _dev(c["dinv"]))
    cd = Z.part(c, "grads_depth")
    failed = []
    for k in DEPTH_KEYS:
        assert np.isfinite(got[k]).all() and np.linalg.norm(cd["r64"]["grads"][k]) > 0, k
        failed += R.check_bounds(cd, k, got[k].astype(np.float64), "GPU depth only")
    assert not failed, failed
    assert not np.any(got["colors"])  # exactly zero: the colours do not enter D
    _exact_zeros(c, got, R.GRAD_KEYS)


# ---- 7. error paths
def _raw_backward_depth(renderer, dg, ubo, W, H, dL, dinv, n=None):
    """The C call with sentinel-filled gradient arrays: (rc, the arrays after a synchronise)."""
    n = int(dg["means"].shape[0]) if n is None else n
    arrs = {"means": 3, "scales": 3, "rotations": 4, "opacities": 1, "colors": 3}
    t = {k: torch.full((max(n, 1) * w,), 7.0, dtype=torch.float32, device="cuda") for k, w in arrs.items()}
    gr = _abi.GaussianGrads()
    for k, v in t.items():
        setattr(gr, k, _ptr(v))
    bg = np.zeros(3, np.float32)
    rc = renderer.lib.ptgs_splat_gaussians_backward_depth(renderer._h, C.byref(_gaussians(dg)), C.byref(ubo), W, H,
                                                          _abi.fptr(bg), _ptr(dL), _ptr(dinv) or None, C.byref(gr),
                                                          _stream(None))
    torch.cuda.synchronize()
    return rc, t


def _rejected(renderer, dg, ubo, W, H, dL, dinv, invdepth_too=True):
    rc, t = _raw_backward_depth(renderer, dg, ubo, W, H, dL, dinv)
    assert rc == _abi.PTGS_EINVAL and renderer._err()
    for k, v in t.items():  # nothing was enqueued: the arrays still hold the sentinel
        assert bool((v == 7.0).all()), k
    if dinv is not None:
        with pytest.raises(PtgsError):
            renderer.splat_gaussians_backward(dg, ubo, W, H, dL, dL_dinvdepth=dinv)
    if invdepth_too:
        out = torch.full((H, W), 7.0, dtype=torch.float32, device="cuda")
        rc = renderer.lib.ptgs_splat_gaussians_invdepth(renderer._h, W, H, _ptr(out), _stream(None))
        torch.cuda.synchronize()
        assert rc == _abi.PTGS_EINVAL and renderer._err() and bool((out == 7.0).all())
        with pytest.raises(PtgsError):
            renderer.splat_gaussians_invdepth(W, H, out)


def test_depth_error_paths(renderer, oracle_lib):
    c = Z.case_reference("edges", oracle_lib)
    W, H, ubo = c["W"], c["H"], c["ubo"]
    dg = {k: _dev(v) for k, v in c["g"].items()}
    dL, dinv = _dev(c["dL"]), _dev(c["dinv"])
    fresh = Renderer(0, publish_splat_buffers=True)
    try:
        _rejected(fresh, dg, ubo, W, H, dL, dinv)  # no prior frame
    finally:
        fresh.close()
    plain = Renderer(0)
    try:
        _forward(plain, c, dg)
        _rejected(plain, dg, ubo, W, H, dL, dinv)  # a frame that was not published
    finally:
        plain.close()
    _forward(renderer, c, dg, want_stats=False)
    _rejected(renderer, dg, ubo, W, H, dL, dinv)  # published context, but a stream-ordered frame (no stats)
    _forward(renderer, c, dg, tile_rows=(0, 1))
    _rejected(renderer, dg, ubo, W, H, dL, dinv)  # tile rows restricted
    _forward(renderer, c, dg)
    wide = torch.zeros((H, W + 1, 4), device="cuda")
    _rejected(renderer, dg, ubo, W + 1, H, wide, wide[..., 0].contiguous())  # another image size
    ids = dict(dg, ids=torch.arange(len(c["g"]["means"]), dtype=torch.int32, device="cuda"))
    _rejected(renderer, ids, ubo, W, H, dL, dinv, invdepth_too=False)  # reordered copies are not differentiated
    fewer = {k: v[:10].contiguous() for k, v in dg.items()}
    _rejected(renderer, fewer, ubo, W, H, dL, dinv, invdepth_too=False)  # another count
    _rejected(renderer, dg, ubo, W, H, dL, None, invdepth_too=False)  # a null dL_dinvdepth
    assert renderer.lib.ptgs_splat_gaussians_invdepth(renderer._h, W, H, None, _stream(None)) == _abi.PTGS_EINVAL
    # the frame is still the latest one: the rejected calls changed nothing
    inv = renderer.splat_gaussians_invdepth(W, H)
    ok = renderer.splat_gaussians_backward(dg, ubo, W, H, dL, bg=c["bg"], dL_dinvdepth=dinv)
    torch.cuda.synchronize()
    assert R.rel_l2(inv.cpu().numpy(), c["r64"]["invdepth"]) < 1e-4
    assert R.rel_l2(ok["means"].cpu().numpy(), c["r64"]["grads"]["means"]) < 1e-4
    # count == 0: PTGS_OK, nothing launched
    empty = {k: v[:0].contiguous() for k, v in dg.items()}
    rc, t = _raw_backward_depth(renderer, empty, ubo, W, H, dL, dinv, n=0)
    assert rc == 0 and all(bool((v == 7.0).all()) for v in t.values())
    assert renderer.splat_gaussians_backward(empty, ubo, W, H, dL, dL_dinvdepth=dinv)["means"].shape == (0, 3)


# ---- 8. the loss
def _ulp_close(got, want64):
    want = np.float32(want64)
    return abs(float(got) - float(want)) <= float(np.spacing(np.abs(want)))


def _loss_maps():
    rng = np.random.default_rng(78)
    H, W = 41, 53  # 2173 pixels: three workgroups, the last one partial
    t = rng.uniform(0.5, 12.0, (H, W)).astype(np.float32)
    D = (1.0 / t + rng.normal(scale=0.05, size=(H, W))).astype(np.float32)
    t[0, 0], t[3, 5], t[7, 11], t[40, 52] = 0.0, -2.5, np.nan, np.inf
    t[10, 10], D[10, 10] = 2.0, 0.5  # an exact tie
    t[25, :] = np.inf  # misses: the target inverse depth is 0
    t[30, 7:19] = np.nan
    return D, t


def test_invdepth_l1_loss(renderer):
    D, t = _loss_maps()
    weight, scale = 0.7, 3.0
    want, want_grad = Z.invdepth_l1(D, t, weight, scale)
    dD, dt = _dev(D), _dev(t)
    grad = torch.full(D.shape, 7.0, dtype=torch.float32, device="cuda")
    terms, g = renderer.invdepth_l1_loss(dD, dt, weight=weight, grad_out=grad, grad_scale=scale)
    only, none = renderer.invdepth_l1_loss(dD, dt, weight=weight, grad_scale=scale)
    again, _ = renderer.invdepth_l1_loss(dD, dt, weight=weight, grad_out=torch.empty_like(grad), grad_scale=scale)
    torch.cuda.synchronize()
    tm = terms.cpu().numpy()
    print(f"invdepth_l1: terms {tm}, restated {want}")
    assert g is grad and none is None
    assert np.isfinite(tm).all() and _ulp_close(tm[0], want[0]) and _ulp_close(tm[1], want[1])
    assert tm[2] == want[2] == D.size - 3 - 12 and tm[3] == 0.0
    got = grad.cpu().numpy()
    assert np.array_equal(got, want_grad)  # bit-equal (both finite: no NaN anywhere)
    for y, x in ((0, 0), (3, 5), (7, 11), (10, 10), (30, 8)):  # 0, negative and NaN targets, and the tie
        assert got[y, x] == 0.0
    assert got[40, 52] != 0.0 and np.count_nonzero(got[25]) == D.shape[1]  # misses are supervised
    assert torch.equal(only, terms) and torch.equal(again, terms)  # dL = NULL: the same bits; two runs: the same
    # the weight scales the first term only; a weight of 0 leaves a zero gradient
    zero_t, zero_g = renderer.invdepth_l1_loss(dD, dt, weight=0.0, grad_out=torch.empty_like(grad))
    torch.cuda.synchronize()
    assert float(zero_t[0]) == 0.0 and float(zero_t[1]) == float(terms[1]) and not bool(zero_g.any())


def test_invdepth_l1_loss_error_paths(renderer):
    D, t = _loss_maps()
    dD, dt = _dev(D), _dev(t)
    H, W = D.shape
    fn, h = renderer.lib.ptgs_image_loss_invdepth_l1, renderer._h
    terms = torch.full((4,), 7.0, dtype=torch.float32, device="cuda")
    grad = torch.full(D.shape, 7.0, dtype=torch.float32, device="cuda")
    host = np.zeros(D.size, np.float32)
    bad = [
        (None, _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), None, W, H, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, 1.0, 1.0, None, _ptr(grad)),
        (_ptr(dD), _ptr(dt), 0, H, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, 0, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), 16385, 1, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, float("nan"), 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, 1.0, float("inf"), _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), _ptr(dD)),  # the gradient over the input
        (host.ctypes.data, _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), _ptr(grad)),  # host pointers
        (_ptr(dD), host.ctypes.data, W, H, 1.0, 1.0, _ptr(terms), _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, 1.0, 1.0, host.ctypes.data, _ptr(grad)),
        (_ptr(dD), _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), host.ctypes.data),
    ]
    for args in bad:
        assert fn(h, *args, _stream(None)) == _abi.PTGS_EINVAL and renderer._err(), args
    torch.cuda.synchronize()
    assert bool((terms == 7.0).all()) and bool((grad == 7.0).all())  # nothing was enqueued
    assert fn(None, _ptr(dD), _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), None, _stream(None)) == _abi.PTGS_EINVAL
    with pytest.raises(PtgsError):
        renderer.invdepth_l1_loss(dD, dt[:-1])
    assert fn(h, _ptr(dD), _ptr(dt), W, H, 1.0, 1.0, _ptr(terms), _ptr(grad), _stream(None)) == 0  # and a good call
    torch.cuda.synchronize()
    assert not bool((grad == 7.0).any())


# ---- 9. autograd
def _direct_total(renderer, c, dg, target, tdepth, weight):
    """The C calls by hand: forward, invdepth, the two losses with their gradients, backward_depth."""
    W, H = c["W"], c["H"]
    _, img = _forward(renderer, c, dg)
    inv = renderer.splat_gaussians_invdepth(W, H)
    _, g_img = renderer.l1_dssim_loss(img, target, grad_out=torch.empty_like(img))
    _, g_inv = renderer.invdepth_l1_loss(inv, tdepth, weight=weight, grad_out=torch.empty_like(inv))
    return renderer.splat_gaussians_backward(dg, c["ubo"], W, H, g_img, bg=c["bg"], dL_dinvdepth=g_inv)


def _targets(c):
    rng = np.random.default_rng(91)
    target = _dev(rng.uniform(0.0, 1.0, (c["H"], c["W"], 3)).astype(np.float32))
    td = rng.uniform(3.0, 9.0, (c["H"], c["W"])).astype(np.float32)
    td[::5, ::3] = np.inf
    td[1, 1] = 0.0
    return target, _dev(td)


@pytest.mark.parametrize("name", ["opaque", "posed"])
def test_autograd_splat_depth_matches_the_direct_calls(renderer, oracle_lib, name):
    c = Z.case_reference(name, oracle_lib)
    W, H = c["W"], c["H"]
    dg = {k: _dev(v) for k, v in c["g"].items()}
    target, tdepth = _targets(c)
    direct = _direct_total(renderer, c, dg, target, tdepth, 0.5)
    leaves = {k: v.clone().requires_grad_(k != "rotations") for k, v in dg.items()}
    img, inv = autograd.splat_depth(renderer, leaves["means"], leaves["scales"], leaves["rotations"],
                                    leaves["opacities"], leaves["colors"], c["ubo"], W, H, bg=c["bg"])
    assert img.shape == (H, W, 4) and inv.shape == (H, W)
    assert R.rel_l2(inv.detach().cpu().numpy(), c["r64"]["invdepth"]) < 1e-4
    loss = autograd.l1_dssim(renderer, img, target) + autograd.invdepth_l1(renderer, inv, tdepth, weight=0.5)
    loss.backward()
    torch.cuda.synchronize()
    assert leaves["rotations"].grad is None
    for k in ("means", "scales", "opacities", "colors"):
        err = R.rel_l2(leaves[k].grad.cpu().numpy(), direct[k].cpu().numpy())
        print(f"{name} autograd splat_depth vs direct {k}: {err:.2e}")
        assert float(direct[k].abs().max()) > 0 and err < SAME_KERNELS, (k, err)
    # img alone: the plain backward, as autograd.splat gives it
    dL = _dev(c["dL"])
    a = {k: v.clone().requires_grad_(True) for k, v in dg.items()}
    b = {k: v.clone().requires_grad_(True) for k, v in dg.items()}
    img_a, _ = autograd.splat_depth(renderer, a["means"], a["scales"], a["rotations"], a["opacities"], a["colors"],
                                    c["ubo"], W, H, bg=c["bg"])
    (img_a * dL).sum().backward()
    img_b = autograd.splat(renderer, b["means"], b["scales"], b["rotations"], b["opacities"], b["colors"], c["ubo"],
                           W, H, bg=c["bg"])
    (img_b * dL).sum().backward()
    torch.cuda.synchronize()
    assert R.rel_l2(img_a.detach().cpu().numpy(), img_b.detach().cpu().numpy()) < SAME_KERNELS
    for k in a:
        err = R.rel_l2(a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy())
        print(f"{name} splat_depth (img only) vs splat {k}: {err:.2e}")
        assert err < SAME_KERNELS, (k, err)
    # invdepth alone: the image's gradient counts as zeros
    d = {k: v.clone().requires_grad_(True) for k, v in dg.items()}
    _, inv_d = autograd.splat_depth(renderer, d["means"], d["scales"], d["rotations"], d["opacities"], d["colors"],
                                    c["ubo"], W, H, bg=c["bg"])
    (inv_d * _dev(c["dinv"])).sum().backward()
    torch.cuda.synchronize()
    assert not bool(d["colors"].grad.any())
    assert R.rel_l2(d["means"].grad.cpu().numpy(), c["r64"]["grads_depth"]["means"]) < 1e-4


def test_autograd_splat_sh_depth_matches_the_direct_calls(renderer, oracle_lib):
    """splat_sh_depth: the checkpoint parameterisation (log-scales, logits, degree-1 SH) around the same calls."""
    c = Z.case_reference("posed", oracle_lib)
    W, H, ubo = c["W"], c["H"], c["ubo"]
    g = c["g"]
    n = len(g["means"])
    rng = np.random.default_rng(92)
    op = np.clip(g["opacities"], 0.02, 0.98)
    params = {"means": _dev(g["means"]), "log_scales": _dev(np.log(g["scales"])), "rotations": _dev(g["rotations"]),
              "opacity_logits": _dev(np.log(op / (1.0 - op)).astype(np.float32)),
              "sh": _dev(rng.normal(scale=0.4, size=(n, 4, 3)).astype(np.float32))}
    target, tdepth = _targets(c)
    cam = tuple(float(v) for v in ubo.camera_pos)[:3]
    # the direct chain
    sc, opac = renderer.activate_gaussians(params["log_scales"], params["opacity_logits"])
    cols = renderer.sh_colors(params["means"], params["sh"], cam)
    dg = {"means": params["means"], "scales": sc, "rotations": params["rotations"], "opacities": opac, "colors": cols}
    gr = _direct_total(renderer, c, dg, target, tdepth, 0.5)
    d_sh, d_means = renderer.sh_colors_backward(params["means"], params["sh"], cam, gr["colors"], dL_dmeans=gr["means"])
    d_ls, d_lo = renderer.activate_gaussians_backward(sc, opac, gr["scales"], gr["opacities"])
    direct = {"means": d_means, "log_scales": d_ls, "rotations": gr["rotations"], "opacity_logits": d_lo, "sh": d_sh}
    leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img, inv = autograd.splat_sh_depth(renderer, leaves["means"], leaves["log_scales"], leaves["rotations"],
                                       leaves["opacity_logits"], leaves["sh"], ubo, W, H, bg=c["bg"])
    loss = autograd.l1_dssim(renderer, img, target) + autograd.invdepth_l1(renderer, inv, tdepth, weight=0.5)
    loss.backward()
    torch.cuda.synchronize()
    for k, v in direct.items():
        err = R.rel_l2(leaves[k].grad.cpu().numpy(), v.cpu().numpy())
        print(f"autograd splat_sh_depth vs direct {k}: {err:.2e}")
        assert float(v.abs().max()) > 0 and err < SAME_KERNELS, (k, err)
    # img alone equals splat_sh
    dL = _dev(c["dL"])
    a = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    b = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    img_a, _ = autograd.splat_sh_depth(renderer, a["means"], a["log_scales"], a["rotations"], a["opacity_logits"],
                                       a["sh"], ubo, W, H, bg=c["bg"])
    (img_a * dL).sum().backward()
    img_b = autograd.splat_sh(renderer, b["means"], b["log_scales"], b["rotations"], b["opacity_logits"], b["sh"], ubo,
                              W, H, bg=c["bg"])
    (img_b * dL).sum().backward()
    torch.cuda.synchronize()
    assert R.rel_l2(img_a.detach().cpu().numpy(), img_b.detach().cpu().numpy()) < SAME_KERNELS
    for k in a:
        err = R.rel_l2(a[k].grad.cpu().numpy(), b[k].grad.cpu().numpy())
        print(f"splat_sh_depth (img only) vs splat_sh {k}: {err:.2e}")
        assert err < SAME_KERNELS, (k, err)
