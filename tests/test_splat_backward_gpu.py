"""ptgs_splat_gaussians_backward on the GPU against the float64 reference (tests/splat_grad_ref.py), its error
paths, and torch.autograd through pathtracer_gaussiansplatting_amd.autograd.splat.

Tolerance: per array, relative L2 against the float64 reference of at most max(1e-4, 8 e32), e32 being the
error of the reference's own float32 run (1e-4: the project's allowance for the blend's hardware exp2; 8x: the
different operation order and the atomics' summation order). The same bound holds on subsets of the Gaussians
(splat_grad_ref.subsets: each quarter by gradient norm, the Gaussians beyond the EWA clamp) with e32 taken on
the same rows, so that the large gradients cannot hide an error in the small ones. The cases hold no
borderline decision (tests/test_splat_grad_ref.py), so the GPU takes the reference's decisions."""
import ctypes as C

import numpy as np
import pytest

import splat_grad_ref as R
from pathtracer_gaussiansplatting_amd import PtgsError, Renderer, _abi, autograd
from pathtracer_gaussiansplatting_amd.renderer import _gaussians, _ptr, _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _forward(renderer, c, dg=None, **kw):
    dg = {k: _dev(v) for k, v in c["g"].items()} if dg is None else dg
    out = torch.zeros((c["H"], c["W"], 4), dtype=torch.float32, device="cuda")
    kw.setdefault("want_stats", True)
    renderer.splat_gaussians(dg, c["ubo"], c["W"], c["H"], out, bg=c["bg"], **kw)
    return dg, out


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_backward_matches_reference(renderer, oracle_lib, name):
    c = R.case_reference(name, oracle_lib)
    assert c["r64"]["borderline"] == 0
    dg, out = _forward(renderer, c)
    got = renderer.splat_gaussians_backward(dg, c["ubo"], c["W"], c["H"], _dev(c["dL"]), bg=c["bg"],
                                            want_means2d=True, want_conics=True)
    torch.cuda.synchronize()
    assert R.rel_l2(out.cpu().numpy(), c["frame"]["image"]) < 1e-4  # (the frame differentiated is the oracle's)
    failed = []
    for k in R.GRAD_KEYS:
        a = got[k].cpu().numpy().astype(np.float64)
        assert np.isfinite(a).all(), k
        # the whole array and every subset of splat_grad_ref.subsets (the quarters by gradient norm, the
        # Gaussians beyond the EWA clamp): max(1e-4, 8 e32) with e32 on the same rows
        failed += R.check_bounds(c, k, a, "GPU")
    assert not failed, failed
    culled = c["frame"]["radii"] == 0
    if name == "edges":
        assert culled.any()
    for k in R.GRAD_KEYS:  # culled Gaussians (near plane, behind the camera, empty rect): exactly zero
        assert not np.any(got[k].cpu().numpy()[culled]), k
    if name == "posed":
        assert np.count_nonzero(c["g"]["opacities"] == 0.0) == 1
    for i in np.flatnonzero(c["g"]["opacities"] == 0.0):  # a listed Gaussian of opacity 0.0: exactly zero
        for k in R.GRAD_KEYS:
            assert not np.any(got[k].cpu().numpy()[i]), (k, i)


def _raw_backward(renderer, dg, ubo, W, H, dL, n=None):
    """The C call with sentinel-filled gradient arrays: (rc, the arrays after a synchronise)."""
    n = int(dg["means"].shape[0]) if n is None else n
    arrs = {"means": 3, "scales": 3, "rotations": 4, "opacities": 1, "colors": 3}
    t = {k: torch.full((max(n, 1) * w,), 7.0, dtype=torch.float32, device="cuda") for k, w in arrs.items()}
    gr = _abi.GaussianGrads()
    for k, v in t.items():
        setattr(gr, k, _ptr(v))
    bg = np.zeros(3, np.float32)
    rc = renderer.lib.ptgs_splat_gaussians_backward(renderer._h, C.byref(_gaussians(dg)), C.byref(ubo), W, H,
                                                    _abi.fptr(bg), _ptr(dL), C.byref(gr), _stream(None))
    torch.cuda.synchronize()
    return rc, t


def _rejected(renderer, dg, ubo, W, H, dL):
    rc, t = _raw_backward(renderer, dg, ubo, W, H, dL)
    assert rc == _abi.PTGS_EINVAL and renderer._err()
    for k, v in t.items():  # nothing was enqueued: the arrays still hold the sentinel
        assert bool((v == 7.0).all()), k
    with pytest.raises(PtgsError):
        renderer.splat_gaussians_backward(dg, ubo, W, H, dL)


def test_backward_error_paths(renderer, oracle_lib):
    c = R.case_reference("edges", oracle_lib)
    W, H, ubo = c["W"], c["H"], c["ubo"]
    dg = {k: _dev(v) for k, v in c["g"].items()}
    dL = _dev(c["dL"])
    fresh = Renderer(0, publish_splat_buffers=True)
    try:
        _rejected(fresh, dg, ubo, W, H, dL)  # no prior frame
    finally:
        fresh.close()
    plain = Renderer(0)
    try:
        _forward(plain, c, dg)
        _rejected(plain, dg, ubo, W, H, dL)  # a frame that was not published
    finally:
        plain.close()
    _forward(renderer, c, dg, want_stats=False)
    _rejected(renderer, dg, ubo, W, H, dL)  # published context, but a stream-ordered frame (no stats)
    _forward(renderer, c, dg, tile_rows=(0, 1))
    _rejected(renderer, dg, ubo, W, H, dL)  # tile rows restricted
    _forward(renderer, c, dg)
    ids = dict(dg, ids=torch.arange(len(c["g"]["means"]), dtype=torch.int32, device="cuda"))
    _rejected(renderer, ids, ubo, W, H, dL)  # reordered copies are not differentiated
    _rejected(renderer, dg, ubo, W + 1, H, torch.zeros((H, W + 1, 4), device="cuda"))  # another image size
    fewer = {k: v[:10].contiguous() for k, v in dg.items()}
    _rejected(renderer, fewer, ubo, W, H, dL)  # another count
    # the frame is still the latest one: the rejected calls changed nothing
    ok = renderer.splat_gaussians_backward(dg, ubo, W, H, dL, bg=c["bg"])
    torch.cuda.synchronize()
    assert R.rel_l2(ok["colors"].cpu().numpy(), c["r64"]["grads"]["colors"]) < 1e-4
    # count == 0: PTGS_OK, nothing launched
    empty = {k: v[:0].contiguous() for k, v in dg.items()}
    rc, t = _raw_backward(renderer, empty, ubo, W, H, dL, n=0)
    assert rc == 0 and all(bool((v == 7.0).all()) for v in t.values())
    assert renderer.splat_gaussians_backward(empty, ubo, W, H, dL)["means"].shape == (0, 3)


SAME_KERNELS = 1e-5  # relative L2 between two runs of the same kernels: only the atomics' order differs


def _backward(renderer, c, dL=None, **kw):
    """Forward (published, with stats) and backward of a case on the given renderer: numpy gradients."""
    dg, _ = _forward(renderer, c)
    got = renderer.splat_gaussians_backward(dg, c["ubo"], c["W"], c["H"], _dev(c["dL"] if dL is None else dL),
                                            bg=c["bg"], want_means2d=True, want_conics=True, **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def test_backward_is_linear_in_the_upstream_gradient(renderer, oracle_lib):
    """backward(2 dL) = 2 backward(dL) and backward(0) = 0 exactly: an accumulator that is not cleared, or a term
    that does not scale with dL, breaks one of the two."""
    c = R.case_reference("clamp", oracle_lib)
    once = _backward(renderer, c)
    twice = _backward(renderer, c, dL=2.0 * c["dL"])
    zero = _backward(renderer, c, dL=np.zeros_like(c["dL"]))
    for k in R.GRAD_KEYS:
        err = R.rel_l2(twice[k], 2.0 * once[k].astype(np.float64))
        print(f"linearity {k}: {err:.2e}")
        assert np.linalg.norm(once[k]) > 0 and err < SAME_KERNELS, (k, err)
        assert not np.any(zero[k]), k


def test_backward_overwrites_its_outputs(renderer, oracle_lib):
    """A successful raw call into sentinel-filled arrays leaves no sentinel: every element is written, the culled
    Gaussians' with exactly 0."""
    c = R.case_reference("edges", oracle_lib)
    dg, _ = _forward(renderer, c)
    dL = _dev(c["dL"])
    rc, t = _raw_backward(renderer, dg, c["ubo"], c["W"], c["H"], dL)
    assert rc == 0
    want = renderer.splat_gaussians_backward(dg, c["ubo"], c["W"], c["H"], dL)  # (the raw call's bg: zero)
    torch.cuda.synchronize()
    culled = c["frame"]["radii"] == 0
    assert culled.any()
    for k, v in t.items():
        a = v.cpu().numpy().reshape(len(culled), -1)
        assert not np.any(a == 7.0), k
        assert not np.any(a[culled]), k
        assert R.rel_l2(a, want[k].cpu().numpy().reshape(a.shape)) < SAME_KERNELS, k


def test_backward_after_a_larger_frame(renderer, oracle_lib):
    """clamp -> deep -> clamp on one renderer (86, 830, 86 Gaussians; lists of at most 60, 530, 60): the scratch
    sized and filled by the larger frame leaves nothing behind in the smaller one."""
    small, large = R.case_reference("clamp", oracle_lib), R.case_reference("deep", oracle_lib)
    assert len(small["g"]["means"]) < len(large["g"]["means"]) and small["frame"]["K"] < large["frame"]["K"]
    first = _backward(renderer, small)
    between = _backward(renderer, large)
    again = _backward(renderer, small)
    for k in R.GRAD_KEYS:
        assert R.rel_l2(between[k].reshape(large["r64"]["grads"][k].shape), large["r64"]["grads"][k]) < 1e-4, k
        err = R.rel_l2(again[k], first[k])
        print(f"clamp after deep {k}: {err:.2e}")
        assert err < SAME_KERNELS, (k, err)


@pytest.mark.parametrize("name", ["opaque", "posed"])
def test_autograd_matches_the_direct_call(renderer, oracle_lib, name):
    c = R.case_reference(name, oracle_lib)
    W, H = c["W"], c["H"]
    dg, _ = _forward(renderer, c)
    dL = _dev(c["dL"])
    direct = renderer.splat_gaussians_backward(dg, c["ubo"], W, H, dL, bg=c["bg"])
    leaves = {k: v.clone().requires_grad_(k != "rotations") for k, v in dg.items()}
    img = autograd.splat(renderer, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"],
                         leaves["colors"], c["ubo"], W, H, bg=c["bg"])
    assert img.shape == (H, W, 4) and R.rel_l2(img.detach().cpu().numpy(), c["frame"]["image"]) < 1e-4
    (img * dL).sum().backward()
    torch.cuda.synchronize()
    assert leaves["rotations"].grad is None  # (an input that does not require grad gets None)
    for k in ("means", "scales", "opacities", "colors"):
        # the same kernels on the same frame: only the atomics' order differs (a few ulp of f32 per sum)
        err = R.rel_l2(leaves[k].grad.cpu().numpy(), direct[k].cpu().numpy())
        print(f"autograd vs direct {k}: {err:.2e}")
        assert err < 1e-5, (k, err)


def test_autograd_rejects_an_intervening_frame(renderer, oracle_lib):
    c = R.case_reference("edges", oracle_lib)
    dg = {k: _dev(v) for k, v in c["g"].items()}
    col = dg["colors"].clone().requires_grad_(True)
    img = autograd.splat(renderer, dg["means"], dg["scales"], dg["rotations"], dg["opacities"], col, c["ubo"],
                         c["W"], c["H"], bg=c["bg"])
    _forward(renderer, c, dg, want_stats=False)  # another splat call between forward and backward
    with pytest.raises(PtgsError):
        img.sum().backward()


def test_adam_steps_reduce_the_loss(renderer, oracle_lib):
    """30 Adam steps on colours and opacities towards a 64x48 target rendered from the true parameters."""
    c = R.case_reference("batches", oracle_lib)
    W, H = c["W"], c["H"]
    dg, target = _forward(renderer, c)
    torch.manual_seed(3)
    colors = (dg["colors"] * 0.5 + 0.25 * torch.rand_like(dg["colors"])).requires_grad_(True)
    opac = (dg["opacities"] * 0.6 + 0.1).requires_grad_(True)
    opt = torch.optim.Adam([colors, opac], lr=0.02)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        img = autograd.splat(renderer, dg["means"], dg["scales"], dg["rotations"], opac, colors, c["ubo"], W, H,
                             bg=c["bg"])
        loss = ((img - target) ** 2).sum()
        loss.backward()
        opt.step()
        with torch.no_grad():
            opac.clamp_(0.01, 0.99)
        losses.append(float(loss.detach()))
    print(f"adam: loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
