"""ptgs_image_loss_l1_dssim on the GPU against the float64 reference of tests/loss_ref.py, Renderer.l1_dssim_loss,
autograd.l1_dssim, and the loss inside an Adam loop.

Sizes. A workgroup owns a tile of T x T = 32 x 32 pixels with a 5-pixel halo; the final sum walks the per-workgroup
pairs STEP = 256 at a time with a carry. 1 x 1 and 3 x 7 are smaller than the window; T x T is one full tile whose
halo is all padding; (T + 3) x (2 T + 1) has ragged right and bottom tiles; 5 x 257 and 257 x 5 have many tiles in
one direction and are thinner than the halo in the other; 67 x 131 has interior tiles whose halo is all real pixels;
3 x (STEP * T + 1) = 3 x 8193 has 257 workgroups, one more than the final sum takes in one step, so its carry is used.

Tolerance. No constant is fixed in advance: per case e32 is the error of the float32 F.conv2d formulation on the CPU
against the float64 reference (relative L2 for the gradient, relative for each term), and the kernels must be within
4 * e32 + 1e-7 of the reference (the factor for the separable summation order, the floor for an e32 near zero).
lambda is the float32 value the C call receives, in the reference and in the float32 formulation alike."""
import ctypes as C
import functools

import numpy as np
import pytest

import loss_ref as L
from pathtracer_gaussiansplatting_amd import PtgsError, autograd

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
T, STEP = 32, 256
SENTINEL = 7.0
GUARD = 1024  # floats (a multiple of 4: the guarded view keeps the buffer's 16-byte alignment)
SHAPES = [(1, 1), (3, 7), (T, T), (T + 3, 2 * T + 1), (5, 257), (257, 5), (67, 131), (3, STEP * T + 1)]
LAMBDAS = (0.0, 0.2, 1.0)
GRAD_SCALES = (1.0, 2.5)


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (C = 4; the C = 3 target is its first three channels) and the lambda-independent reference parts."""
    image, target4 = L.make_inputs(*shape, 4, seed=7)
    return image, target4, L.parts(image, target4)


def _target(target4, c):
    return target4 if c == 4 else np.ascontiguousarray(target4[..., :3])


def _dev(a, offset=0):
    """A device copy of `a` whose base is `offset` floats past a 16-byte boundary."""
    flat = torch.from_numpy(np.array(a)).reshape(-1)
    buf = torch.empty(flat.numel() + offset, dtype=torch.float32, device="cuda")
    v = buf[offset:]
    v.copy_(flat)
    assert v.data_ptr() % 16 == 4 * offset
    return v.view(a.shape)


def _guarded(shape, offset=0):
    n = int(np.prod(shape))
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD + offset:GUARD + offset + n].view(shape)


def _guards_intact(buf, shape, offset=0):
    n = int(np.prod(shape))
    return bool((buf[:GUARD + offset] == SENTINEL).all()) and bool((buf[GUARD + offset + n:] == SENTINEL).all())


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_loss_and_gradient_against_the_reference(renderer, shape, C):
    image, target4, parts = _case(shape)
    target = _target(target4, C)
    d_img, d_tgt = _dev(image), _dev(target)
    H, W = shape
    for lam in LAMBDAS:
        lam = float(F(lam))
        for gs in GRAD_SCALES:
            ref = L.combine(parts, lam, gs)
            e32 = L.eager(image, target, lam, gs, "float32")
            buf, grad = _guarded((H, W, 4))
            tbuf, terms = _guarded((4,))
            t, g = renderer.l1_dssim_loss(d_img, d_tgt, lam=lam, grad_out=grad, grad_scale=gs, terms_out=terms)
            assert t is terms and g is grad
            t2, none = renderer.l1_dssim_loss(d_img, d_tgt, lam=lam)
            assert none is None
            buf3, grad3 = _guarded((H, W, 4))
            t3, _ = renderer.l1_dssim_loss(d_img, d_tgt, lam=lam, grad_out=grad3, grad_scale=gs)
            torch.cuda.synchronize()
            assert _guards_intact(buf, (H, W, 4)) and _guards_intact(tbuf, (4,)) and _guards_intact(buf3, (H, W, 4))
            assert torch.equal(t2, terms), "loss-only terms differ from the terms of the call with the gradient"
            assert torch.equal(t3, terms) and torch.equal(grad3, grad), "two runs differ"
            got_t, got_g = terms.cpu().numpy().astype(np.float64), grad.cpu().numpy()
            assert got_t[3] == 0.0
            assert not got_g[..., 3].any(), "alpha of the gradient is not 0"
            assert not (got_g[..., :3] == SENTINEL).any()
            for k, name in enumerate(("loss", "l1", "ssim")):
                err, bound = L.rel(got_t[k], ref[k]), 4 * L.rel(e32[k], ref[k]) + 1e-7
                print(f"{H}x{W} C={C} lam={lam:.1f} gs={gs} {name}: {err:.2e} (e32 {L.rel(e32[k], ref[k]):.2e})")
                assert err <= bound, (name, err, bound)
            err, e = L.rel_l2(got_g, ref[3]), L.rel_l2(e32[3], ref[3])
            print(f"{H}x{W} C={C} lam={lam:.1f} gs={gs} grad: {err:.2e} (e32 {e:.2e})")
            assert err <= 4 * e + 1e-7, (err, e)


def test_unaligned_bases_give_the_same_bits(renderer):
    """Bases 4 bytes past a 16-byte boundary take the scalar loads and stores: the same arithmetic."""
    shape = (T + 3, 2 * T + 1)
    image, target4, _ = _case(shape)
    want_t, want_g = renderer.l1_dssim_loss(_dev(image), _dev(target4), grad_out=torch.empty(shape + (4,), device="cuda"))
    buf, grad = _guarded(shape + (4,), offset=1)
    got_t, _ = renderer.l1_dssim_loss(_dev(image, 1), _dev(target4, 1), grad_out=grad)
    torch.cuda.synchronize()
    assert torch.equal(got_t, want_t) and torch.equal(grad, want_g) and _guards_intact(buf, shape + (4,), 1)


def test_argument_table(renderer):
    H, W = 6, 9
    image, target4, _ = _case((3, 7))
    img = torch.rand((H, W, 4), device="cuda")
    tgt = torch.rand((H, W, 4), device="cuda")
    terms = torch.zeros(4, device="cuda")
    grad = torch.full((H, W, 4), SENTINEL, device="cuda")
    host = np.zeros(H * W * 4, F)
    fn, h = renderer.lib.ptgs_image_loss_l1_dssim, renderer._h
    ok = dict(ctx=h, image=img.data_ptr(), target=tgt.data_ptr(), c=4, w=W, h=H, lam=0.2, gs=1.0,
              out=terms.data_ptr(), grad=grad.data_ptr())

    def call(**kw):
        a = dict(ok, **kw)
        return fn(a["ctx"], a["image"], a["target"], a["c"], a["w"], a["h"], a["lam"], a["gs"], a["out"], a["grad"], None)

    bad = [dict(ctx=None), dict(image=None), dict(target=None), dict(out=None), dict(w=0), dict(h=0), dict(w=16385),
           dict(h=16385), dict(c=2), dict(c=5), dict(c=0), dict(lam=float("nan")), dict(lam=-0.01), dict(lam=1.01),
           dict(gs=float("inf")), dict(gs=float("nan")), dict(grad=img.data_ptr()), dict(grad=tgt.data_ptr()),
           dict(grad=img.data_ptr() + 16 * (H * W - 1)), dict(grad=tgt.data_ptr() - 16 * (H * W - 1)),
           dict(out=host.ctypes.data), dict(grad=host.ctypes.data)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert bool((grad == SENTINEL).all()) and not bool(terms.any()), "a rejected call wrote something"
    assert call() == 0 and call(grad=None) == 0 and call(lam=0.0) == 0 and call(lam=1.0, gs=-3.0) == 0
    torch.cuda.synchronize()
    # the Python layer's own checks
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img[..., :3].contiguous(), tgt)
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img, tgt[:, :, :2].contiguous())
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img, tgt[:5].contiguous())
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img.double(), tgt)
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img, tgt, grad_out=torch.empty((H, W, 3), device="cuda"))
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img, tgt, terms_out=torch.empty(3, device="cuda"))
    with pytest.raises(PtgsError):
        renderer.l1_dssim_loss(img, tgt, lam=1.5)


def test_autograd_on_a_leaf_image(renderer):
    shape = (T + 3, 2 * T + 1)
    image, target4, _ = _case(shape)
    d_tgt = _dev(target4)
    terms, grad = renderer.l1_dssim_loss(_dev(image), d_tgt, grad_out=torch.empty(shape + (4,), device="cuda"))
    leaf = _dev(image).requires_grad_(True)
    loss = autograd.l1_dssim(renderer, leaf, d_tgt)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (2.5 * loss).backward()
    torch.cuda.synchronize()
    assert torch.equal(loss.detach(), terms[0])
    assert torch.equal(leaf.grad, grad * 2.5)
    with torch.no_grad():
        assert torch.equal(autograd.l1_dssim(renderer, leaf, d_tgt), terms[0])


LEARNING_RATES = {"means": 1e-3, "log_scales": 5e-3, "rotations": 1e-3, "opacity_logits": 0.05, "sh": 0.02}


def test_training_with_the_loss(renderer):
    """15 Adam steps over all five leaves of the `batches` checkpoint (perturbed SH and opacity logits) towards
    its own rendering, with autograd.l1_dssim as the loss."""
    import test_sh_backward_gpu as B
    p, g, ubo, W, H, bg, _ = B._checkpoint_case("batches")
    c = {"ubo": ubo, "W": W, "H": H, "bg": bg}
    d = {k: torch.from_numpy(np.array(p[k])).cuda() for k in B.PARAM_KEYS}
    with torch.no_grad():
        target = B._splat_sh(renderer, d, c).clone()
    torch.manual_seed(3)
    lv = dict(d)
    lv["sh"] = d["sh"] + 0.3 * torch.randn_like(d["sh"])
    lv["opacity_logits"] = d["opacity_logits"] * 0.6 - 0.3
    lv = {k: v.clone().requires_grad_(True) for k, v in lv.items()}
    opt = torch.optim.Adam([{"params": [lv[k]], "lr": LEARNING_RATES[k]} for k in B.PARAM_KEYS])
    losses = []
    for _ in range(15):
        opt.zero_grad()
        loss = autograd.l1_dssim(renderer, B._splat_sh(renderer, lv, c), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in torch.stack(losses).cpu()]
    print(f"l1_dssim training: first {losses[0]:.6f} last {losses[-1]:.6f}")
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
