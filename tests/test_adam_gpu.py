"""ptgs_gaussians_adam_step and ptgs_gaussians_opacity_reset on the GPU against the numpy float32 reference of
tests/adam_ref.py, bit for bit (the contract has no transcendental on the device and no atomics, so apart from the
subnormal check there is no tolerance in this file), and GaussianAdam inside a training loop with densification.

Sizes. A workgroup of the step covers BLOCK = 1024 elements (256 work-items x 4), floats or float4s. N = 1 025 with
width 1 has a second block holding one element; N = 6 145 has a ragged last block in every width; a table of several
rows makes a block find its segment."""
import ctypes as C

import numpy as np
import pytest

import adam_ref as A
from pathtracer_gaussiansplatting_amd import DensifyStats, GaussianAdam, PtgsError, _abi, densify_and_prune

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
BLOCK = 1024
SENTINEL = 7.0
GUARD = 1024
WIDTHS = (1, 3, 4, 27, 48)
WRITTEN = ("param", "exp_avg", "exp_avg_sq")
E = _abi.PTGS_EINVAL


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _placed(a, offset):
    """(buffer, view): a device copy of `a`, `offset` floats past a 16-byte boundary, sentinels around it."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.full((offset + flat.numel() + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    v = buf[offset:offset + flat.numel()]
    v.copy_(flat)
    assert v.data_ptr() % 16 == 4 * offset
    return buf, v


def _table(dev_rows):
    arr = (_abi.AdamRows * max(1, len(dev_rows)))()
    for k, (r, d) in enumerate(dev_rows):
        arr[k].param, arr[k].grad = d["param"][1].data_ptr(), d["grad"][1].data_ptr()
        arr[k].exp_avg, arr[k].exp_avg_sq = d["exp_avg"][1].data_ptr(), d["exp_avg_sq"][1].data_ptr()
        arr[k].width, arr[k].head = r["param"].shape[1], r["head"]
        arr[k].lr, arr[k].lr_head = float(r["lr"]), float(r["lr_head"])
    return arr


def _step_raw(renderer, rows, step, radii=None, offset=0, eps=1e-15, betas=(0.9, 0.999), steps=1):
    """The C call on raw pointers: every array `offset` floats past 16-byte alignment in a sentinel-filled buffer
    with guards. Returns (rc, [(param, exp_avg, exp_avg_sq) as numpy]); checks that nothing outside the arrays and
    no gradient changed, and that a rejected call changed nothing at all."""
    n = rows[0]["param"].shape[0]
    dev = [(r, {k: _placed(r[k], offset) for k in WRITTEN + ("grad",)}) for r in rows]
    arr = _table(dev)
    rd = None if radii is None else torch.from_numpy(np.asarray(radii, np.int32)).cuda()
    rc = 0
    for t in range(steps):
        prm = _abi.AdamParams(betas[0], betas[1], eps, step + t)
        rc = renderer.lib.ptgs_gaussians_adam_step(renderer._h, n, arr, len(rows), C.byref(prm),
                                                   None if rd is None else rd.data_ptr(), None)
        if rc != 0:
            break
    torch.cuda.synchronize()
    out = []
    for r, d in dev:
        got = {}
        for k, (buf, view) in d.items():
            b = buf.cpu().numpy()
            assert np.all(b[:offset] == SENTINEL) and np.all(b[offset + view.numel():] == SENTINEL), k
            got[k] = b[offset:offset + view.numel()].reshape(r[k].shape)
        assert np.array_equal(_bits(got["grad"]), _bits(r["grad"]))  # the gradients are read only
        if rc != 0:  # a rejected call enqueued nothing
            assert all(np.array_equal(_bits(got[k]), _bits(r[k])) for k in WRITTEN)
        out.append(tuple(got[k] for k in WRITTEN))
    if rd is not None:
        assert np.array_equal(rd.cpu().numpy(), radii)
    return rc, out


def _reference(rows, step, radii=None, eps=1e-15, steps=1):
    for t in range(steps):
        rows = A.adam_step(rows, step=step + t, eps=eps, radii=radii)
    return rows


def _same(got, ref):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        for name, a in zip(WRITTEN, g):  # (as integers: a NaN would not hide)
            assert np.array_equal(_bits(a), _bits(r[name])), (k, name)


# ---------------------------------------------------------------------------------------------------------
# the step
# ---------------------------------------------------------------------------------------------------------
SIZES = {"n1": (1, WIDTHS, None), "n257": (257, WIDTHS, "third"), "n1000": (1000, WIDTHS, "third"),
         "n1025-width1": (BLOCK + 1, (1,), "third"), "n6145": (6 * BLOCK + 1, WIDTHS, "third"),
         "n6145-dense": (6 * BLOCK + 1, WIDTHS, None)}


@pytest.mark.parametrize("name", list(SIZES))
def test_step_matches_the_reference(renderer, name):
    n, widths, mask = SIZES[name]
    rows = A.make_rows(n, widths)
    radii = A.make_radii(n, mask) if mask else None
    rc, got = _step_raw(renderer, rows, 3, radii)
    assert rc == 0
    ref = _reference(rows, 3, radii)
    _same(got, ref)
    if n > 1:
        assert all(not np.array_equal(r["param"], o["param"]) for r, o in zip(ref, rows))
    if radii is not None:  # invisible Gaussians are untouched in every written array
        hidden = radii <= 0
        assert hidden.any() and (~hidden).any() and (radii < 0).any()
        for g, o in zip(got, rows):
            for name_, a in zip(WRITTEN, g):
                assert np.array_equal(_bits(a[hidden]), _bits(o[name_][hidden]))


@pytest.mark.parametrize("width", WIDTHS)
def test_each_width_alone(renderer, width):
    rows = A.make_rows(1000, (width,), seed=width)
    radii = A.make_radii(1000, "third")
    rc, got = _step_raw(renderer, rows, 2, radii)
    assert rc == 0
    _same(got, _reference(rows, 2, radii))


def test_sixteen_rows_and_the_seventeenth(renderer):
    widths = (48, 1, 3, 4, 27, 12, 8, 2, 5, 16, 1, 3, 48, 7, 4, 9)
    rows = A.make_rows(257, widths, seed=16)
    assert len(rows) == _abi.ADAM_MAX_ROWS
    radii = A.make_radii(257, "third")
    rc, got = _step_raw(renderer, rows, 4, radii)
    assert rc == 0
    _same(got, _reference(rows, 4, radii))
    rc, _ = _step_raw(renderer, rows + A.make_rows(257, (2,)), 4, radii)
    assert rc == E and b"n_rows 17" in renderer.lib.ptgs_last_error(renderer._h)


def test_head_rates_on_the_wide_row(renderer):
    """head 0, 3 and 48 on 48-wide rows: with head 3 the first float4 of every row mixes the two rates."""
    rows = A.make_rows(1000, (48, 48, 48), heads=(0, 3, 48), seed=4)
    assert [r["head"] for r in rows] == [0, 3, 48] and rows[1]["lr"] != rows[1]["lr_head"]
    rc, got = _step_raw(renderer, rows, 1)
    assert rc == 0
    ref = _reference(rows, 1)
    _same(got, ref)
    same_state = [A.row(rows[0]["param"], rows[0]["grad"], rows[0]["exp_avg"], rows[0]["exp_avg_sq"], r["lr"], r["head"],
                        r["lr_head"]) for r in rows]
    a, b, c = (r["param"] for r in _reference(same_state, 1))
    assert np.array_equal(b[:, 3:], a[:, 3:]) and np.array_equal(b[:, :3], c[:, :3]) and not np.array_equal(a, c)


def test_misaligned_bases_take_the_scalar_path(renderer):
    """Every base 4 bytes past a 16-byte boundary, where a 16-byte access would fault or tear: the same bits."""
    rows = A.make_rows(1000, WIDTHS)
    radii = A.make_radii(1000, "third")
    rc0, aligned = _step_raw(renderer, rows, 5, radii, offset=0)
    rc1, shifted = _step_raw(renderer, rows, 5, radii, offset=1)
    assert rc0 == 0 and rc1 == 0
    ref = _reference(rows, 5, radii)
    _same(aligned, ref)
    _same(shifted, ref)


def test_masks(renderer):
    n = 1000
    rows = A.make_rows(n, WIDTHS)
    rc, dense = _step_raw(renderer, rows, 7)
    assert rc == 0
    _same(dense, _reference(rows, 7))
    # none visible: every written array is bit-equal to its input
    rc, got = _step_raw(renderer, rows, 7, A.make_radii(n, "none"))
    assert rc == 0
    for g, o in zip(got, rows):
        for name, a in zip(WRITTEN, g):
            assert np.array_equal(_bits(a), _bits(o[name]))
    # all visible: the dense call
    rc, got = _step_raw(renderer, rows, 7, A.make_radii(n, "all"))
    assert rc == 0
    for g, d in zip(got, dense):
        assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(g, d))
    # the visible rows of a masked call are the same rows of the dense call; alternate: the fate changes within one
    # float4 group of a narrow row
    for kind in ("third", "alternate"):
        radii = A.make_radii(n, kind)
        vis = radii > 0
        rc, got = _step_raw(renderer, rows, 7, radii)
        assert rc == 0
        _same(got, _reference(rows, 7, radii))
        for g, d, o in zip(got, dense, rows):
            for name, a, b in zip(WRITTEN, g, d):
                assert np.array_equal(_bits(a[vis]), _bits(b[vis]))
                assert np.array_equal(_bits(a[~vis]), _bits(o[name][~vis]))
    assert np.array_equal(A.make_radii(n, "alternate")[:4] > 0, [True, False, True, False])


@pytest.mark.parametrize("step", [1, 2, 1000, 100_000])
def test_steps(renderer, step):
    """100 000: both bias corrections are exactly 1."""
    rows = A.make_rows(257, WIDTHS, warm=step > 1)
    rc, got = _step_raw(renderer, rows, step)
    assert rc == 0
    _same(got, _reference(rows, step))


def test_ten_steps_in_place_and_two_runs(renderer):
    rows = A.make_rows(1000, WIDTHS, warm=False)
    radii = A.make_radii(1000, "third")
    runs = [_step_raw(renderer, rows, 1, radii, steps=10) for _ in range(2)]
    assert runs[0][0] == 0 and runs[1][0] == 0
    _same(runs[0][1], _reference(rows, 1, radii, steps=10))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))
    rc, got = _step_raw(renderer, rows, 1, radii, eps=1e-8, steps=2)
    assert rc == 0
    _same(got, _reference(rows, 1, radii, eps=1e-8, steps=2))


def test_subnormal_territory_stays_finite(renderer):
    """g = 1e-25: g * g underflows and (ob2 * g) * g is subnormal or zero. Outside the bit-exact claim; the
    outputs are finite and the parameters move by at most their rate."""
    rows = A.make_rows(257, WIDTHS, warm=False)
    rows = [{**r, "grad": np.full_like(r["grad"], 1e-25)} for r in rows]
    rc, got = _step_raw(renderer, rows, 1)
    assert rc == 0
    for (p, m, v), r in zip(got, rows):
        assert np.isfinite(p).all() and np.isfinite(m).all() and np.isfinite(v).all()
        rate = max(float(r["lr"]), float(r["lr_head"]))
        assert np.abs(p.astype(np.float64) - r["param"]).max() <= 1.001 * rate + 1e-6


# ---------------------------------------------------------------------------------------------------------
# the reset
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", ["both", "neither"])
@pytest.mark.parametrize("n", [1, 257, 6145])
def test_opacity_reset(renderer, n, moments):
    x, m, v = A.reset_case(n)
    dx, dm, dv = _placed(x, 1), _placed(m, 1), _placed(v, 1)
    with_m = moments == "both"
    rc = renderer.lib.ptgs_gaussians_opacity_reset(renderer._h, dx[1].data_ptr(), n, 0.01,
                                                   dm[1].data_ptr() if with_m else None,
                                                   dv[1].data_ptr() if with_m else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    ref, _, _ = A.opacity_reset(x, 0.01)
    host = []
    for buf, view in (dx, dm, dv):
        b = buf.cpu().numpy()
        assert np.all(b[:1] == SENTINEL) and np.all(b[1 + n:] == SENTINEL)
        host.append(b[1:1 + n])
    assert np.array_equal(_bits(host[0]), _bits(ref))
    if with_m:
        assert not host[1].any() and not host[2].any()
    else:
        assert np.array_equal(_bits(host[1]), _bits(m)) and np.array_equal(_bits(host[2]), _bits(v))
    cap = A.reset_cap(0.01)
    if n > 1:
        assert np.isnan(ref).sum() == 1 and (ref == cap).sum() > 2 and (ref < cap).any()
        assert np.nextafter(cap, F(-np.inf)) in ref and not (ref > cap).any()
    else:
        assert x[0] > cap and ref[0] == cap


# ---------------------------------------------------------------------------------------------------------
# the argument tables of include/ptgs/ptgs.h, row by row
# ---------------------------------------------------------------------------------------------------------
def test_argument_table_of_the_step(renderer):
    L = renderer.lib
    err = lambda: L.ptgs_last_error(renderer._h)  # noqa: E731
    n, w = 257, 4
    full = lambda: torch.full((n * w,), SENTINEL, device="cuda")  # noqa: E731
    p, g, m, v = full(), full(), full(), full()
    radii = torch.ones(n, dtype=torch.int32, device="cuda")
    host = np.zeros(n * w, F)

    def call(param=p, grad=g, exp_avg=m, exp_avg_sq=v, width=w, head=0, lr=0.01, lr_head=0.0, step=1, beta1=0.9,
             beta2=0.999, eps=1e-15, n_rows=1, ctx=renderer._h, rows=True, params=True, rad=None, count=n):
        ptr = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        arr = (_abi.AdamRows * 17)()
        for k in range(17):
            arr[k].param, arr[k].grad, arr[k].exp_avg, arr[k].exp_avg_sq = ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq)
            arr[k].width, arr[k].head, arr[k].lr, arr[k].lr_head = width, head, lr, lr_head
        prm = _abi.AdamParams(beta1, beta2, eps, step)
        return L.ptgs_gaussians_adam_step(ctx, count, arr if rows else None, n_rows, C.byref(prm) if params else None,
                                          ptr(rad), None)

    def rejected(msg=None, **kw):
        """PTGS_EINVAL with `msg` in ptgs_last_error, and every array still holds its sentinels."""
        assert call(**kw) == E, kw
        assert msg is None or msg in err(), (kw, err())
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (p, g, m, v)), kw

    nan, inf = float("nan"), float("inf")
    rejected(ctx=None)
    rejected(b"null", rows=False)
    rejected(b"null", params=False)
    rejected(b"n_rows 0", n_rows=0)
    rejected(b"n_rows 17", n_rows=17)
    for name in ("param", "grad", "exp_avg", "exp_avg_sq"):
        rejected(b"null", **{name: None})
    rejected(b"width 0", width=0)
    rejected(b"head", head=w + 1)
    rejected(b"step 0", step=0)
    for bad in (nan, -0.1, 1.0, 1.5):
        rejected(b"beta", beta1=bad)
        rejected(b"beta", beta2=bad)
    for bad in (nan, -1e-8, inf):
        rejected(b"eps", eps=bad)
    for bad in (nan, inf, -inf):
        rejected(b"not finite", lr=bad)
        rejected(b"not finite", lr_head=bad)
    # a written array overlapping another array of the table, or the radii
    rejected(b"overlaps", grad=p)
    rejected(b"overlaps", exp_avg=p)
    rejected(b"overlaps", exp_avg_sq=m)
    rejected(b"overlaps", exp_avg=g.data_ptr() + 16)
    rejected(b"overlaps", param=v.data_ptr() + 4 * (n * w - 1))  # by one float
    rejected(b"overlaps", n_rows=2)  # the same row twice
    rejected(b"overlaps", rad=m)
    for name in WRITTEN:
        rejected(b"not a device pointer", **{name: host.ctypes.data})
    rejected(count=0, rows=False)
    # n == 0: PTGS_OK before the rows' pointers are looked at
    assert call(count=0, param=None, grad=None, exp_avg=None, exp_avg_sq=None) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (p, g, m, v))
    # what the table accepts: head == width, eps == 0, beta == 0
    assert call(head=w, lr_head=0.5, eps=0.0, beta1=0.0, beta2=0.0, rad=radii) == 0
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((p == SENTINEL - 0.5).all())  # m' = g, v' = g * g: one rate down
    # the Python layer
    t4 = lambda: torch.zeros((n, w), device="cuda")  # noqa: E731
    with pytest.raises(PtgsError):
        renderer.adam_step([], step=1)
    with pytest.raises(PtgsError):
        renderer.adam_step([(t4(), t4(), t4(), t4(), 0.01)] * 17, step=1)
    with pytest.raises(PtgsError):
        renderer.adam_step([(t4(), t4().double(), t4(), t4(), 0.01)], step=1)
    with pytest.raises(PtgsError):
        renderer.adam_step([(t4(), t4(), t4(), t4(), 0.01)], step=1, radii=torch.ones(n + 1, dtype=torch.int32, device="cuda"))
    with pytest.raises(PtgsError) as e:
        renderer.adam_step([(t4(), t4(), t4(), t4(), 0.01)], step=0)
    assert e.value.code == E


def test_argument_table_of_the_reset(renderer):
    L = renderer.lib
    err = lambda: L.ptgs_last_error(renderer._h)  # noqa: E731
    n = 257
    x, m, v = (torch.full((n,), SENTINEL, device="cuda") for _ in range(3))
    host = np.zeros(n, F)
    call = lambda lx=x.data_ptr(), mo=0.01, a=m.data_ptr(), b=v.data_ptr(), ctx=renderer._h, count=n: \
        L.ptgs_gaussians_opacity_reset(ctx, lx, count, mo, a, b, None)  # noqa: E731
    def rejected(msg=None, **kw):
        assert call(**kw) == E, kw
        assert msg is None or msg in err(), (kw, err())
        torch.cuda.synchronize()
        assert all(bool((t == SENTINEL).all()) for t in (x, m, v)), kw  # a rejected call enqueued nothing

    rejected(ctx=None)
    rejected(b"null", lx=None)
    for bad in (float("nan"), 0.0, 1.0, -0.5, 2.0):
        rejected(b"max_opacity", mo=bad)
    rejected(b"overlap", a=x.data_ptr())
    rejected(b"overlap", b=m.data_ptr() + 4)
    rejected(b"overlap", b=x.data_ptr() + 4 * (n - 1))
    rejected(b"not a device pointer", lx=host.ctypes.data)
    rejected(b"not a device pointer", a=host.ctypes.data)
    rejected(b"not a device pointer", b=host.ctypes.data)
    assert call(count=0, lx=None, a=None, b=None) == 0
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in (x, m, v))
    assert call(a=None, b=None) == 0
    torch.cuda.synchronize()
    assert bool((x == float(A.reset_cap(0.01))).all()) and bool((m == SENTINEL).all())
    with pytest.raises(PtgsError):
        renderer.opacity_reset(x, 0.01, exp_avg=torch.zeros(n + 1, device="cuda"))
    with pytest.raises(PtgsError) as e:
        renderer.opacity_reset(x, 1.5)
    assert e.value.code == E


# ---------------------------------------------------------------------------------------------------------
# GaussianAdam on a checkpoint
# ---------------------------------------------------------------------------------------------------------
# the rates of test_densify_gpu.py's Adam loop, and the trainer's f_dc : f_rest = 20 : 1 for the coefficients
LEARNING_RATES = {"means": 1e-3, "log_scales": 5e-3, "rotations": 1e-3, "opacity_logits": 0.05, "sh": 0.02 / 20,
                  "sh_dc": 0.02}
PERCENT_DENSE = 0.01


# The two tests that render use the session's context. They once had one of their own: this file runs before
# test_configs_gpu.py, whose C4 hybrid frame (1M Gaussians, 1920 x 1080, `over` in place, with stats) came out
# wrong after a small published frame. The cause was not the buffers' sizes: such a frame leaves small fused rows,
# the C4 frame overflowed them and was re-run inside its call, and the second blend composited over the first
# one's result. A call with stats now blends over a copy of `under` (tests/test_splat_over_gpu.py).


def _frame_radii(renderer, n):
    torch.cuda.synchronize()
    b = renderer.splat_buffers()
    assert b.num_gaussians == n
    radii = np.zeros(n, np.int32)
    renderer.copy_d2h(radii, b.radii, 4 * n)
    return radii


def test_gaussian_adam_one_step_from_a_backward(renderer):
    """One backward of autograd.splat_sh on the `batches` checkpoint (N = 520), then a dense step: bit for bit the
    reference applied to those .grad tensors; and a masked step with the frame's radii from the same state leaves
    the Gaussians of radius 0 untouched."""
    import test_sh_backward_gpu as B
    p, g, ubo, W, H, bg, dL = B._checkpoint_case("batches")
    n = len(p["means"])
    assert n == 520
    behind = [3, 100, 519]  # the case's own Gaussians are all in view: these three go behind the camera
    p = {**p, "means": p["means"].copy()}
    p["means"][behind] = [0.3, -0.2, 3.0]
    c = {"ubo": ubo, "W": W, "H": H, "bg": bg}
    dLd = torch.from_numpy(dL).cuda()
    M0, V0 = F(1e-3), F(1e-6)  # warm moments: a dense step moves a Gaussian whose gradient is zero too
    for masked in (False, True):
        lv = B._leaves(p)
        opt = GaussianAdam(lv, LEARNING_RATES)
        for k in B.PARAM_KEYS:
            opt.exp_avg[k].fill_(float(M0))
            opt.exp_avg_sq[k].fill_(float(V0))
        opt.step_count = 4
        opt.zero_grad()
        img = B._splat_sh(renderer, lv, c)
        (img * dLd).sum().backward()
        grads = {k: lv[k].grad.cpu().numpy().copy() for k in B.PARAM_KEYS}
        radii = _frame_radii(renderer, n)
        hidden = radii <= 0
        assert hidden[behind].all() and (~hidden).sum() > 400
        versions = {k: lv[k]._version for k in B.PARAM_KEYS}
        opt.step(renderer, masked=masked)
        torch.cuda.synchronize()
        assert opt.step_count == 5
        full = lambda k, x: np.full((n, p[k].size // n), x, F)  # noqa: E731
        rows = [A.row(p[k].reshape(n, -1), grads[k].reshape(n, -1), full(k, M0), full(k, V0), LEARNING_RATES[k],
                      3 if k == "sh" else 0, LEARNING_RATES["sh_dc"] if k == "sh" else 0.0) for k in B.PARAM_KEYS]
        ref = A.adam_step(rows, step=5, radii=radii if masked else None)
        for k, r in zip(B.PARAM_KEYS, ref):
            got = lv[k].detach().cpu().numpy().reshape(n, -1)
            assert np.array_equal(_bits(got), _bits(r["param"])), k
            assert np.array_equal(_bits(opt.exp_avg[k].cpu().numpy().reshape(n, -1)), _bits(r["exp_avg"])), k
            assert np.array_equal(_bits(opt.exp_avg_sq[k].cpu().numpy().reshape(n, -1)), _bits(r["exp_avg_sq"])), k
            assert np.array_equal(_bits(lv[k].grad.cpu().numpy()), _bits(grads[k]))  # the gradients are read only
            assert lv[k]._version > versions[k]  # autograd knows the leaf changed
            before = p[k].reshape(n, -1)
            assert not np.array_equal(got[~hidden], before[~hidden])
            if masked:  # radius 0: untouched, moments included
                assert np.array_equal(_bits(got[hidden]), _bits(before[hidden]))
                assert bool((opt.exp_avg[k][torch.from_numpy(hidden).cuda()] == float(M0)).all())
                assert bool((opt.exp_avg_sq[k][torch.from_numpy(hidden).cuda()] == float(V0)).all())
            else:
                assert not np.array_equal(got[hidden], before[hidden])
    # a leaf without a gradient is skipped; a frame of another size cannot mask
    lv = B._leaves(p)
    opt = GaussianAdam(lv, LEARNING_RATES)
    lv["sh"].grad = torch.ones_like(lv["sh"])
    opt.step(renderer, masked=False)
    torch.cuda.synchronize()
    assert np.array_equal(lv["means"].detach().cpu().numpy(), p["means"]) and opt.step_count == 1
    assert not np.array_equal(lv["sh"].detach().cpu().numpy(), p["sh"])
    opt.zero_grad()
    assert lv["sh"].grad is None
    small = {k: v.detach()[:100].clone().requires_grad_(True) for k, v in lv.items()}
    opt2 = GaussianAdam(small, LEARNING_RATES)
    small["sh"].grad = torch.ones_like(small["sh"])
    with pytest.raises(PtgsError):
        opt2.step(renderer, masked=True)
    with pytest.raises(PtgsError):
        opt2.set_lr("colors", 0.1)
    opt2.set_lr("means", 0.5)
    assert opt2.lr["means"] == 0.5


def test_gaussian_adam_densify_reset_adam(renderer):
    """test_adam_densify_adam of test_densify_gpu.py with GaussianAdam, the DC term at its own rate and the masked
    step: 15 steps with the statistic, densify_and_prune at the statistic's median, reset_opacity(0.01), 15 more
    steps. Measured: loss 22.2530 -> 8.8953, then (520 -> 781 Gaussians, every opacity at most 0.01) 174.0835 ->
    151.7356."""
    import densify_ref as D
    import test_sh_backward_gpu as B
    lr = LEARNING_RATES
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
    opt = GaussianAdam(lv, lr)
    n = len(p["means"])
    stats = DensifyStats(n)
    losses = []

    def steps(lv, stats, count):
        for _ in range(count):
            opt.zero_grad()
            m2d = torch.zeros((lv["means"].shape[0], 2), dtype=torch.float32, device="cuda")
            img = B._splat_sh(renderer, lv, c, means2d_grad=m2d)
            loss = ((img - target) ** 2).sum()
            loss.backward()
            opt.step(renderer, masked=True)
            stats.update(renderer, m2d, W, H)
            losses.append(float(loss.detach()))

    steps(lv, stats, 15)
    assert opt.step_count == 15
    seen = stats.denom > 0
    assert bool(seen.any()) and float(stats.denom.max()) == 15.0
    thr = float((stats.accum[seen] / stats.denom[seen]).median())
    extent = float((d["means"] - d["means"].mean(dim=0)).norm(dim=1).max())
    before = {k: {m: getattr(opt, m)[k].clone() for m in ("exp_avg", "exp_avg_sq")} for k in B.PARAM_KEYS}
    old = {k: v.detach().clone() for k, v in lv.items()}
    sc, _ = renderer.activate_gaussians(old["log_scales"], old["opacity_logits"])
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    new, counts, stats2 = densify_and_prune(renderer, lv, stats, grad_threshold=thr, scale_split=PERCENT_DENSE * extent,
                                            min_opacity=0.005, optimizer=opt, generator=gen)
    nn = counts.total
    print("densify:", {k: int(getattr(counts, k)) for k in ("survivors", "clones", "split_sources", "total")})
    assert nn != n and counts.clones + counts.split_sources > 0 and stats2.n == nn
    _, _, _, src = renderer.densify_apply(nn, old["means"], old["log_scales"], old["rotations"], sc,
                                          torch.zeros((2, n, 3), device="cuda"), want_source=True)
    src = src.cpu().numpy().view(np.uint32)
    kind, idx = src >> np.uint32(D.KIND_SHIFT), (src & np.uint32((1 << D.KIND_SHIFT) - 1)).astype(np.int64)
    S = counts.survivors
    assert np.all(kind[:S] == 0) and np.all(kind[S:] != 0)
    keep = torch.from_numpy(idx[:S]).cuda()
    assert opt.step_count == 15
    for k in B.PARAM_KEYS:
        t = new[k]
        assert opt.params[k] is t and t.is_leaf and t.requires_grad and t.shape[0] == nn
        for m in ("exp_avg", "exp_avg_sq"):
            mom = getattr(opt, m)[k]
            assert mom.shape == t.shape
            assert torch.equal(mom[:S], before[k][m][keep])  # survivors keep their moments, bit for bit
            assert not bool(mom[S:].any())  # new rows start from zero
        assert bool(before[k]["exp_avg_sq"].any())
    opt.reset_opacity(renderer, 0.01)
    cap = float(A.reset_cap(0.01))
    logits = new["opacity_logits"].detach()
    assert bool((logits <= cap).all()) and bool((logits == cap).any())
    assert not bool(opt.exp_avg["opacity_logits"].any()) and not bool(opt.exp_avg_sq["opacity_logits"].any())
    steps(new, stats2, 15)
    print(f"adam / densify + reset / adam: loss {losses[0]:.4f} -> {losses[14]:.4f} | {losses[15]:.4f} -> {losses[-1]:.4f}")
    assert opt.step_count == 30 and len(losses) == 30 and np.isfinite(losses).all()
    assert losses[14] < losses[0]
    assert losses[-1] < losses[15]
    assert float(stats2.denom.max()) == 15.0
