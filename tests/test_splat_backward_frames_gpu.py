"""The 3DGS backward and the inverse-depth render on training-size frames, after each front end.

What a trainer does on every iteration and tests/test_splat_backward_gpu.py / test_splat_depth_gpu.py do not: the
frame the backward consumes is the second frame of a context (the fused front end: the rows compacted by
gs_publish_copy_kernel), a fused frame that overflowed its rows and was re-run through three launches, or a frame
whose lists went through the large-tile sort; the image is up to 1992 pixels wide or 1096 high (tile indices beyond
64, pixel coordinates that float32 resolves to 1.2e-4); the lists hold up to ten staged batches; the projection
backward runs 79 workgroups; a thousand pixels stop.

Every test opens its own Renderer, so the front end follows from the test's own frames and nothing else, and
asserts what ran from what the API reports (stats.fused, splat_status). The cases are
splat_grad_ref.FRAME_CASES: their upstream gradients are exactly 0 on the pixels where the float64 reference counts
a borderline decision (at most 1% of the image, tests/test_splat_grad_ref.py), so every other pixel is compared
with no allowance for decisions. Tolerances are the project's existing ones, unchanged:
splat_grad_ref.check_bounds (max(1e-4, 8 e32) on the whole array, each quarter by gradient norm and the clamped
subset, e32 from the case's own float32 reference), 1e-4 relative L2 for a blended map, 1e-5 between two runs of
the same kernels on the same lists.

The direct calls are the C entry points behind Renderer.splat_gaussians_backward(want_means2d=True,
want_conics=True[, dL_dinvdepth]) and splat_gaussians_invdepth, with every output array inside a sentinel-guarded
buffer."""
import ctypes as C

import numpy as np
import pytest

import splat_depth_ref as Z
import splat_grad_ref as R
from pathtracer_gaussiansplatting_amd import Renderer, _abi, autograd
from pathtracer_gaussiansplatting_amd import synthetic as Y
from pathtracer_gaussiansplatting_amd.renderer import _gaussians, _ptr, _stream

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

SAME_KERNELS = 1e-5  # relative L2 between two runs of the same kernels: only the atomics' order differs
GUARD, SENTINEL = 1024, -7.25
WIDTHS = {"means": 3, "scales": 3, "rotations": 4, "opacities": 1, "colors": 3, "means2d": 2, "conics": 3}
FRONT_END = {0: "three launches", 1: "fused"}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Guarded:
    """Device arrays with GUARD sentinel floats on either side of each (tests/test_loss_gpu.py::_guarded)."""

    def __init__(self):
        self.bufs = []

    def new(self, shape):
        n = int(np.prod(shape))
        buf = torch.full((GUARD + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
        self.bufs.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def intact(self):
        return all(bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all())
                   for b, n in self.bufs)


def _open():
    return Renderer(0, publish_splat_buffers=True)


def _device_case(c):
    return {"g": {k: _dev(v) for k, v in c["g"].items()}, "dL": _dev(c["dL"]), "dinv": _dev(c["dinv"])}


def _forward(r, c, d, guards, want_fused, label):
    """One published frame with stats into a guarded image; asserts the front end that ran."""
    out = guards.new((c["H"], c["W"], 4))
    st = r.splat_gaussians(d["g"], c["ubo"], c["W"], c["H"], out, bg=c["bg"], want_stats=True)
    torch.cuda.synchronize()
    status = r.splat_status()
    print(f"{c['name']} {label}: st.fused {st.fused} ({FRONT_END[int(st.fused)]}), K {st.num_rendered}, status frames "
          f"{status.frames} spilled_tiles {status.spilled_tiles} touched_runs {status.touched_runs}")
    assert st.fused == want_fused, (label, st.fused)
    assert st.num_rendered == c["frame"]["K"] and (st.tiles_x, st.tiles_y) == ((c["W"] + 15) // 16, (c["H"] + 15) // 16)
    assert status.frames == 0 and status.fused == want_fused
    if want_fused:  # rows sized from the previous frame of the same lists: nothing spills
        assert status.spilled_tiles == 0
    return st, status, out


def _backward(r, c, d, guards, dinv=None):
    """ptgs_splat_gaussians_backward[_depth] of the latest frame into guarded arrays (all seven): numpy float64."""
    n = len(c["g"]["means"])
    t = {k: guards.new((n, w) if w > 1 else (n,)) for k, w in WIDTHS.items()}
    gr = _abi.GaussianGrads()
    for k, v in t.items():
        setattr(gr, k, _ptr(v))
    bg = np.asarray(c["bg"], np.float32)
    args = (r._h, C.byref(_gaussians(d["g"])), C.byref(c["ubo"]), c["W"], c["H"], _abi.fptr(bg), _ptr(d["dL"]))
    if dinv is None:
        rc = r.lib.ptgs_splat_gaussians_backward(*args, C.byref(gr), _stream(None))
    else:
        rc = r.lib.ptgs_splat_gaussians_backward_depth(*args, _ptr(dinv), C.byref(gr), _stream(None))
    assert rc == 0, r._err()
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in t.items()}


def _check_frame(r, c, d, guards, img, label):
    """After a frame: the plain backward, the inverse depth, the backward with both gradients, each against the
    case's reference. Returns (plain, invdepth tensor, full)."""
    keep = ~c["mask"]
    failed = []
    err = R.rel_l2(img.cpu().numpy()[keep], c["r64"]["image"][keep])
    print(f"{c['name']} {label}: image rel L2 {err:.2e}")
    assert err < 1e-4, (label, err)
    plain = _backward(r, c, d, guards)
    colour = Z.part(c, "grads_color")  # (splat_grad_ref's own gradients: tests/test_splat_depth_ref.py)
    for k in R.GRAD_KEYS:
        assert np.isfinite(plain[k]).all(), k
        failed += R.check_bounds(colour, k, plain[k], f"{label}, backward")
    inv = guards.new((c["H"], c["W"]))
    assert r.splat_gaussians_invdepth(c["W"], c["H"], inv) is inv
    torch.cuda.synchronize()
    got = inv.cpu().numpy()
    err = R.rel_l2(got[keep], c["r64"]["invdepth"][keep])
    print(f"{c['name']} {label}: invdepth rel L2 {err:.2e}")
    assert np.isfinite(got).all() and np.linalg.norm(c["r64"]["invdepth"][keep]) > 0 and err < 1e-4, (label, err)
    assert not np.any(got[c["r64"]["empty"]])  # a pixel of an empty tile: exactly 0
    full = _backward(r, c, d, guards, d["dinv"])
    for k in R.GRAD_KEYS:
        assert np.isfinite(full[k]).all(), k
        failed += R.check_bounds(c, k, full[k], f"{label}, backward_depth")
    assert not failed, failed
    culled = c["frame"]["radii"] == 0
    for got_grads in (plain, full):  # culled Gaussians: exactly zero
        for k in R.GRAD_KEYS:
            assert not np.any(got_grads[k][culled]), k
    assert guards.intact(), label
    return plain, inv, full


def _same_lists(c, a, b, what):
    """Two frames of the same lists: the gradients agree within SAME_KERNELS, the inverse depths bit for bit."""
    for which, ga, gb in (("backward", a[0], b[0]), ("backward_depth", a[2], b[2])):
        for k in R.GRAD_KEYS:
            err = R.rel_l2(gb[k], ga[k])
            print(f"{c['name']} {what} {which} {k}: {err:.2e}")
            assert np.linalg.norm(ga[k]) > 0 and err < SAME_KERNELS, (which, k, err)
    assert torch.equal(a[1], b[1]), "the inverse depth of two frames of the same lists must be bit-equal"


@pytest.mark.parametrize("name", ["field", "layers", "wide", "tall"])
def test_backward_after_three_launches_then_fused(native_lib, oracle_lib, name):
    """Frames 0 and 1 of a fresh context: three launches, then the fused front end (its published layout). By the
    code frame 0 sorts lists above 256 inside the blend and frame 1 of field and layers runs the large-tile sort
    ahead of it. wide and tall: the tile grid is 125 and 69 tiles long, and no array is written out of bounds."""
    c = Z.frame_case_reference(name, oracle_lib)
    r = _open()
    try:
        d, guards, got = _device_case(c), _Guarded(), []
        for frame in range(2):
            label = f"frame {frame} ({FRONT_END[frame]})"
            _, _, img = _forward(r, c, d, guards, frame, label)
            got.append(_check_frame(r, c, d, guards, img, label))
        _same_lists(c, got[0], got[1], "frame 1 vs frame 0")
        assert guards.intact()
    finally:
        r.close()


def test_backward_above_the_fused_capacity(native_lib, oracle_lib):
    """crowd: lists of up to ten staged batches, above the fused rows' capacity: both frames run three launches,
    the second with the large-tile sort planned from the first."""
    c = Z.frame_case_reference("crowd", oracle_lib)
    r = _open()
    try:
        d, guards, got = _device_case(c), _Guarded(), []
        for frame in range(2):
            label = f"frame {frame} (three launches)"
            _, status, img = _forward(r, c, d, guards, 0, label)
            assert status.spilled_tiles == 0  # (no fused attempt)
            got.append(_check_frame(r, c, d, guards, img, label))
        _same_lists(c, got[0], got[1], "frame 1 vs frame 0")
    finally:
        r.close()


def test_backward_after_a_rerun_frame(native_lib, oracle_lib):
    """A sparse frame sizes the fused rows at 256 pairs; field then overflows them and, with stats, is re-run
    through three launches: the backward consumes the re-run's layout. The third frame is fused."""
    c = Z.frame_case_reference("field", oracle_lib)
    W, H, ubo = c["W"], c["H"], c["ubo"]
    sparse = Y.gaussians_c2(500, seed=2)
    ref = oracle_lib.splat_gaussians(sparse, ubo, W, H, bg=c["bg"])
    longest = int(np.diff(np.asarray(ref["ranges"]).reshape(-1, 2), axis=1).max())
    assert 0 < longest and longest + longest // 4 <= 256  # rows of 256 pairs from here
    assert int(np.diff(np.asarray(c["frame"]["ranges"]).reshape(-1, 2), axis=1).max()) > 256  # which field outgrows
    r = _open()
    try:
        d, guards = _device_case(c), _Guarded()
        st = r.splat_gaussians({k: _dev(v) for k, v in sparse.items()}, ubo, W, H,
                               torch.zeros((H, W, 4), dtype=torch.float32, device="cuda"), bg=c["bg"], want_stats=True)
        assert st.fused == 0 and st.num_rendered == ref["K"]
        _, status, img = _forward(r, c, d, guards, 0, "re-run (fused, overflowed, three launches)")
        assert status.spilled_tiles > 0  # the superseded fused run's overflowing tiles: the frame was run twice
        redone = _check_frame(r, c, d, guards, img, "re-run")
        _, _, img = _forward(r, c, d, guards, 1, "after the re-run (fused)")
        after = _check_frame(r, c, d, guards, img, "after the re-run (fused)")
        _same_lists(c, redone, after, "fused vs re-run")
    finally:
        r.close()


def test_autograd_on_the_fused_iteration(native_lib, oracle_lib):
    """autograd.splat_depth on layers, two iterations of loss = sum(img dL) + sum(inv dinv) on a fresh context: the
    second differentiates a fused frame, and its leaf gradients are the direct calls' on that frame."""
    c = Z.frame_case_reference("layers", oracle_lib)
    W, H = c["W"], c["H"]
    keys = ("means", "scales", "rotations", "opacities", "colors")
    r = _open()
    try:
        d, guards = _device_case(c), _Guarded()
        for it in range(2):
            leaves = {k: d["g"][k].clone().requires_grad_(True) for k in keys}
            img, inv = autograd.splat_depth(r, *(leaves[k] for k in keys), c["ubo"], W, H, bg=c["bg"])
            torch.cuda.synchronize()
            status = r.splat_status()
            print(f"layers autograd iteration {it}: status fused {status.fused} frames {status.frames}")
            assert status.fused == it and status.frames == 0
            ((img * d["dL"]).sum() + (inv * d["dinv"]).sum()).backward()
            torch.cuda.synchronize()
        direct = _backward(r, c, d, guards, d["dinv"])  # (no forward in between: the same fused frame)
        failed = []
        for k in keys:
            got = leaves[k].grad.cpu().numpy().astype(np.float64)
            err = R.rel_l2(got, direct[k])
            print(f"layers autograd (fused iteration) vs direct {k}: {err:.2e}")
            assert np.linalg.norm(direct[k]) > 0 and err < SAME_KERNELS, (k, err)
            failed += R.check_bounds(c, k, got, "autograd, fused iteration")
        assert not failed, failed
        keep = ~c["mask"]
        assert R.rel_l2(inv.detach().cpu().numpy()[keep], c["r64"]["invdepth"][keep]) < 1e-4
        assert guards.intact()
    finally:
        r.close()
