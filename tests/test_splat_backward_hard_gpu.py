"""The 3DGS backward (ptgs_splat_gaussians_backward, _backward_depth) on the inputs chosen to break the forward:
needle-shaped, giant, near-plane, sub-pixel, tied and opacity-edge Gaussians, long lists, and frames of 1x1 to
130x9 pixels (tests/splat_hard_grad_ref.py: splat_forward_ref's cases, their gradients from splat_depth_ref.evaluate
on a frame built from the forward reference alone; nothing here comes from oracle/).

Every case opens its own Renderer and renders two consecutive published frames with stats; the front end of each is
printed, not prescribed. After each frame the image and the inverse depth are held to splat_forward_ref.compare on
the unmasked pixels (the frame differentiated is the reference's), and three backward calls to
splat_grad_ref.check_bounds, unchanged (max(1e-4, 8 e32) on the whole array, each quarter by gradient norm and the
Gaussians beyond the EWA clamp): the plain backward, the backward with both gradients, and the depth-only backward
(a zero dL_dout). All seven outputs are requested, each inside a sentinel-guarded buffer. Both upstream gradients
are exactly 0 on the reference's mask, so no comparison depends on a decision float32 could take either way."""
import numpy as np
import pytest

import splat_depth_ref as Z
import splat_forward_ref as F
import splat_grad_ref as R
import splat_hard_grad_ref as HG
from test_splat_backward_frames_gpu import FRONT_END, SAME_KERNELS, _Guarded, _backward, _dev, _open

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _frame(r, c, d, guards, label):
    """One published frame with stats and its three backward calls, each checked against the reference. Returns
    {part: gradients} and the worst error / bound seen."""
    W, H, fwd = c["W"], c["H"], c["fwd"]
    img = guards.new((H, W, 4))
    st = r.splat_gaussians(d["g"], c["ubo"], W, H, img, bg=c["bg"], want_stats=True)
    torch.cuda.synchronize()
    status = r.splat_status()
    print(f"{c['name']} {label}: front end {FRONT_END[int(st.fused)]} (st.fused {st.fused}, status.fused {status.fused}), "
          f"K {st.num_rendered}, spilled_tiles {status.spilled_tiles}, touched_runs {status.touched_runs}")
    assert st.num_rendered == c["frame"]["K"], (st.num_rendered, c["frame"]["K"])
    inv = guards.new((H, W))
    assert r.splat_gaussians_invdepth(W, H, inv) is inv
    torch.cuda.synchronize()
    failed = F.compare(fwd, img.cpu().numpy(), label) + F.compare(fwd, inv.cpu().numpy(), label, key="invdepth")
    assert not failed, failed
    zero = dict(d, dL=torch.zeros_like(d["dL"]))
    got = {"grads_color": _backward(r, c, d, guards), "grads": _backward(r, c, d, guards, d["dinv"]),
           "grads_depth": _backward(r, c, zero, guards, d["dinv"])}
    culled = c["frame"]["radii"] == 0
    transparent = ~culled & (c["g"]["opacities"] == 0.0)
    failed = []
    for which, what, keys in HG.checked(c):
        p = Z.part(c, which)
        for k in R.GRAD_KEYS:
            assert np.isfinite(got[which][k]).all(), (label, what, k)
            assert not np.any(got[which][k][culled]), (label, what, k)  # culled: exactly zero
            assert not np.any(got[which][k][transparent]), (label, what, k)  # visible, opacity 0.0: exactly zero
        for k in keys:
            failed += [(label, what) + f for f in R.check_bounds(p, k, got[which][k], f"{label}, {what}")]
    assert not np.any(got["grads_depth"]["colors"])  # the colours do not enter the inverse depth
    assert not failed, failed
    assert guards.intact(), label
    return got


@pytest.mark.parametrize("name", HG.CASES)
def test_backward_on_the_forwards_hard_cases(native_lib, name):
    c = HG.case_reference(name)
    if name == "opacity_edges":
        assert ((c["frame"]["radii"] > 0) & (c["g"]["opacities"] == 0.0)).any()
    if name in ("around", "near"):
        assert (c["frame"]["radii"] == 0).any()
    r = _open()
    try:
        d = {"g": {k: _dev(v) for k, v in c["g"].items()}, "dL": _dev(c["dL"]), "dinv": _dev(c["dinv"])}
        guards = _Guarded()
        got = [_frame(r, c, d, guards, f"frame {frame}") for frame in range(2)]
        for which, what, _ in HG.checked(c):  # the same lists twice: only the atomics' order differs
            for k in R.GRAD_KEYS:
                err = R.rel_l2(got[1][which][k], got[0][which][k])
                print(f"{name} frame 1 vs frame 0, {what} {k}: {err:.2e}")
                assert err < SAME_KERNELS, (what, k, err)
        assert guards.intact()
    finally:
        r.close()
