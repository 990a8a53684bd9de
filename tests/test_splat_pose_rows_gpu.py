"""The camera gradients' second-stage sums past their first pass, and dL/d view on the forward's hard cases.

gs_sum_partial_rows<K, BLOCK> (csrc/splat_partial_sum.h): work-item t adds the rows t + j BLOCK, j < 4, steps by
4 BLOCK, and a halving tree adds the work-items' sums. A row is 256 Gaussians. The pose finish (BLOCK 256) loads
j >= 1 from 65 537 Gaussians on and steps from 262 145 on; the eye finish (BLOCK 1024) from 262 145 and 1 048 577.
tests/test_splat_pose_gpu.py stops at 79 rows. Here:

  ROWS    327 736 Gaussians = 1281 rows, the last one partial; 98 visible ones at the first, last and middle lanes
          of the rows on either side of every j and of the step (tests/splat_pose_grad_ref.py), the rest culled;
          and its prefixes of 65 536 / 65 537 / 262 144 / 262 145 Gaussians, rows = 256 / 257 / 1024 / 1025
  LANES   65 536 Gaussians, one visible per row, at row j lane j
  the eye at 262 144 / 262 145 and 1 048 732 Gaussians against float64, and with one Gaussian per workgroup
          against the float64 sum of what the same call adds to dL_dmeans, to one float32 ulp
  dL/d view on every splat_hard_grad_ref case: a per-Gaussian NaN would poison all twelve sums

tests/test_splat_pose_grad_ref.py asserts on the reference alone that every occupied row (1%), every LANES
Gaussian (10 bounds) and every class of eye rows (5%) carries a share no tolerance here can hide. Tolerances are
the project's: max(1e-4, 8 e32) per block of dL/d view and for dL/d eye, 1e-5 between two runs of the same kernels
on the same Gaussians (only the order of the blend's float atomics and of the sums differs)."""
import numpy as np
import pytest

import sh_grad_ref as S
import splat_grad_ref as R
import splat_hard_grad_ref as HG
import splat_pose_grad_ref as P
from test_splat_backward_frames_gpu import FRONT_END, SAME_KERNELS, _Guarded, _backward, _open
from test_splat_pose_gpu import _check_view, _dev, _forward, _pose_call

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32


def _pose(renderer, c):
    """Forward, then backward_pose with both upstream gradients: ({key: numpy}, view [4, 4])."""
    dg, _ = _forward(renderer, c)
    return _pose_call(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]))


def _check_rows_case(renderer, oracle, c):
    """dL/d view of a rows_reference() case against its reference and against the GPU's own result on the visible
    Gaussians alone (one partial row); the culled Gaussians' gradients exactly 0. Returns the view."""
    got, view = _pose(renderer, c)
    failed = _check_view(c, "grads", view, "backward_pose")
    assert not failed, failed
    culled = c["frame"]["radii"] == 0
    assert int(culled.sum()) == len(culled) - len(c["vis"])
    for k, v in got.items():
        assert np.isfinite(v).all() and not np.any(v[culled]), k
        assert np.any(v[~culled]), k
    k = P.compact_of(c, oracle)
    _, compact = _pose(renderer, k)
    assert not _check_view(k, "grads", compact, "backward_pose, the visible Gaussians alone")
    err = R.rel_l2(view[:3], compact[:3])
    print(f"{c['name']}: dL/d view against the compact case's on the GPU: {err:.2e}")
    assert err < SAME_KERNELS
    return view


# ---- 1. the pose finish past one pass
@pytest.mark.parametrize("n", P.ROWS_PREFIXES + (P.ROWS_N,))
def test_pose_rows(renderer, oracle_lib, n):
    """rows = 256, 257 (the first j = 1 load, for work-item 0 alone), 1024, 1025 (the second step, for work-item 0
    alone: its j >= 1 guards are false), 1281 (the second step with j = 0 for all and j = 1 for work-item 0)."""
    c = P.rows_prefix(n, oracle_lib)
    assert (len(c["g"]["means"]) + 255) // 256 == {65536: 256, 65537: 257, 262144: 1024, 262145: 1025}.get(n, 1281)
    view = _check_rows_case(renderer, oracle_lib, c)
    if n == P.ROWS_N:  # the same frame again: what test_backward_pose_matches_reference asks of two runs
        dg, _ = _forward(renderer, c)
        _, again = _pose_call(renderer, c, dg, _dev(c["dL"]), _dev(c["dinv"]))
        assert R.rel_l2(again, view) < SAME_KERNELS


def test_pose_rows_stale_partials(renderer, oracle_lib):
    """On one renderer: ROWS moved up by three rows (rows 3, 258, ... hold the visible Gaussians), then ROWS: the
    workgroups of rows 3, 258, ... are now all culled and wrote a non-zero row a call earlier. Then the 65 537 prefix:
    rows 257 .. 1280 of the scratch are ROWS' and must not be read."""
    shifted = tuple(i + 3 * 256 for i in P.ROWS if i + 3 * 256 < P.ROWS_N)
    assert len(shifted) == 88 and not set(i // 256 for i in shifted) & set(P.ROWS_AT)
    s = P.rows_inputs(shifted, P.ROWS_N, oracle_lib)
    got, view = _pose(renderer, s)
    assert np.isfinite(view).all() and np.any(view[:3]) and all(np.isfinite(v).all() for v in got.values())
    rows = np.flatnonzero(np.abs(got["means"]).sum(1) > 0) // 256
    assert set(rows) == set(i // 256 for i in shifted)  # those rows did carry a gradient
    for n in (P.ROWS_N, 65537):
        c = P.rows_prefix(n, oracle_lib)
        _, view = _pose(renderer, c)
        failed = _check_view(c, "grads", view, "backward_pose after a call with other rows")
        assert not failed, failed


def test_pose_lanes(renderer, oracle_lib):
    """One visible Gaussian per row, at lane j of row j: every lane of every wave of the first stage carries its
    workgroup's sum alone, and every work-item of the finish holds one row."""
    _check_rows_case(renderer, oracle_lib, P.lanes_reference(oracle_lib))


# ---- 2. the eye finish past one pass
@pytest.mark.parametrize("deg,n", sorted(P.EYE_DENSE))
def test_eye_rows_dense(renderer, deg, n):
    """dL/d eye against float64 at rows = 1024, 1025 (the first j = 1 load) and 4097 (the second step), the short
    classes of rows scaled up to at least 5% of the result (splat_pose_grad_ref.EYE_DENSE)."""
    means, sh, dcol = P.eye_dense_inputs(deg, n)
    dm, dsh_in, dc = _dev(means), _dev(sh), _dev(dcol)
    _, _, eye = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dc, active_degree=deg, want_eye=True)
    _, _, eye2 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dc, active_degree=deg, want_means=False, want_eye=True)
    torch.cuda.synchronize()
    assert torch.equal(eye, eye2)  # no atomics: the same bits, with and without dL_dmeans
    ref = P.eye_grad(means, sh, S.CAM, deg, dcol, torch.float64)
    e32 = R.rel_l2(P.eye_grad(means, sh, S.CAM, deg, dcol, torch.float32), ref)
    err = R.rel_l2(eye.cpu().numpy().astype(np.float64), ref)
    print(f"degree {deg}, n {n}: dL/d eye rel L2 {err:.2e}  e32 {e32:.2e}  bound {max(1e-4, 8 * e32):.1e}")
    assert np.linalg.norm(ref) > 0 and err <= max(1e-4, 8.0 * e32)


@pytest.mark.parametrize("deg", [1, 3])
def test_eye_one_gaussian_per_workgroup(renderer, deg):
    """dcol is non-zero at index r * 256 + r % 256 of every row r alone. sh_backward_one adds dm = (v - dir (dir . v))
    / len to dL_dmeans (zeros before the call: 0 + dm is dm) and hands the same float to the eye sum (read in
    csrc/splat_sh_math.h: one `dm`, stored to both), and a Gaussian with a zero dcol has dres = 0, v = 0, dm = 0. So
    every partial row is one Gaussian's dm plus exact zeros, and the finish adds those 4097 float32 values in float64:
    only the order of a float64 sum of 4097 terms can move the rounded float32, by at most one ulp of it."""
    n = P.EYE_N_STEP
    means, sh, _ = S.inputs(deg, n, False)
    dcol, at = P.eye_sparse_dcol(deg, n)
    dm, dsh_in, dc = _dev(means), _dev(sh), _dev(dcol)
    zeros = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
    _, dmeans, eye = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dc, active_degree=deg, dL_dmeans=zeros,
                                                 want_eye=True)
    _, _, eye2 = renderer.sh_colors_backward(dm, dsh_in, S.CAM, dc, active_degree=deg, want_means=False, want_eye=True)
    torch.cuda.synchronize()
    assert dmeans is zeros and torch.equal(eye, eye2)
    live = torch.zeros(n, dtype=torch.bool, device="cuda")
    live[_dev(at)] = True
    assert not bool(dmeans[~live].any())  # a zero dcol adds an exact zero
    # every row's Gaussian does count, but for those whose colour the forward clamps on all three channels (dres = 0;
    # the numpy restatement of the contract says which: none at degree 1, 43 at degree 3, the last row's not among them)
    dead = S.np_dsh(means[at], sh[at], S.CAM, deg, dcol[at])[1].all(1)
    assert len(at) == 4097 and not dead[4096] and max(dead[k:k + 1024].mean() for k in range(0, 4096, 1024)) < 0.02
    assert np.array_equal((dmeans[live] != 0).any(1).cpu().numpy(), ~dead)
    want = -(dmeans.double().sum(0).cpu().numpy().astype(F))
    got = eye.cpu().numpy()
    ulp = np.spacing(np.abs(want))
    print(f"degree {deg}: dL/d eye {got} against the float64 sum of dL_dmeans {want}: {np.abs(got - want) / ulp} ulp")
    assert np.all(want != 0) and np.all(np.abs(got.astype(np.float64) - want.astype(np.float64)) <= ulp)


# ---- 3. dL/d view on the forward's hard cases
@pytest.mark.parametrize("name", HG.CASES)
def test_backward_pose_on_the_forwards_hard_cases(native_lib, name):
    """Needles, giants, near-plane, sub-pixel, tied and opacity-edge Gaussians, long lists, 1x1 to 130x9 frames: the
    three pose calls (both gradients, colour only, depth only) give sixteen finite floats, row 3 exactly 0, each block
    within max(1e-4, 8 e32) of its part of the reference (8 e32 capped at BOUND_CAP), and the seven per-Gaussian
    arrays of the same call are the non-pose backward's of the same frame."""
    c = P.hard_case_reference(name)
    W, H = c["W"], c["H"]
    r = _open()
    try:
        d = {"g": {k: _dev(v) for k, v in c["g"].items()}, "dL": _dev(c["dL"]), "dinv": _dev(c["dinv"])}
        img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        st = r.splat_gaussians(d["g"], c["ubo"], W, H, img, bg=c["bg"], want_stats=True)
        torch.cuda.synchronize()
        print(f"{name}: front end {FRONT_END[int(st.fused)]}, K {st.num_rendered}")
        assert st.num_rendered == c["frame"]["K"]
        guards = _Guarded()
        zero = dict(d, dL=torch.zeros_like(d["dL"]))
        calls = (("grads", d, d["dinv"]), ("grads_color", d, None), ("grads_depth", zero, d["dinv"]))
        failed = []
        for which, dd, dinv in calls:
            plain = _backward(r, c, dd, guards, dinv)
            got, view = _pose_call(r, c, d["g"], dd["dL"], dinv)
            assert np.isfinite(view).all(), (which, view)
            assert np.array_equal(view[3], np.zeros(4, F)) and not np.signbit(view[3]).any()  # row 3: exactly 0
            ref = c["pose"][which]
            failed += P.check_blocks(ref["r64"], ref["r32"], view[:3], f"{name} GPU backward_pose ({which})",
                                     cap=HG.BOUND_CAP)
            for k in R.GRAD_KEYS:
                assert np.isfinite(got[k]).all(), (which, k)
                err = R.rel_l2(got[k], plain[k])
                print(f"{name} {which} {k}: backward_pose against the backward of the same frame {err:.2e}")
                assert err < SAME_KERNELS, (which, k, err)
        assert not failed, failed
        assert guards.intact()
    finally:
        r.close()
