"""The training loop on the GPU: ptgs_gaussians_checkpoint_init and ptgs_image_mse against their restatements
(tests/train_ref.py), and pathtracer_gaussiansplatting_amd.train.Trainer on the reference scene: the first step against
the float64 reference's gradient, the convergence run beside the reference's trajectory, a run that crosses three
densifications, an opacity reset and two SH-degree steps, and the saved checkpoint rendered back."""
import numpy as np
import pytest
import torch

import adam_ref as A
import train_ref as TR

pytestmark = pytest.mark.gpu

F = np.float32


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------
# ptgs_gaussians_checkpoint_init
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("n", TR.SIZES)
def test_checkpoint_init_bit_exact(renderer, n, deg):
    """Out of place and in place against the numpy float32 restatement, bit for bit; then activate() of the result
    returns to the inputs within the logarithm's error measured on the host (TR.LOG_ABS_ERR) plus expx's own
    (2e-7 max(1, |x|), ptgs.h): relative for the scales, times o (1 - o) for the opacities."""
    scales, o, colors = TR.init_case(n, seed=deg)
    ref = TR.checkpoint_init(scales, o, colors, deg)
    ds, do, dc = _dev(scales), _dev(o), _dev(colors)
    got = renderer.checkpoint_init(ds, do, dc, deg)
    torch.cuda.synchronize()
    assert torch.equal(ds.cpu(), torch.from_numpy(scales)) and torch.equal(do.cpu(), torch.from_numpy(o))
    for name, a, b in zip(("log_scales", "opacity_logits", "sh"), got, ref):
        assert a.shape == b.shape and np.array_equal(_bits(a.cpu().numpy()), _bits(b)), (name, n, deg)
    sh = torch.full((n, (deg + 1) ** 2, 3), 7.0, device="cuda")  # every element of sh is written
    ls, lo, sh2 = renderer.checkpoint_init(ds, do, dc, deg, out=(ds, do, sh))
    assert ls is ds and lo is do and sh2 is sh
    for name, a, b in zip(("log_scales", "opacity_logits", "sh"), (ds, do, sh), ref):
        assert np.array_equal(_bits(a.cpu().numpy()), _bits(b)), ("in place", name, n, deg)
    back_s, back_o = renderer.activate_gaussians(ds, do)
    bs, bo = back_s.cpu().numpy().astype(np.float64), back_o.cpu().numpy().astype(np.float64)
    normal = scales >= np.finfo(F).tiny  # (a subnormal scale comes back from expx's flush as 0)
    rel = np.abs(bs / scales.astype(np.float64) - 1.0)
    bound_s = TR.LOG_ABS_ERR + 2e-7 * np.maximum(1.0, np.abs(ref[0].astype(np.float64)))
    assert (rel <= bound_s)[normal].all(), float((rel - bound_s)[normal].max())
    o64 = o.astype(np.float64)
    bound_o = (TR.LOG_ABS_ERR + 2e-7 * np.maximum(1.0, np.abs(ref[1].astype(np.float64)))) * o64 * (1.0 - o64) + 1e-7
    assert (np.abs(bo - o64) <= bound_o).all(), float((np.abs(bo - o64) - bound_o).max())


def test_checkpoint_init_arguments(renderer):
    from pathtracer_gaussiansplatting_amd import PtgsError
    scales, o, colors = (_dev(a) for a in TR.init_case(8))
    lib, h = renderer.lib, renderer._h
    p = lambda t: t.data_ptr()  # noqa: E731
    ls, lo, sh = torch.empty_like(scales), torch.empty_like(o), torch.empty((8, 1, 3), device="cuda")
    call = lambda *a: lib.ptgs_gaussians_checkpoint_init(h, *a, None)  # noqa: E731
    assert call(p(scales), p(o), p(colors), 8, 0, p(ls), p(lo), p(sh)) == 0
    assert call(None, None, None, 0, 3, None, None, None) == 0            # n == 0 before any pointer
    assert call(p(scales), p(o), p(colors), 8, 4, p(ls), p(lo), p(sh)) == -1
    assert b"sh_degree" in lib.ptgs_last_error(h)
    for k in range(6):
        a = [p(scales), p(o), p(colors), p(ls), p(lo), p(sh)]
        a[k] = None
        assert call(a[0], a[1], a[2], 8, 0, a[3], a[4], a[5]) == -1
    host = np.zeros(24, F)
    assert call(p(scales), p(o), p(colors), 8, 0, p(ls), p(lo), host.ctypes.data) == -1
    assert b"device" in lib.ptgs_last_error(h)
    assert call(p(scales), p(o), p(colors), 8, 0, p(ls), p(lo), p(colors)) == -1   # sh over colors is not in place
    assert call(p(scales), p(o), p(colors), 8, 0, p(scales) + 4, p(lo), p(sh)) == -1
    with pytest.raises(PtgsError):
        renderer.checkpoint_init(scales, o, colors, 5)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------
# ptgs_image_mse
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [3, 4])
@pytest.mark.parametrize("size", TR.MSE_SIZES)
def test_image_mse(renderer, size, channels):
    """Against numpy float64: relative difference <= 1e-8 (float64 sums of fewer than 2^18 non-negative terms: any
    order agrees to 2^18 x 2^-53); exactly 0 on equal images; two runs bit-equal."""
    W, H = size
    image, target = TR.mse_case(W, H, channels)
    ref = TR.image_sq_err(image, target)
    di, dt = _dev(image), _dev(target)
    a = renderer.image_mse(di, dt)
    b = renderer.image_mse(di, dt, out=torch.full((1,), -1.0, dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    got = float(a.cpu()[0])
    print(f"{W}x{H} c{channels}: {got!r} reference {ref!r} rel {abs(got - ref) / ref:.2e}")
    assert ref > 0 and abs(got - ref) <= 1e-8 * ref
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    same = image if channels == 4 else np.ascontiguousarray(image[..., :3])
    z = renderer.image_mse(di, _dev(same))
    assert float(z.cpu()[0]) == 0.0 and not np.signbit(z.cpu().numpy()[0])


def test_image_mse_arguments(renderer):
    from pathtracer_gaussiansplatting_amd import PtgsError
    lib, h = renderer.lib, renderer._h
    img, tgt = torch.zeros((2, 3, 4), device="cuda"), torch.ones((2, 3, 3), device="cuda")
    out = torch.full((1,), 5.0, dtype=torch.float64, device="cuda")
    p = lambda t: t.data_ptr()  # noqa: E731
    assert lib.ptgs_image_mse(h, None, None, 3, 0, 7, None, None) == 0    # W * H == 0 before any pointer
    assert lib.ptgs_image_mse(h, p(img), p(tgt), 3, 3, 0, p(out), None) == 0
    torch.cuda.synchronize()
    assert float(out.cpu()[0]) == 5.0                                     # ... and nothing is written
    assert lib.ptgs_image_mse(h, p(img), p(tgt), 2, 3, 2, p(out), None) == -1
    for a in ((None, p(tgt), p(out)), (p(img), None, p(out)), (p(img), p(tgt), None)):
        assert lib.ptgs_image_mse(h, a[0], a[1], 3, 3, 2, a[2], None) == -1
    host = np.zeros(1, np.float64)
    assert lib.ptgs_image_mse(h, p(img), p(tgt), 3, 3, 2, host.ctypes.data, None) == -1
    assert b"device" in lib.ptgs_last_error(h)
    assert float(renderer.image_mse(img, tgt, out=out).cpu()[0]) == 18.0  # 2 x 3 pixels x 3 channels of (0 - 1)^2
    with pytest.raises(PtgsError):
        renderer.image_mse(img, tgt[:, :, :2].contiguous())


# ---------------------------------------------------------------------------------------------------------
# the trainer on the reference scene
# ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle_lib):
    """The reference scene, its float64 targets and the reference's first step (computed once, left unchanged)."""
    s = TR.first_step_scene(oracle_lib)
    for a in list(s["targets"]) + [s["held_target"]]:
        a.setflags(write=False)
    return s


def _view(eye, target, name=""):
    from pathtracer_gaussiansplatting_amd import View
    u = TR.eye_ubo(eye)
    return View(u, TR.W, TR.H, tuple(float(v) for v in u.camera_pos), _dev(target[..., :3].astype(F)), name)


def _views(scene):
    train = [_view(e, t, f"train_{k}") for k, (e, t) in enumerate(zip(scene["scene"]["eyes"], scene["targets"]))]
    return train, _view(scene["scene"]["held_out"], scene["held_target"], "held_out")


def _start(renderer, scene, sh_degree, extra=None):
    from pathtracer_gaussiansplatting_amd import init_params
    xyz, rgb = scene["scene"]["xyz"], scene["scene"]["rgb"]
    if extra is not None:
        xyz = np.concatenate([xyz, extra.astype(F)])
        rgb = np.concatenate([rgb, np.full((len(extra), 3), 128, np.uint8)])
    return init_params(renderer, _dev(xyz), _dev(rgb), sh_degree)


def _host(params):
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy().copy() for k, v in params.items()}


def test_init_params_is_the_reference_start(renderer, scene, oracle_lib):
    """init_params on the device against the oracle's gaussians_from_points and the restated checkpoint_init."""
    got = _host(_start(renderer, scene, 2))
    ref = TR.start_leaves(scene["scene"], oracle_lib, 2)
    for k in TR.KEYS:
        assert got[k].shape == ref[k].shape and np.array_equal(_bits(got[k]), _bits(ref[k])), k


def test_first_step(renderer, scene):
    """One Trainer.step from the reference start plus four Gaussians behind the first view's camera. The unseen ones
    are bit-unchanged in parameters and moments; for a seen element (p1 - p0) / lr = -sign(g_ref) wherever |g_ref| >=
    1e-3 max|g_ref| of its leaf (Adam's first step is lr sign(g)), within TR.sign_tolerance. The rotations take no
    part: with isotropic scales their reference gradient is exactly 0 (tests/train_ref.py, sign_mask)."""
    from pathtracer_gaussiansplatting_amd import Trainer, schedule
    first = scene["first"]
    k = first["view"]
    assert int(np.random.default_rng(TR.SCENE_SEED).permutation(6)[0]) == k  # the trainer's first view is that one
    eye = np.asarray(scene["scene"]["eyes"][k], np.float64)
    extra = eye[None, :] * 1.5 + np.array([[0.0, 0.0, 0.0], [0.03, 0.0, 0.0], [0.0, 0.03, 0.0], [0.0, 0.0, 0.03]])
    cfg = TR.run_config()
    train, _ = _views(scene)
    t = Trainer(renderer, _start(renderer, scene, 0, extra), train, cfg, extent=1.0)
    n = TR.N_TRUE
    p0 = _host(t.params)
    loss = t.step()
    radii = np.zeros(n + 4, np.int32)
    renderer.copy_d2h(radii, renderer.splat_buffers().radii, radii.nbytes)
    p1 = _host(t.params)
    m1, v1 = _host(t.optimizer.exp_avg), _host(t.optimizer.exp_avg_sq)
    assert t.iteration == 1 and t.optimizer.step_count == 1 and np.isfinite(float(loss))
    assert float(loss) == pytest.approx(first["loss"], rel=1e-4)
    seen = radii > 0
    assert not seen[n:].any() and np.array_equal(seen[:n], first["radii"] > 0) and seen[:n].any()
    for key in TR.KEYS:
        assert np.array_equal(_bits(p1[key][~seen]), _bits(p0[key][~seen])), key
        assert not _bits(m1[key][~seen]).any() and not _bits(v1[key][~seen]).any(), key
    masks, vanishing, left_out = TR.sign_mask(first["grads"], first["radii"])
    assert vanishing == ["rotations"] and left_out <= TR.SIGN_MAX_LEFT_OUT
    lr = {"means": schedule(1, cfg, 1.0, 0).lr_means, "log_scales": cfg.scaling_lr, "opacity_logits": cfg.opacity_lr,
          "sh": cfg.sh_dc_lr}
    for key, rate in lr.items():
        d = (p1[key][:n].astype(np.float64) - p0[key][:n]) / rate
        want = -np.sign(first["grads"][key])
        worst = float(np.abs(d - want)[masks[key]].max())
        tol = TR.sign_tolerance(p0[key][:n], rate)
        print(f"{key}: {int(masks[key].sum())} of {int(seen[:n].sum()) * d[0].size} elements, worst {worst:.2e}, tol {tol:.2e}")
        assert worst <= tol, key


def test_convergence(renderer, scene):
    """Trainer.train(120) with the reference run's constants: the held-out MSE ends at <= 0.5 of its initial value
    (the float64 reference: 0.123, asked 0.25)."""
    from pathtracer_gaussiansplatting_amd import Trainer
    train, held = _views(scene)
    t = Trainer(renderer, _start(renderer, scene, 0), train, TR.run_config(), extent=1.0)
    traj = [(0, t.evaluate([held])[0]["mse"])]
    for _ in range(TR.STEPS // 20):
        loss = t.train(20)
        traj.append((t.iteration, t.evaluate([held])[0]["mse"]))
    assert np.isfinite(float(loss)) and t.count == TR.N_TRUE and t.iteration == TR.STEPS
    m0, r0 = traj[0][1], TR.REF_TRAJECTORY[0][1]
    for (it, m), (rit, rm) in zip(traj, TR.REF_TRAJECTORY):
        assert it == rit
        print(f"iteration {it:3d}: held-out MSE {m:.3e} ({m / m0:.3f})   reference {rm:.3e} ({rm / r0:.3f})")
    assert m0 == pytest.approx(r0, rel=1e-3)  # the same start
    assert traj[-1][1] <= TR.GPU_ASKED * m0
    e = t.evaluate([held])[0]
    assert e["psnr"] == pytest.approx(-10.0 * np.log10(e["mse"])) and 0.0 < e["ssim"] <= 1.0 and e["name"] == "held_out"


def test_events(renderer, scene):
    """100 steps with degree-2 leaves and the small config (densify from 20 every 20 until 80, reset every 50, a
    degree every 30), the rates of the convergence run and the trainer's own extent (the cameras' orbit: with
    extent 1 the size pruning of steps 60 and 80, 0.1 x extent, would remove every Gaussian of this scene)."""
    from pathtracer_gaussiansplatting_amd import Trainer
    train, held = _views(scene)
    t = Trainer(renderer, _start(renderer, scene, 2), train, TR.small_config())  # extent: scene_extent(views)
    assert t.extent == pytest.approx(1.1 * 6.0, rel=0.05)
    mse0 = t.evaluate([held])[0]["mse"]
    counts, losses = [t.count], []
    cap = A.reset_cap(0.01)
    for it in range(1, 101):
        sh_leaf = t.params["sh"]
        losses.append(t.step())
        # the buffers keep one size, and the step count survives every densification
        n = t.count
        counts.append(n)
        for k, p in t.params.items():
            assert p.shape[0] == n and p.requires_grad
            assert t.optimizer.params[k] is p
            assert t.optimizer.exp_avg[k].shape == p.shape and t.optimizer.exp_avg_sq[k].shape == p.shape
        assert t.stats.n == n and t.stats.accum.shape == (n,) and t._m2d.shape == (n, 2)
        assert t.optimizer.step_count == t.iteration == it
        if it in (40, 60, 80):
            assert t.last_counts is not None and n == t.last_counts.total
            assert n == t.last_counts.survivors + t.last_counts.clones + 2 * t.last_counts.split_sources
        else:
            assert n == counts[-2], it
        # the SH gradient of the bands above the active degree is exactly 0: bands >= 1 before step 31, >= 2 before 61
        g = sh_leaf.grad
        assert g is not None and g.shape[1] == 9
        hi1, hi2 = bool(g[:, 1:4].any()), bool(g[:, 4:].any())
        assert hi1 == (it >= 31) and hi2 == (it >= 61), (it, hi1, hi2)
        if it == 50:
            logits = t.params["opacity_logits"].detach()
            assert float(logits.max()) <= float(cap)
            _, op = renderer.activate_gaussians(t.params["log_scales"].detach(), logits)
            assert float(op.max()) <= 0.01 * (1.0 + 4e-7)  # (expx's error at |x| = 4.6, ptgs.h)
            assert not t.optimizer.exp_avg["opacity_logits"].any()
            assert not t.optimizer.exp_avg_sq["opacity_logits"].any()
    assert len(set(counts[:40])) == 1 and counts[0] == TR.N_TRUE
    print("counts after 0 / 40 / 60 / 80 / 100:", [counts[k] for k in (0, 40, 60, 80, 100)])
    assert counts[40] != counts[39] or counts[60] != counts[59] or counts[80] != counts[79]  # something densified
    assert bool(torch.isfinite(torch.stack(losses)).all())
    mse1 = t.evaluate([held])[0]["mse"]
    print(f"held-out MSE {mse0:.3e} -> {mse1:.3e}")
    assert mse1 <= mse0


def test_save_renders_back(renderer, scene, tmp_path):
    """save -> load_gaussian_ply -> splat_gaussians_sh gives the trainer's own render of the view, bit for bit."""
    from pathtracer_gaussiansplatting_amd import Trainer, load_gaussian_ply
    train, held = _views(scene)
    t = Trainer(renderer, _start(renderer, scene, 2), train, TR.small_config())
    t.train(35)  # (degree 1 is active)
    assert t.active_degree() == 1
    mine = t.render(held).clone()
    path = str(tmp_path / "point_cloud.ply")
    t.save(path)
    ck = load_gaussian_ply(path)
    assert ck["sh_degree"] == 2 and len(ck["means"]) == t.count
    for k, v in _host(t.params).items():
        assert np.array_equal(_bits(ck[k]), _bits(v)), k
    d = {k: _dev(ck[k]) for k in TR.KEYS}
    scales, opac = renderer.activate_gaussians(d["log_scales"], d["opacity_logits"])
    g = {"means": d["means"], "scales": scales, "rotations": d["rotations"], "opacities": opac, "sh": d["sh"]}
    out = torch.empty((TR.H, TR.W, 4), dtype=torch.float32, device="cuda")
    renderer.splat_gaussians_sh(g, held.ubo, TR.W, TR.H, out, active_degree=1, bg=TR.BG)
    torch.cuda.synchronize()
    assert float(mine[..., 3].max()) > 0.1  # something is in view
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(mine.cpu().numpy()))
