"""ptgs_densify_accumulate, ptgs_gaussians_densify_plan and ptgs_gaussians_densify_apply on the GPU against the
sequential numpy float32 reference of tests/densify_ref.py: counts, source map and every output array bit for bit
(the contract has no transcendental and no atomics, so there is no tolerance anywhere in this file), and
densify_and_prune inside an Adam loop.

Sizes. The plan's workgroup covers BLOCK = 2048 Gaussians (8 rounds of 256) and its second level walks the block
sums STEP = 256 at a time with a carry. N = 3 * BLOCK + 1 = 6145 has four blocks, the last with one Gaussian (block
offsets from the second level, a ragged tail); N = STEP * BLOCK + 1 = 524289 has 257 blocks, one more than the second
level takes in one step, so its carry is used."""
import ctypes as C

import numpy as np
import pytest

import densify_ref as D
from pathtracer_gaussiansplatting_amd import DensifyStats, PtgsError, Renderer, _abi, densify_and_prune

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

F = np.float32
BLOCK, STEP = 2048, 256
SENTINEL = 7.0
GUARD = 1024
COUNT_NAMES = ("survivors", "clones", "split_sources", "pruned_originals", "pruned_children", "total")
STAT_KEYS = ("scales", "opacities", "accum", "denom", "max_radii")


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _counts(c):
    return {k: int(getattr(c, k)) for k in COUNT_NAMES}


def _plan(renderer, case, d=None):
    d = d or {k: _dev(case[k]) for k in STAT_KEYS}
    th = {k: float(v) for k, v in case["thresholds"].items()}
    return renderer.densify_plan(d["scales"], d["opacities"], d["accum"], d["denom"], d["max_radii"], **th)


def _placed(a, offset):
    """A device copy of `a` whose base is `offset` floats past a 16-byte boundary."""
    flat = torch.from_numpy(np.ascontiguousarray(a).reshape(-1))
    buf = torch.empty(flat.numel() + offset, dtype=torch.float32, device="cuda")
    v = buf[offset:]
    v.copy_(flat)
    assert flat.numel() == 0 or v.data_ptr() % 16 == 4 * offset
    return v


def _guarded(numel, offset, dtype=torch.float32):
    buf = torch.full((offset + numel + GUARD,), SENTINEL, dtype=dtype, device="cuda")
    return buf, buf[offset:offset + numel]


def _apply_raw(renderer, case, n_out, offset=0, n=None, rows=None, source=True):
    """The C call on raw pointers: inputs and outputs `offset` floats past 16-byte alignment, outputs in
    sentinel-filled buffers with guards. Returns (rc, outputs as numpy or None)."""
    n = case["n"] if n is None else n
    src = {k: _placed(case[k], offset) for k in ("means", "log_scales", "rotations", "scales", "noise")}
    rows = case["rows"] if rows is None else rows
    widths = [a.reshape(case["n"], -1).shape[1] for a, _ in rows]
    row_src = [_placed(a, offset) for a, _ in rows]
    outs = [_guarded(3 * n_out, offset), _guarded(3 * n_out, offset)] + [_guarded(w * n_out, offset) for w in widths]
    smap = _guarded(n_out, 0, torch.int32) if source else (None, None)
    arr = (_abi.DensifyRows * max(1, len(rows)))()
    for k, (a, z) in enumerate(rows):
        arr[k].src, arr[k].dst, arr[k].width, arr[k].zero_new = row_src[k].data_ptr(), outs[2 + k][1].data_ptr(), widths[k], int(z)
    rc = renderer.lib.ptgs_gaussians_densify_apply(
        renderer._h, n, n_out, src["means"].data_ptr(), src["log_scales"].data_ptr(), src["rotations"].data_ptr(),
        src["scales"].data_ptr(), src["noise"].data_ptr(), outs[0][1].data_ptr(), outs[1][1].data_ptr(), arr, len(rows),
        smap[1].data_ptr() if source else None, None)
    torch.cuda.synchronize()
    if rc != 0:
        for buf, _ in outs:  # a rejected call enqueued nothing
            assert bool((buf == SENTINEL).all())
        return rc, None
    host = []
    for buf, view in outs + ([smap] if source else []):
        b = buf.cpu().numpy()
        lo = offset if buf.dtype == torch.float32 else 0
        assert np.all(b[:lo] == SENTINEL) and np.all(b[lo + view.numel():] == SENTINEL)  # nothing outside is touched
        host.append(b[lo:lo + view.numel()])
    got = {"means": host[0].reshape(n_out, 3), "log_scales": host[1].reshape(n_out, 3),
           "rows": [h.reshape(n_out, w) for h, w in zip(host[2:2 + len(rows)], widths)],
           "source": host[-1].view(np.uint32) if source else None}
    # the inputs are untouched
    for k, v in src.items():
        assert np.array_equal(v.cpu().numpy().view(np.uint32), np.ascontiguousarray(case[k]).reshape(-1).view(np.uint32))
    return rc, got


def _same(got, ref):
    assert np.array_equal(got["source"], ref["source"])
    for k in ("means", "log_scales"):  # (as integers: a NaN would not hide)
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert len(got["rows"]) == len(ref["rows"])
    for k, (a, b) in enumerate(zip(got["rows"], ref["rows"])):
        assert np.array_equal(a.view(np.uint32), np.ascontiguousarray(b).reshape(a.shape).view(np.uint32)), k


# ---------------------------------------------------------------------------------------------------------
# the statistic
# ---------------------------------------------------------------------------------------------------------
def test_accumulate_three_views(renderer):
    n = 1000
    rng = np.random.default_rng(3)
    stats = DensifyStats(n)
    ref = tuple(np.zeros(n, F) for _ in range(3))
    for W, H in ((60, 44), (800, 600), (1, 7)):
        radii = rng.integers(1, 50, n).astype(np.int32)
        radii[rng.random(n) < 1 / 3] = 0
        g2d = rng.normal(0.0, 1e-3, (n, 2)).astype(F)
        stats.update(renderer, _dev(g2d), W, H, radii=_dev(radii))
        ref = D.accumulate(g2d, radii, W, H, *ref)
    got = (stats.accum, stats.denom, stats.max_radii)
    for a, b in zip(got, ref):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), b.view(np.uint32))
    assert (ref[1] == 0).any() and (ref[1] == 3).any() and ref[0].max() > 0
    stats.reset()
    assert not any(bool(t.any()) for t in got)


def test_accumulate_through_splat_sh(renderer):
    """The statistic of one real view: dL/d(2D mean) from autograd.splat_sh(..., means2d_grad=) of the 60 x 44
    `chunks` case and the radii the frame itself published."""
    import test_sh_backward_gpu as B
    p, g, ubo, W, H, bg, dL = B._checkpoint_case("chunks")
    assert (W, H) == (60, 44)
    n = len(p["means"])
    c = {"ubo": ubo, "W": W, "H": H, "bg": bg}
    lv = B._leaves(p)
    m2d = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    img = B._splat_sh(renderer, lv, c, means2d_grad=m2d)
    (img * _dev(dL)).sum().backward()
    stats = DensifyStats(n)
    stats.update(renderer, m2d, W, H)  # (radii: the published frame's)
    torch.cuda.synchronize()
    b = renderer.splat_buffers()
    assert b.num_gaussians == n
    radii = np.zeros(n, np.int32)
    renderer.copy_d2h(radii, b.radii, 4 * n)
    z = np.zeros(n, F)
    ref = D.accumulate(m2d.cpu().numpy(), radii, W, H, z, z, z)
    for a, r in zip((stats.accum, stats.denom, stats.max_radii), ref):
        assert np.array_equal(a.cpu().numpy().view(np.uint32), r.view(np.uint32))
    assert (radii > 0).any() and ref[0].max() > 0 and np.array_equal(ref[1] > 0, radii > 0)
    with pytest.raises(PtgsError):  # a statistic of another size than the frame
        DensifyStats(n + 1).update(renderer, torch.zeros((n + 1, 2), device="cuda"), W, H)


# ---------------------------------------------------------------------------------------------------------
# plan and apply
# ---------------------------------------------------------------------------------------------------------
NARROW = dict(widths=(4,), zero_widths=(3,))
CASES = {"n1-survive": lambda: D.single("survive"), "n1-clone": lambda: D.single("clone"),
         "n1-split": lambda: D.single("split"), "n1-pruned": lambda: D.single("pruned"),
         "n257": lambda: D.make_case(257), "main-n1000": lambda: D.make_case(1000),
         "three-blocks-and-one": lambda: D.make_case(3 * BLOCK + 1, **NARROW),
         "second-level-carry": lambda: D.make_case(STEP * BLOCK + 1, **NARROW),
         "all-pruned": lambda: D.make_case(300, mix="pruned"), "all-split": lambda: D.make_case(300, mix="split"),
         "nothing-hot": lambda: D.make_case(300, thresholds=D.NOTHING_HOT, special=False)}
_REF = {}


def _case(name):
    if name not in _REF:
        c = CASES[name]()
        _REF[name] = (c, D.densify_and_prune(c))
    return _REF[name]


@pytest.mark.parametrize("name", list(CASES))
def test_plan_and_apply_match_the_sequence(renderer, name):
    c, ref = _case(name)
    n = c["n"]
    if name == "main-n1000":  # the case's own precondition, before any output is looked at
        assert D.fates_present(ref["counts"], n), ref["counts"]
    if name in ("three-blocks-and-one", "second-level-carry"):
        assert n == {"three-blocks-and-one": 6145, "second-level-carry": 524289}[name]
        assert D.fates_present(ref["counts"], n)
    counts = _counts(_plan(renderer, c))
    print(name, counts)
    assert counts == ref["counts"]
    rc, got = _apply_raw(renderer, c, counts["total"])
    assert rc == 0
    _same(got, ref)
    if name == "all-pruned":
        assert counts["total"] == 0
    if name == "all-split":
        assert counts["total"] == 2 * n and counts["split_sources"] == n
    if name == "nothing-hot":  # the outputs are the inputs, moments included
        assert counts["total"] == n and np.array_equal(got["means"], c["means"])
        assert np.array_equal(got["log_scales"], c["log_scales"])
        for a, (b, _) in zip(got["rows"], c["rows"]):
            assert np.array_equal(a, b)
    if name.startswith("n1-"):
        want = {"survive": (1, 0, 0, 0, 0, 1), "clone": (1, 1, 0, 0, 0, 2), "split": (0, 0, 1, 0, 0, 2),
                "pruned": (0, 0, 0, 1, 0, 0)}[name[3:]]
        assert tuple(counts.values()) == want


@pytest.mark.parametrize("offset", [0, 1], ids=["aligned", "misaligned"])
def test_row_widths(renderer, offset):
    """SH rows of degree 0..3 (3, 12, 27, 48 floats), widths 1 and 4, a copied and a zero-for-new row of each;
    misaligned: every base 4 bytes past a 16-byte boundary, where a 16-byte access would fault or tear."""
    w = (3, 12, 27, 48, 1, 4)
    c = D.make_case(129, widths=w, zero_widths=w)
    ref = D.densify_and_prune(c)
    assert D.fates_present(ref["counts"], 129)
    counts = _counts(_plan(renderer, c))
    assert counts == ref["counts"]
    rc, got = _apply_raw(renderer, c, counts["total"], offset=offset)
    assert rc == 0
    _same(got, ref)
    new = (ref["source"] >> np.uint32(D.KIND_SHIFT)) != 0
    for a in got["rows"][len(w):]:
        assert not np.any(a[new]) and np.any(a[~new])


def test_python_apply_and_two_runs_are_bit_equal(renderer):
    c, ref = _case("main-n1000")
    d = {k: _dev(c[k]) for k in STAT_KEYS + ("means", "log_scales", "rotations", "noise")}
    rows = [(_dev(a), z) for a, z in c["rows"]]
    runs = []
    for _ in range(2):
        counts = _plan(renderer, c, d)
        assert _counts(counts) == ref["counts"]
        mo, lo, outs, src = renderer.densify_apply(counts.total, d["means"], d["log_scales"], d["rotations"],
                                                   d["scales"], d["noise"], rows, want_source=True)
        runs.append([mo, lo, src] + outs)
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    mo, lo, src = runs[0][:3]
    got = {"means": mo.cpu().numpy(), "log_scales": lo.cpu().numpy(), "source": src.cpu().numpy().view(np.uint32),
           "rows": [t.cpu().numpy() for t in runs[0][3:]]}
    _same(got, ref)
    assert got["rows"][2].shape == (counts.total, 48)


def test_argument_table(renderer):
    L, E = renderer.lib, _abi.PTGS_EINVAL
    c, ref = _case("n257")
    n, total = 257, ref["counts"]["total"]
    err = lambda r=renderer: r.lib.ptgs_last_error(r._h)  # noqa: E731
    # apply without a plan: a context of its own
    fresh = Renderer(0)
    try:
        rc, _ = _apply_raw(fresh, c, total)
        assert rc == E and b"no plan" in err(fresh)
    finally:
        fresh.close()
    assert _counts(_plan(renderer, c)) == ref["counts"]
    # a stale n / n_out
    small = {**c, "n": 256, **{k: c[k][:256] for k in ("means", "log_scales", "rotations", "scales")},
             "noise": np.ascontiguousarray(c["noise"][:, :256]), "rows": [(a[:256], z) for a, z in c["rows"]]}
    rc, _ = _apply_raw(renderer, small, total)
    assert rc == E and b"latest plan" in err()
    rc, _ = _apply_raw(renderer, c, total + 1)
    assert rc == E and b"latest plan" in err()
    # n_rows = 17, a width of 0
    a17 = np.zeros((n, 1), F)
    rc, _ = _apply_raw(renderer, c, total, rows=[(a17, False)] * 17)
    assert rc == E and b"n_rows 17" in err()
    d = {k: _dev(c[k]) for k in ("means", "log_scales", "rotations", "scales", "noise")}
    mo, lo = (torch.full((total, 3), SENTINEL, device="cuda") for _ in range(2))
    row_in, row_out = torch.zeros((n, 4), device="cuda"), torch.full((total, 4), SENTINEL, device="cuda")

    def call(means=d["means"], means_out=mo, src=row_in, dst=row_out, width=4, n_rows=1, ctx=renderer._h):
        arr = (_abi.DensifyRows * 1)()
        p = lambda t: None if t is None else (t if isinstance(t, int) else t.data_ptr())  # noqa: E731
        arr[0].src, arr[0].dst, arr[0].width, arr[0].zero_new = p(src), p(dst), width, 0
        return L.ptgs_gaussians_densify_apply(ctx, n, total, p(means), d["log_scales"].data_ptr(),
                                              d["rotations"].data_ptr(), d["scales"].data_ptr(), d["noise"].data_ptr(),
                                              p(means_out), lo.data_ptr(), arr, n_rows, None, None)

    assert call(width=0) == E and b"width 0" in err()
    # an aliased dst: a row onto its own source, the means onto themselves, two outputs onto each other
    assert call(dst=row_in) == E and b"aliases" in err()
    assert call(means_out=d["means"]) == E and b"aliases" in err()
    assert call(dst=mo) == E and b"aliases" in err()
    # null context / required pointers, an output that is not a device pointer
    assert call(ctx=None) == E
    assert call(means=None) == E and b"null" in err()
    assert call(means_out=None) == E and b"null" in err()
    assert call(src=None) == E and b"null" in err()
    host = np.zeros(total * 3, F)
    assert call(means_out=host.ctypes.data) == E and b"not a device pointer" in err()
    assert call(n_rows=0) == 0  # (rows are optional)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(mo.cpu().numpy().view(np.uint32), ref["means"].view(np.uint32))
    # the plan's own arguments
    s = {k: _dev(c[k]) for k in STAT_KEYS}
    th, out = _abi.DensifyParams(0.0002, 0.05, 0.005, 0.0, 0.0), _abi.DensifyCounts()
    ptrs = [s[k].data_ptr() for k in STAT_KEYS]
    assert L.ptgs_gaussians_densify_plan(None, *ptrs, n, C.byref(th), C.byref(out), None) == E
    assert L.ptgs_gaussians_densify_plan(renderer._h, *ptrs, n, None, C.byref(out), None) == E and b"null" in err()
    assert L.ptgs_gaussians_densify_plan(renderer._h, *ptrs, n, C.byref(th), None, None) == E
    for miss in range(5):
        q = list(ptrs)
        q[miss] = None
        assert L.ptgs_gaussians_densify_plan(renderer._h, *q, n, C.byref(th), C.byref(out), None) == E, miss
    assert L.ptgs_gaussians_densify_plan(renderer._h, *ptrs, (1 << 30) + 1, C.byref(th), C.byref(out), None) == E
    assert b"2^30" in err()
    # n == 0: PTGS_OK before the pointers are looked at, all-zero counts, and a plan of 0 -> 0
    out.total = 9
    assert L.ptgs_gaussians_densify_plan(renderer._h, None, None, None, None, None, 0, C.byref(th), C.byref(out), None) == 0
    assert _counts(out) == dict.fromkeys(COUNT_NAMES, 0)
    assert L.ptgs_gaussians_densify_apply(renderer._h, 0, 0, None, None, None, None, None, None, None, None, 0, None,
                                          None) == 0
    assert call() == E and b"latest plan" in err()  # (the plan of 257 is gone)
    assert L.ptgs_densify_accumulate(renderer._h, None, None, 0, 4, 4, None, None, None, None) == 0
    g2d, radii = torch.zeros((n, 2), device="cuda"), torch.ones(n, dtype=torch.int32, device="cuda")
    acc = [torch.full((n,), SENTINEL, device="cuda") for _ in range(3)]
    ap = [t.data_ptr() for t in acc]
    assert L.ptgs_densify_accumulate(None, g2d.data_ptr(), radii.data_ptr(), n, 4, 4, *ap, None) == E
    assert L.ptgs_densify_accumulate(renderer._h, None, radii.data_ptr(), n, 4, 4, *ap, None) == E and b"null" in err()
    assert L.ptgs_densify_accumulate(renderer._h, g2d.data_ptr(), radii.data_ptr(), n, 4, 4, ap[0], None, ap[2], None) == E
    assert L.ptgs_densify_accumulate(renderer._h, g2d.data_ptr(), radii.data_ptr(), n, 4, 4, ap[0], ap[1],
                                     host.ctypes.data, None) == E
    assert b"device pointers" in err()
    torch.cuda.synchronize()
    assert all(bool((t == SENTINEL).all()) for t in acc)  # every rejected call enqueued nothing
    # n_out == 0 (everything pruned): PTGS_OK, nothing is written
    cp, rp = _case("all-pruned")
    assert _counts(_plan(renderer, cp))["total"] == 0
    rc, got = _apply_raw(renderer, cp, 0)
    assert rc == 0 and got["means"].shape == (0, 3)
    # the Python layer
    with pytest.raises(PtgsError):
        renderer.densify_apply(0, _dev(cp["means"]), _dev(cp["log_scales"]), _dev(cp["rotations"]), _dev(cp["scales"]),
                               _dev(cp["noise"]), rows=[(torch.zeros((300, 1), device="cuda"), False)] * 17)
    with pytest.raises(PtgsError) as e:
        renderer.densify_apply(5, _dev(cp["means"]), _dev(cp["log_scales"]), _dev(cp["rotations"]), _dev(cp["scales"]),
                               _dev(cp["noise"]))
    assert e.value.code == E


# ---------------------------------------------------------------------------------------------------------
# end to end: Adam, densify_and_prune, Adam
# ---------------------------------------------------------------------------------------------------------
# the reference trainer's learning rates (position 0.00016 x extent, scaling 0.005, rotation 0.001, opacity 0.05) and,
# for the coefficients, the rate of the existing Adam test of test_sh_backward_gpu.py
LEARNING_RATES = {"means": 1e-3, "log_scales": 5e-3, "rotations": 1e-3, "opacity_logits": 0.05, "sh": 0.02}
PERCENT_DENSE = 0.01  # the trainer's: clone at or below percent_dense x extent, split above


def test_adam_densify_adam(renderer):
    """15 Adam steps over all five leaves of the `batches` checkpoint with the statistic updated each step,
    densify_and_prune with the gradient threshold at the accumulated statistic's median (half of the seen
    Gaussians are hot) and the trainer's percent_dense x extent between clone and split, 15 more steps."""
    _adam_densify_adam(renderer, LEARNING_RATES, PERCENT_DENSE)


def _adam_densify_adam(renderer, lr, percent_dense, check=True):
    import test_sh_backward_gpu as B
    p, g, ubo, W, H, bg, _ = B._checkpoint_case("batches")
    c = {"ubo": ubo, "W": W, "H": H, "bg": bg}
    d = {k: _dev(p[k]) for k in B.PARAM_KEYS}
    with torch.no_grad():
        target = B._splat_sh(renderer, d, c).clone()
    torch.manual_seed(3)
    lv = dict(d)
    lv["sh"] = d["sh"] + 0.3 * torch.randn_like(d["sh"])
    lv["opacity_logits"] = d["opacity_logits"] * 0.6 - 0.3
    lv = {k: v.clone().requires_grad_(True) for k, v in lv.items()}
    opt = torch.optim.Adam([{"params": [lv[k]], "lr": lr[k]} for k in B.PARAM_KEYS])
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
            opt.step()
            stats.update(renderer, m2d, W, H)
            losses.append(float(loss.detach()))

    steps(lv, stats, 15)
    seen = stats.denom > 0
    assert bool(seen.any()) and float(stats.denom.max()) == 15.0
    avg = (stats.accum[seen] / stats.denom[seen])
    thr = float(avg.median())
    sc, _ = renderer.activate_gaussians(lv["log_scales"].detach(), lv["opacity_logits"].detach())
    extent = float((d["means"] - d["means"].mean(dim=0)).norm(dim=1).max())  # (stands in for the cameras' extent)
    split = percent_dense * extent
    before = {k: {m: opt.state[lv[k]][m].clone() for m in ("exp_avg", "exp_avg_sq")} for k in B.PARAM_KEYS}
    old = {k: v.detach().clone() for k, v in lv.items()}
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    new, counts, stats2 = densify_and_prune(renderer, lv, stats, grad_threshold=thr, scale_split=split,
                                            min_opacity=0.005, optimizer=opt, generator=gen)
    nn = counts.total
    print("densify:", _counts(counts), f"threshold {thr:.3e} split {split:.3e}")
    assert nn != n and counts.clones + counts.split_sources > 0
    assert nn == counts.survivors + counts.clones + 2 * counts.split_sources
    assert stats2.n == nn and not bool(stats2.accum.any()) and stats2.accum.shape == (nn,)
    # the map of the plan the call left (applied once more, to the old arrays)
    mo, _, _, src = renderer.densify_apply(nn, old["means"], old["log_scales"], old["rotations"], sc,
                                           torch.zeros((2, n, 3), device="cuda"), want_source=True)
    src = src.cpu().numpy().view(np.uint32)
    kind, idx = src >> np.uint32(D.KIND_SHIFT), (src & np.uint32((1 << D.KIND_SHIFT) - 1)).astype(np.int64)
    A = counts.survivors
    assert np.all(kind[:A] == 0) and np.all(kind[A:] != 0)
    keep = torch.from_numpy(idx[:A]).cuda()
    not_child = torch.from_numpy(np.flatnonzero(kind < 2)).cuda()
    for gi, k in enumerate(B.PARAM_KEYS):
        t = new[k]
        assert t.is_leaf and t.requires_grad and t.shape[0] == nn and t.shape[1:] == old[k].shape[1:]
        assert opt.param_groups[gi]["params"][0] is t and lv[k] not in opt.state
        st = opt.state[t]
        assert float(st["step"]) == 15.0
        for m in ("exp_avg", "exp_avg_sq"):
            assert st[m].shape == t.shape
            assert torch.equal(st[m][:A], before[k][m][keep])  # survivors keep their moments, bit for bit
            assert not bool(st[m][A:].any())  # new rows start from zero
        if k not in ("means", "log_scales"):
            assert torch.equal(t.detach(), old[k][torch.from_numpy(idx).cuda()])
    assert torch.equal(new["means"].detach()[not_child], old["means"][torch.from_numpy(idx).cuda()[not_child]])
    assert torch.equal(new["means"].detach()[not_child], mo[not_child])
    # the new set renders, and training goes on
    with torch.no_grad():
        B._splat_sh(renderer, new, c)
    assert renderer.splat_buffers().num_gaussians == nn
    steps(new, stats2, 15)
    print(f"adam / densify / adam: loss {losses[0]:.4f} -> {losses[14]:.4f} | {losses[15]:.4f} -> {losses[-1]:.4f}")
    if not check:
        return losses
    assert len(losses) == 30 and np.isfinite(losses).all() and losses[-1] < losses[0]
    assert float(opt.state[new["sh"]]["step"]) == 30.0 and float(stats2.denom.max()) == 15.0
