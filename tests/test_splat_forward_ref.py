"""The tile-free float64 reference of the 3DGS forward (tests/splat_forward_ref.py) on the CPU: every case has the
structural property it exists for (asserted from the reference alone), keeps its borderline pixels under MASK_CAP
and its per-pixel bound under 1e-3; the CPU oracle agrees with the reference on visibility, radii, pair counts and
the image; the oracle's tight binning keeps every pair the reference says matters; each mutation of the reference
moves an unmasked pixel by more than 4x the case's per-pixel tolerance (the comparison has teeth); the
reference's projection agrees with splat_grad_ref._project. The GPU comparison is tests/test_splat_forward_gpu.py."""
import numpy as np
import pytest

import splat_forward_ref as F
import splat_grad_ref as G

torch = pytest.importorskip("torch")

NAMES = list(F.CASES)


def _args(c):
    return c["g"], c["ubo"], c["W"], c["H"], c["bg"]


def _frame(c, oracle, **kw):
    key = "frame_tight" if kw.get("tight") else "frame"
    if key not in c:
        c[key] = oracle.splat_gaussians(*_args(c)[:4], bg=c["bg"], over=c["over"], **kw)
    return c[key]


# ---------------------------------------------------------------------------------------------------------
# what each case is for, from the reference alone
# ---------------------------------------------------------------------------------------------------------
def _span(t, axis):
    """Per Gaussian: how many tile columns (axis 1: rows) of the bool [n, gy, gx] map hold a tile."""
    return t.any(axis).sum(1)


def _purpose_needles(c, r):
    pairs, reach = r["tiles_member"], r["tiles_reach"]
    share = (pairs & ~reach).sum() / pairs.sum()
    assert share >= 0.25, share
    thin = ((_span(pairs, 1) >= 3) & (_span(reach, 1) == 1)) | ((_span(pairs, 2) >= 3) & (_span(reach, 2) == 1))
    assert thin.any()
    return f"{share:.0%} of {int(pairs.sum())} 3-sigma pairs reach no pixel, {int(thin.sum())} rectangles span >= 3 tiles around a one-tile box"


def _purpose_giants(c, r):
    W, H = c["W"], c["H"]
    big = r["vis"] & (r["radius"] > max(W, H))
    pix = r["proj"]["pix"]
    off = (pix[:, 0] < -0.5) | (pix[:, 0] > W - 0.5) | (pix[:, 1] < -0.5) | (pix[:, 1] > H - 0.5)
    gx, gy = r["proj"]["grid"]
    whole = r["vis"] & off & (r["rect"] == np.array([0, 0, gx, gy])).all(1)
    assert big.sum() >= 10 and whole.sum() >= 5, (big.sum(), whole.sum())
    return f"{int(big.sum())} radii above {max(W, H)} (largest {int(r['radius'].max())}), {int(whole.sum())} off-screen means cover the grid"


def _purpose_near(c, r):
    d = r["d"]
    culled, close = int(((d > 0) & (d <= 0.2)).sum()), int((r["vis"] & (d < 0.3)).sum())
    assert culled >= 20 and close >= 20 and r["counters"]["beyond"] >= 10, (culled, close, r["counters"])
    return f"{culled} culled by d <= 0.2, {close} visible with d < 0.3, {r['counters']['beyond']} beyond the EWA clamp"


def _purpose_opacity_edges(c, r):
    assert r["counters"]["clamped"] > 0 and r["counters"]["stopped"] > 0, r["counters"]
    faint = c["g"]["opacities"] <= np.float32(1.0 / 255.0)
    assert faint.sum() >= 50 and (r["vis"] & faint).sum() >= 50
    assert np.all(r["weight"][faint] == 0.0)
    assert set(np.unique(c["g"]["opacities"])) == set(np.float32(F.OPACITY_EDGES))
    return f"{r['counters']['clamped']} pairs at 0.99, {r['counters']['stopped']} pixels stop, {int(faint.sum())} Gaussians with o <= 1/255 weigh 0"


def _purpose_subpixel(c, r):
    dilation = int(np.ceil(3.0 * np.sqrt(0.3 + np.sqrt(0.1))))
    assert r["vis"].sum() >= 250 and np.all(r["radius"][r["vis"]] == dilation)
    return f"{int(r['vis'].sum())} radii of {dilation}"


def _purpose_ties(c, r):
    m = c["g"]["means"].view(np.uint32)
    assert np.array_equal(m[1::2], m[0::2])
    assert r["tie_pixels"].sum() >= 50, r["tie_pixels"].sum()
    return f"{int(r['tie_pixels'].sum())} pixels blend both Gaussians of a bit-equal pair"


def _purpose_around(c, r):
    share = r["counters"]["culled_near"] / len(r["d"])
    assert share >= 0.4, share
    view = np.asarray(c["ubo"].view, np.float64).reshape(4, 4).T
    assert np.all(view[:3, :] != 0.0)
    assert r["counters"]["culled_behind"] >= 100 and r["vis"].sum() >= 50
    return f"{share:.0%} culled ({r['counters']['culled_behind']} behind), {int(r['vis'].sum())} visible"


def _purpose_lists(c, r):
    lengths = r["tiles_member"].sum(0)
    for (tx, ty), k in F.LIST_TILES.items():
        assert lengths[ty, tx] == k, (tx, ty, lengths[ty, tx])
    assert lengths.sum() == sum(F.LIST_TILES.values())
    deep = int(((r["blended"] >= 20) & ~r["stopped"]).sum())
    assert deep >= 100, deep
    return f"lists {sorted(F.LIST_TILES.values())}, {deep} pixels blend >= 20 entries without stopping (most {int(r['blended'].max())})"


def _purpose_sizes(c, r):
    W, H = c["W"], c["H"]
    assert (W, H) in F.SIZES and r["proj"]["grid"] == ((W + 15) // 16, (H + 15) // 16)
    assert r["image"][..., 3].max() > 0.1
    if W * H < 100:
        assert not c["mask"].any()
    return f"grid {r['proj']['grid']}, largest alpha {r['image'][..., 3].max():.2f}"


def _purpose_over(c, r):
    depth = c["over"][0]
    W = c["W"]
    assert np.all(np.isinf(depth[:, :W // 3])) and len(np.unique(depth[:, W // 3:2 * W // 3])) == 1
    assert np.all(depth[:, 2 * W // 3:].view(np.uint32) == r["d"].astype(np.float32)[c["star"]].view(np.uint32))
    assert r["counters"]["cut"] >= 100 and r["counters"]["limit_equal"] >= 1, r["counters"]
    return f"{r['counters']['cut']} pixels cut by the limit, {r['counters']['limit_equal']} where the limit equals Gaussian {c['star']}'s depth"


def _purpose(name):
    return globals()["_purpose_" + ("sizes" if name.startswith("sizes") else name)]


@pytest.mark.parametrize("name", NAMES)
def test_case_serves_its_purpose(name):
    c = F.case_reference(name)
    print(f"{name}: {_purpose(name)(c, c['r64'])}")
    share = float(c["mask"].mean())
    b_l2, b_px = F.bounds(c)
    print(f"{name}: masked {share:.4f} ({int(c['mask'].sum())} pixels)  e32 {c['e32']:.2e}  e32_px {c['e32_px']:.2e}  "
          f"bounds {b_l2:.1e} / {b_px:.1e}  invdepth e32 {c['e32_inv']:.2e}  e32_px {c['e32_inv_px']:.2e}")
    assert share <= F.MASK_CAP, share
    assert b_px < 1e-3 and F.bounds(c, "invdepth")[1] < 1e-3


def test_membership_margins_are_the_measured_ones():
    """MEASURED holds the largest |float32 - float64| per membership quantity over all cases, rounded up to two
    digits: recomputed here."""
    worst = {k: 0.0 for k in F.MEASURED}
    for name in NAMES:
        c = F.make_case(name)
        p64, p32 = (F.project(*_args(c)[:4], dt) for dt in (np.float64, np.float32))
        diffs = F.membership_diffs(p64, p32)
        print(f"{name}: " + "  ".join(f"{k} {v:.2e}" for k, v in diffs.items()))
        worst = {k: max(worst[k], diffs[k]) for k in worst}
    print("largest: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()) + f"  margins (8x MEASURED): {F.MARGIN}")
    for k, v in worst.items():
        assert 0.9 * F.MEASURED[k] <= v <= F.MEASURED[k], (k, v, F.MEASURED[k])


# ---------------------------------------------------------------------------------------------------------
# the oracle against the reference
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_reference(oracle_lib, name):
    c = F.case_reference(name)
    r, frame = c["r64"], _frame(c, oracle_lib)
    assert np.array_equal(r["vis"], frame["radii"] > 0)
    sure = ~r["member_border"]
    assert np.array_equal(r["radius"][sure], frame["radii"][sure])
    areas = r["tiles_member"].sum((1, 2))
    assert np.array_equal(areas[sure], frame["touched"][sure])
    if sure.all():
        assert r["K"] == frame["K"]
    if c["star"] is not None:  # the limit's band holds the bits of the depth the oracle (and the product) sorts by
        assert frame["depths"][c["star"]].view(np.uint32) == c["over"][0][0, -1].view(np.uint32)
    print(f"{name}: {int(r['vis'].sum())} visible, {int((~sure).sum())} with a borderline membership, K {r['K']} / oracle {frame['K']}")
    failed = F.compare(c, frame["image"], "oracle")
    assert not failed, failed


@pytest.mark.parametrize("name", NAMES)
def test_tight_binning_keeps_what_matters(oracle_lib, name):
    """The alpha box is conservative: every (Gaussian, tile) in which an unmasked pixel has a float64 alpha of
    1/255 (1 + BORDER) or more is among the tight frame's pairs, and the tight frame's image is the same bits."""
    c = F.case_reference(name)
    frame, tight = _frame(c, oracle_lib), _frame(c, oracle_lib, tight=True)
    assert np.array_equal(frame["image"].view(np.uint32), tight["image"].view(np.uint32))
    gx, gy = c["r64"]["proj"]["grid"]
    have = np.zeros(c["r64"]["tiles_strong"].shape, bool)
    tile = (tight["keys"] >> np.uint64(32)).astype(np.int64)
    have[tight["vals"].astype(np.int64), tile // gx, tile % gx] = True
    need = c["r64"]["tiles_strong"]
    print(f"{name}: {int(need.sum())} pairs matter, tight frame holds {tight['K']} of the rectangles' {frame['K']}")
    assert need.sum() > 0 and tight["K"] <= frame["K"]
    assert not (need & ~have).any(), np.argwhere(need & ~have)[:5]


def test_tile_row_shards_of_the_reference(oracle_lib):
    """render(tile_rows=) clamps the rectangles as the oracle does, and the shards compose to the full image."""
    c = F.case_reference("giants")
    whole = np.zeros_like(c["r64"]["image"])
    for rows in ((0, 1), (1, 3)):
        part = F.render(*_args(c), tile_rows=rows)
        frame = oracle_lib.splat_gaussians(*_args(c)[:4], bg=c["bg"], tile_rows=rows)
        assert np.array_equal(part["vis"], frame["radii"] > 0) and part["K"] == frame["K"]
        whole[16 * rows[0]:16 * rows[1]] = part["image"][16 * rows[0]:16 * rows[1]]
    assert np.array_equal(whole, c["r64"]["image"])


# ---------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------
def _heaviest_tile(r):
    gi, ty, tx = np.unravel_index(np.argmax(r["tiles_weight"]), r["tiles_weight"].shape)
    return ("drop", int(gi), (int(tx), int(ty)))


def _costliest_radius(c, r):
    """The Gaussian that loses the most weight when its radius shrinks by one."""
    p = r["proj"]
    rect = F._rects(p["pix"][:, 0], p["pix"][:, 1], np.maximum(p["radius"] - 1, 0), *p["grid"], p["rows"])[0]
    lost = r["tiles_member"] & ~F._tile_map(rect, *p["grid"])
    return ("radius", int(np.argmax((r["tiles_weight"] * lost).sum((1, 2)))), -1)


def _tie_swap(c, r):
    w = r["weight"]
    k = int(np.argmax(np.minimum(w[0::2], w[1::2])))
    return ("swap", 2 * k, 2 * k + 1)


def _deep_swap(c, r):
    """Two neighbours in the order, deep inside the largest list, that overlap the most."""
    (tx, ty), n = max(F.LIST_TILES.items(), key=lambda kv: kv[1])
    inside = r["order"][r["tiles_member"][r["order"], ty, tx]]
    assert len(inside) == n
    lo = n // 2
    pix = r["proj"]["pix"]
    gap = np.linalg.norm(pix[inside[lo:-1]] - pix[inside[lo + 1:]], axis=1)
    k = lo + int(np.argmin(gap))
    return ("swap", int(inside[k]), int(inside[k + 1]))


def _mutations(name, c, r):
    if name in ("needles", "giants"):
        return [_heaviest_tile(r), _costliest_radius(c, r)]
    if name == "near":
        return [("near", 0.25)]
    if name == "opacity_edges":
        return ["no_clamp", "no_stop", "no_skip"]
    if name == "ties":
        return [_tie_swap(c, r)]
    if name == "lists":
        return [_deep_swap(c, r)]
    if name == "over":
        return [("over_le",)]
    return [_heaviest_tile(r)]  # subpixel, around, sizes


@pytest.mark.parametrize("name", NAMES)
def test_mutations_are_visible(name):
    c = F.case_reference(name)
    r = c["r64"]
    ok = ~c["mask"]
    b_px = F.bounds(c)[1]
    for mutate in _mutations(name, c, r):
        wrong = F.render(*_args(c), over=c["over"], mutate=mutate)
        moved = float(np.abs(wrong["image"] - r["image"])[ok].max())
        print(f"{name} {mutate}: moves an unmasked pixel by {moved:.2e} (4x the per-pixel bound: {4 * b_px:.1e})")
        assert moved > 4.0 * b_px, (mutate, moved, b_px)


# ---------------------------------------------------------------------------------------------------------
# the two projections
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_projection_agrees_with_the_backward_reference(name):
    c = F.make_case(name)
    p = F.project(*_args(c)[:4])
    vis = np.flatnonzero(p["vis"])
    t = lambda k: torch.tensor(np.asarray(c["g"][k], np.float64)[vis])
    m2d, conic = G._project(t("means"), t("scales"), t("rotations"), c["ubo"].view, c["ubo"].proj, c["W"], c["H"])
    for got, want, what in ((p["pix"][vis], m2d.numpy(), "means2d"), (p["conic"][vis], conic.numpy(), "conic")):
        err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
        print(f"{name} {what}: {err:.2e}")
        assert err <= 1e-12, (what, err)
