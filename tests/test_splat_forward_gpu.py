"""The 3DGS forward on the GPU against the tile-free float64 reference (tests/splat_forward_ref.py) on hard inputs:
needles, giants, the near plane, opacity edges, sub-pixel Gaussians, bit-equal means, a posed camera with Gaussians
behind it, lists of 257 / 513 / 2 100 pairs, frames smaller than a tile, the over composite. Every way the product
renders a frame is compared on the pixels no borderline decision reaches (the reference's mask, at most 1 % of a
case): the published frame, stream-ordered frames with the alpha-box binning on the previous frame's hints, tile-row
shards with and without the row pre-cull and the chunk cull, one of several views, frames in flight, the inverse
depth, and for `over` the composite into a separate buffer and in place. Bounds: relative L2 max(1e-4, 8 e32), per
pixel and channel max(8 e32_px, 8 2^-23), e32 being the float32 evaluation of the reference against float64; where
the project promises equal bits, those are asserted too. tests/test_splat_forward_ref.py checks the cases, the mask
and the comparison's teeth on the CPU.

What it found (MI355X): the blend evaluated z from the quadratic expanded about the tile's corner, A ux^2 + B ux uy
+ C uy^2 + D ux + E uy + F. For a Gaussian that is all dilation (conic 1 / 0.3) F and D ux reach 1 200 inside the
tile and cancel to a z of a few units: 1e-4 in z, and in the image max abs 4.69e-05 at (y 26, x 31) of `subpixel`
(bound 2.2e-05), 2.59e-05 at (15, 25) of `opacity_edges` (6.6e-06), 2.22e-05 at (9, 31) of `ties` (1.4e-05),
1.56e-05 at (2, 14) of `sizes_16x16` (2.6e-06), 1.82e-05 at (12, 8) of `sizes_17x15` (5.9e-06), in every mode alike;
the relative L2 stayed under 7.9e-6. splat_blend.h now takes z from (dx, dy) = pixel - mean, as ptgs.h states it."""
import numpy as np
import pytest

import splat_forward_ref as F

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

NAMES = list(F.CASES)
FILL = -7.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_DEV = {}


def _case(name):
    """The case's reference and its device arrays: "dg", "dover" ((depth, under) or None)."""
    c = F.case_reference(name)
    if name not in _DEV:
        _DEV[name] = ({k: _dev(v) for k, v in c["g"].items()}, None if c["over"] is None else tuple(_dev(a) for a in c["over"]))
    return c, _DEV[name][0], _DEV[name][1]


def _plain(name):
    """For the calls that take no depth limit (views, inverse depth): `over` is `around`'s Gaussians and camera."""
    if name != "over":
        return _case(name)
    c, a = F.case_reference("over"), F.case_reference("around")
    assert all(np.array_equal(c["g"][k], a["g"][k]) for k in a["g"]) and bytes(c["ubo"]) == bytes(a["ubo"])
    return _case("around")


def _buf(c):
    return torch.full((c["H"], c["W"], 4), FILL, dtype=torch.float32, device="cuda")


def _frame(r, c, dg, dover, **kw):
    out = _buf(c)
    st = r.splat_gaussians(dg, c["ubo"], c["W"], c["H"], out, bg=c["bg"], over=dover, **kw)
    return out, st


def _check(c, got, label, key="image"):
    torch.cuda.synchronize()
    failed = F.compare(c, got.cpu().numpy(), label, key)
    assert not failed, failed


_PUBLISHED = {}


def _read(renderer, ptr, n, dtype):
    out = np.zeros(n, dtype)
    renderer.copy_d2h(out, ptr, out.nbytes)
    return out


def _published(renderer, name):
    """(1): the synchronised frame with stats, 3-sigma rectangles, rendered once per case: (image (a device
    tensor), K, radii, tiles touched)."""
    if name not in _PUBLISHED:
        c, dg, dover = _case(name)
        out, st = _frame(renderer, c, dg, dover, want_stats=True)
        torch.cuda.synchronize()
        b, n = renderer.splat_buffers(), len(c["g"]["opacities"])
        _PUBLISHED[name] = (out, st.num_rendered, _read(renderer, b.radii, n, np.int32),
                            _read(renderer, b.tiles_touched, n, np.uint32))
    return _PUBLISHED[name]


@pytest.fixture(scope="module")
def tight_renderer(native_lib):
    from pathtracer_gaussiansplatting_amd import Renderer
    r = Renderer(0, publish_splat_buffers="tight")
    yield r
    r.close()


@pytest.mark.parametrize("name", NAMES)
def test_published_frame(renderer, name):
    """The image, and what the reference says each Gaussian is: culled or not, its radius, its rectangle's area."""
    c, _, _ = _case(name)
    out, K, radii, touched = _published(renderer, name)
    r = c["r64"]
    sure = ~r["member_border"]
    assert np.array_equal(radii > 0, r["vis"])
    assert np.array_equal(radii[sure], r["radius"][sure])
    assert np.array_equal(touched[sure], r["tiles_member"].sum((1, 2))[sure])
    if sure.all():
        assert K == r["K"], (K, r["K"])
    _check(c, out, "published")


@pytest.mark.parametrize("name", NAMES)
def test_stream_ordered_tight_frames(renderer, tight_renderer, name):
    """Frames without stats bin by the alpha box; the 2nd and 3rd run the front end the previous frame's report
    chose. A published tight frame has their bits."""
    c, dg, dover = _case(name)
    frames = []
    tight_renderer.splat_status()  # (the counts are since the last query)
    for k in range(3):
        frames.append(_frame(tight_renderer, c, dg, dover)[0])
        torch.cuda.synchronize()  # (frame k's report reaches the host before frame k + 1)
    st = tight_renderer.splat_status()
    assert st.frames == 0 and st.incomplete_tiles == 0, (st.frames, st.incomplete_tiles)
    for k in (1, 2):
        _check(c, frames[k], f"stream-ordered frame {k + 1}")
    pub, stats = _frame(tight_renderer, c, dg, dover, want_stats=True)
    torch.cuda.synchronize()
    assert stats.num_rendered <= _published(renderer, name)[1]
    for k in (1, 2):
        assert torch.equal(frames[k], pub), f"stream-ordered frame {k + 1} != published tight frame"


def _shards(gy):
    two = [(0, gy)] if gy < 2 else [(0, gy // 2), (gy // 2, gy)]
    each = [(k, k + 1) for k in range(gy)]
    return {"two": two, "each": each}


@pytest.mark.parametrize("name", NAMES)
def test_tile_row_shards_compose(renderer, name):
    """Restricted frames written into one buffer, as given and as the Morton copy with ids and chunk bounds (the row
    pre-cull and the chunk cull): the composed image is the published frame's, bit for bit."""
    c, dg, dover = _case(name)
    whole = _published(renderer, name)[0]
    ds = renderer.sort_gaussians_spatial(dg)
    assert sorted(ds["ids"].cpu().tolist()) == list(range(len(c["g"]["opacities"])))
    dsb = dict(ds, chunk_bounds=renderer.gaussians_chunk_bounds(ds))
    copy, _ = _frame(renderer, c, ds, dover, want_stats=True)
    _check(c, copy, "ids copy")
    assert torch.equal(copy, whole), "the ids copy does not render like the original order"
    gy = (c["H"] + 15) // 16
    for gname, gs in (("as given", dg), ("ids + chunk bounds", dsb)):
        for sname, shards in _shards(gy).items():
            out = _buf(c)
            for rows in shards:
                renderer.splat_gaussians(gs, c["ubo"], c["W"], c["H"], out, bg=c["bg"], tile_rows=rows, over=dover)
            _check(c, out, f"shards {sname} {shards} {gname}")
            assert torch.equal(out, whole), f"shards {sname} {gname}: not the published frame"


@pytest.mark.parametrize("name", NAMES)
def test_one_of_three_views(renderer, name):
    c, dg, _ = _plain(name)
    W, H = c["W"], c["H"]
    ubos = [F.make_ubo(W, H, (0.5, 0.2, 1.0), (0.0, 0.0, -8.0)), c["ubo"], F.make_ubo(W, H, (-2.0, 1.0, 0.0), (0.5, 0.0, -6.0))]
    outs = [_buf(c) for _ in ubos]
    renderer.splat_gaussians_views(dg, ubos, W, H, outs, bg=c["bg"])
    _check(c, outs[1], "view 2 of 3")
    for o in (outs[0], outs[2]):
        assert bool(torch.isfinite(o).all()) and not bool((o == FILL).any())
    assert torch.equal(outs[1], _published(renderer, c["name"])[0])


@pytest.mark.parametrize("name", NAMES)
def test_frames_in_flight(renderer, name):
    c, dg, dover = _case(name)
    whole = _published(renderer, name)[0]
    renderer.splat_status()  # (clears the counts that earlier tests left on the shared context)
    renderer.set_splat_overlap(True)
    try:
        outs = [_frame(renderer, c, dg, dover)[0] for _ in range(4)]
        torch.cuda.synchronize()
    finally:
        renderer.set_splat_overlap(False)
    st = renderer.splat_status()
    assert st.frames == 0 and st.incomplete_tiles == 0
    for k, o in enumerate(outs):
        _check(c, o, f"in flight {k + 1}")
        assert torch.equal(o, whole), f"frame in flight {k + 1} != published frame"


@pytest.mark.parametrize("name", NAMES)
def test_inverse_depth(renderer, name):
    c, dg, _ = _plain(name)
    _frame(renderer, c, dg, None, want_stats=True)
    inv = renderer.splat_gaussians_invdepth(c["W"], c["H"])
    _check(c, inv, "inverse depth", key="invdepth")


@pytest.mark.parametrize("want_stats", [False, True])
def test_over_separate_and_in_place(renderer, want_stats):
    c, dg, (depth, under) = _case("over")
    whole = _published(renderer, "over")[0]
    separate, _ = _frame(renderer, c, dg, (depth, under), want_stats=want_stats)
    _check(c, separate, f"over, separate buffer, stats {want_stats}")
    buf = under.clone()
    renderer.splat_gaussians(dg, c["ubo"], c["W"], c["H"], buf, over=(depth, buf), want_stats=want_stats)
    _check(c, buf, f"over, in place, stats {want_stats}")
    assert torch.equal(separate, whole) and torch.equal(buf, whole)
