"""The stream-ordered 3DGS splat behind a moving camera: PTGS_OK must mean a
rendered frame. The reference's viewer renders a new view every frame (camera.cpp:11,
engine.cpp:2070-2072); the splat sizes its per-tile rows, its pair buffer and its tile order from
earlier frames, so a camera that moves closer than the previous frame outgrows them. Those tiles are
completed on the device through the spill pool (gs_spill_tile): every frame here must equal the exact
(stats, re-run) frame bit for bit - whose published keys / values / ranges are the oracle's - and the
oracle's image within 1e-4 relative L2.
"""
import numpy as np
import pytest

import scenes_util as U
from pathtracer_gaussiansplatting_amd import Camera, make_ubo
from pathtracer_gaussiansplatting_amd import synthetic as Y

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _read(renderer, ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        renderer.copy_d2h(out, ptr, out.nbytes)
    return out


def orbit_ubo(k, W, H, radius=None, sc=None):
    """Frame k of an orbit around the C2 cloud's centre (0, 0, -8) with a slow dolly-in; frame k = 0 is
    the C2 camera (origin, looking down -Z)."""
    r = 8.0 - 0.2 * k if radius is None else radius
    th = np.radians(4.0 * k)
    c = np.array([0.0, 0.0, -8.0])
    eye = c + np.array([r * np.sin(th), 0.15 * r * np.sin(0.5 * th), r * np.cos(th)])
    pose = Camera(aspect=W / H).look_at(eye.tolist(), c.tolist())
    return make_ubo(pose, U.cornell() if sc is None else sc, 0)


def _exact(r2, dg, ubo, W, H, oracle_lib, g, bg=(0.0, 0.0, 0.0)):
    """The exact frame: stats (a frame that spilled is re-run through three launches with grown
    buffers) + published keys / values / ranges, checked against the oracle."""
    out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    st = r2.splat_gaussians(dg, ubo, W, H, out, bg=bg, want_stats=True)
    torch.cuda.synchronize()
    ref = oracle_lib.splat_gaussians(g, ubo, W, H, bg=bg)
    b = r2.splat_buffers()
    assert st.num_rendered == ref["K"]
    np.testing.assert_array_equal(_read(r2, b.sorted_keys, ref["K"], np.uint64), ref["keys"])
    np.testing.assert_array_equal(_read(r2, b.sorted_values, ref["K"], np.uint32), ref["vals"])
    np.testing.assert_array_equal(_read(r2, b.tile_ranges, 2 * b.num_tiles, np.uint32), ref["ranges"])
    err = U.rel_l2(out.cpu().numpy(), ref["image"])
    assert err < 1e-4, err
    return out, ref


def test_gaussians_moving_camera_sequence(native_lib, oracle_lib):
    """An orbiting, dollying camera over 20k C2 Gaussians (Morton copy with ids: the fused front end,
    rows sized from the previous frame), with one sudden zoom out that grows the densest tile far past
    its row (into the pool-sorted spill path): every stream-ordered frame (no
    stats) equals the exact frame bit for bit (keys / values / ranges of the exact frame = the
    oracle's), no frame is incomplete, and the zoom frame spilled."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=31)
    g["means"][1::59] = g["means"][0::59][: len(g["means"][1::59])]  # duplicated means: equal depths
    # orbit + dolly-in, then a sudden dolly-out to 20 units (the whole cloud in a few hundred tiles:
    # the densest tile grows from ~380 to ~2300 pairs, past the 512-pair rows sized from frame 7 and
    # past the spill LDS sort), further out, then back into the orbit
    frames = [orbit_ubo(k, W, H) for k in range(8)] + [orbit_ubo(8, W, H, radius=20.0)] + \
             [orbit_ubo(k, W, H, radius=20.0 + 3.0 * (k - 8)) for k in range(9, 12)] + \
             [orbit_ubo(k, W, H) for k in (12, 13)]
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers=True)
    try:
        da = ra.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        db = {k: _dev(v) for k, v in g.items()}
        spilled = []
        for k, ubo in enumerate(frames):
            out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
            ra.splat_gaussians(da, ubo, W, H, out, bg=(0.1, 0.2, 0.3))  # stream-ordered
            st = ra.splat_status()
            assert st.frames == 0 and st.incomplete_tiles == 0, (k, st.frames, st.incomplete_tiles)
            spilled.append(int(st.spilled_tiles))
            exact, ref = _exact(rb, db, ubo, W, H, oracle_lib, g, bg=(0.1, 0.2, 0.3))
            assert torch.equal(out, exact), f"frame {k}: stream-ordered != exact"
        print("spilled tiles per frame:", spilled)
        assert spilled[8] > 0, spilled  # the zoom outgrew the rows sized from frame 7
        assert ra.splat_status().fused == 1
    finally:
        ra.close()
        rb.close()


def test_gaussians_timed_c2_mode_vs_oracle(native_lib, oracle_lib):
    """The exact mode bench.py's C2 headline times: 100k Gaussians at 1920x1080, a Morton-ordered copy
    with ids (ptgs_gaussians_sort_spatial), no stats, steady state (fused front end, rows and tile
    order from the previous frame). Its frames equal the oracle's image (< 1e-4) and, bit for bit, the
    exact published frame whose keys / values / ranges are the oracle's; nothing spills."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 1920, 1080, 100_000
    g = Y.gaussians_c2(n, seed=1)
    sc = U.cornell()
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), sc, 0)
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers=True)
    try:
        dg = ra.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        outs = []
        for k in range(4):  # frame 0: three launches; 1..3: fused, steady state
            out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            ra.splat_gaussians(dg, ubo, W, H, out)
            outs.append(out)
            if k == 0:
                # the row sizes reach the host once frame 0 has run (a finished frame's hint, never
                # waited for by the call): without this wait a fast host enqueues every frame before
                # frame 0 has finished, and they all take the three-launch path
                torch.cuda.synchronize()
        st = ra.splat_status()
        assert st.fused == 1 and st.frames == 0 and st.spilled_tiles == 0, (st.fused, st.frames, st.spilled_tiles)
        exact, ref = _exact(rb, {k: _dev(v) for k, v in g.items()}, ubo, W, H, oracle_lib, g)
        for k, o in enumerate(outs):
            assert torch.equal(o, exact), k
        print(f"C2 timed mode: K={ref['K']}, rel L2 vs oracle {U.rel_l2(outs[-1].cpu().numpy(), ref['image']):.2e}")
    finally:
        ra.close()
        rb.close()


def test_gaussians_graph_replay_fused_spill(native_lib, oracle_lib):
    """a hipGraph of a fused frame bakes its row capacity. Replays of that graph after the
    Gaussians were made denser in place (tiles above the rows) must render completely through the
    spill pool, and a later replay of the original data must render normally again (no stale state
    left by the spilled replay)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 320, 180, 20_000
    s1 = Y.gaussians_c2(n, seed=41)
    s2 = {k: v.copy() for k, v in s1.items()}
    s2["means"][:, :2] *= np.float32(0.5)  # the cloud squeezed to half the width: tiles of up to ~3000
                                           # pairs, above the 1024-pair rows sized from s1's ~800
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers=True)
    try:
        dg = ra.sort_gaussians_spatial({k: _dev(v) for k, v in s1.items()})
        ids = dg["ids"].cpu().numpy().astype(np.int64)
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for _ in range(3):
            ra.splat_gaussians(dg, ubo, W, H, out, want_stats=True)
        assert ra.splat_status().fused == 1
        exact1, ref1 = _exact(rb, {k: _dev(v) for k, v in s1.items()}, ubo, W, H, oracle_lib, s1)
        exact2, ref2 = _exact(rb, {k: _dev(v) for k, v in s2.items()}, ubo, W, H, oracle_lib, s2)
        assert int(np.diff(ref2["ranges"].reshape(-1, 2), axis=1).max()) > \
            2 * int(np.diff(ref1["ranges"].reshape(-1, 2), axis=1).max())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ra.splat_gaussians(dg, ubo, W, H, out)

        def load(src):
            for k in ("means", "scales", "rotations", "opacities", "colors"):
                dg[k].copy_(_dev(src[k][ids]))
            torch.cuda.synchronize()

        for data, exact in ((s1, exact1), (s2, exact2), (s1, exact1), (s2, exact2)):
            load(data)
            out.fill_(-7.0)
            graph.replay()
            torch.cuda.synchronize()
            st = ra.splat_status()
            assert st.frames == 0 and st.incomplete_tiles == 0
            assert (st.spilled_tiles > 0) == (data is s2), st.spilled_tiles
            assert torch.equal(out, exact)
        del graph
    finally:
        ra.close()
        rb.close()


def test_gaussians_spill_tiles_beyond_lds(native_lib, oracle_lib):
    """Spilled tiles of more than GS_SPILL_LDS (1984) pairs are sorted in the spill pool (global
    bitonic) instead of the blend's LDS: 3000 screen-filling Gaussians at 128x72 on a fresh context
    (every tile holds ~3000 pairs, K ~ 120k > the 8-per-Gaussian pair buffer)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H = 128, 72
    g = Y.gaussians_c2(3000, seed=43)
    g["scales"] *= np.float32(40.0)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers=True)
    try:
        dg = {k: _dev(v) for k, v in g.items()}
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        ra.splat_gaussians(dg, ubo, W, H, out)
        st = ra.splat_status()
        exact, ref = _exact(rb, dg, ubo, W, H, oracle_lib, g)
        per_tile = np.diff(ref["ranges"].reshape(-1, 2), axis=1).ravel()
        assert per_tile.max() > 1984 and ref["K"] > 8 * 3000, (per_tile.max(), ref["K"])
        assert st.frames == 0 and st.incomplete_tiles == 0 and st.spilled_tiles > 0
        assert torch.equal(out, exact)
    finally:
        ra.close()
        rb.close()


def test_gaussians_spill_pool_exhausted_is_reported(native_lib):
    """The only incomplete case: a frame whose spilled tiles need more than the spill pool (here ~16M
    pairs on a fresh context: 2000 screen-filling Gaussians at 1920x1080 against an 8-per-Gaussian
    pair buffer and a 2^20-pair pool). Its tiles beyond the pool stay at the background, and the next
    call - after that frame finished - returns PTGS_EINCOMPLETE having grown the buffers and rendered
    its own frame completely; ptgs_splat_reserve rules the case out beforehand."""
    from pathtracer_gaussiansplatting_amd import Renderer, PtgsError
    from pathtracer_gaussiansplatting_amd._abi import PTGS_EINCOMPLETE
    W, H = 1920, 1080
    g = Y.gaussians_c2(2000, seed=45)
    g["scales"] *= np.float32(60.0)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    dg = {k: _dev(v) for k, v in g.items()}
    rb = Renderer(0)
    try:
        exact = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        st = rb.splat_gaussians(dg, ubo, W, H, exact, want_stats=True)
        K = st.num_rendered
        assert K > (1 << 20) + 8 * 2000, K
    finally:
        rb.close()
    ra = Renderer(0)
    try:
        out = torch.zeros_like(exact)
        ra.splat_gaussians(dg, ubo, W, H, out)  # incomplete: its spilled tiles exceed the pool
        torch.cuda.synchronize()
        with pytest.raises(PtgsError) as ei:
            ra.splat_gaussians(dg, ubo, W, H, out)  # reports the earlier frame; renders its own
        assert ei.value.code == PTGS_EINCOMPLETE
        torch.cuda.synchronize()
        st = ra.splat_status()
        assert st.frames == 1 and st.incomplete_tiles > 0, (st.frames, st.incomplete_tiles)
        assert torch.equal(out, exact)  # the reporting call's own frame is complete
        ra.splat_gaussians(dg, ubo, W, H, out)  # nothing more to report
        st = ra.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0 and torch.equal(out, exact)
    finally:
        ra.close()
    rc = Renderer(0)
    try:
        rc.splat_reserve(K)  # reserved: the first stream-ordered frame is complete
        out = torch.zeros_like(exact)
        rc.splat_gaussians(dg, ubo, W, H, out)
        st = rc.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0 and torch.equal(out, exact)
    finally:
        rc.close()


def test_gaussians_views_pool_exhausted_renders_every_view(native_lib):
    """a views call whose view v >= 1 reports an earlier incomplete frame still renders every
    view (the report is returned after all of them are enqueued), and the reporting call's own frames are
    complete. Two views of the exhausting frame above on a fresh context: both are incomplete; the next
    views call returns PTGS_EINCOMPLETE with both outputs equal to the exact frame."""
    from pathtracer_gaussiansplatting_amd import Renderer, PtgsError
    from pathtracer_gaussiansplatting_amd._abi import PTGS_EINCOMPLETE
    W, H = 1920, 1080
    g = Y.gaussians_c2(2000, seed=45)
    g["scales"] *= np.float32(60.0)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    dg = {k: _dev(v) for k, v in g.items()}
    rb = Renderer(0)
    try:
        exact = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rb.splat_gaussians(dg, ubo, W, H, exact, want_stats=True)
    finally:
        rb.close()
    ra = Renderer(0)
    try:
        outs = [torch.zeros_like(exact) for _ in range(2)]
        ra.splat_gaussians_views(dg, [ubo, ubo], W, H, outs)  # both views exhaust their pools
        torch.cuda.synchronize()
        outs = [torch.full_like(exact, -3.0) for _ in range(2)]
        with pytest.raises(PtgsError) as ei:
            ra.splat_gaussians_views(dg, [ubo, ubo], W, H, outs)
        assert ei.value.code == PTGS_EINCOMPLETE
        torch.cuda.synchronize()
        for v, o in enumerate(outs):  # (before the fix view 0 was never enqueued: still -3)
            assert torch.equal(o, exact), f"view {v} not rendered completely"
        st = ra.splat_status()
        assert st.views[0] + st.views[1] >= 1 and st.incomplete_tiles > 0
        ra.splat_gaussians_views(dg, [ubo, ubo], W, H, outs)  # nothing more to report
        st = ra.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0
        assert all(torch.equal(o, exact) for o in outs)
    finally:
        ra.close()


def test_gaussians_out_of_range_ids_are_reported(native_lib, oracle_lib):
    """ids must be a permutation of [0, N). An id >= N is never used as an index (the
    Gaussian is dropped: no out-of-bounds write) and the next call returns PTGS_EBADIDS (its own code:
    a report about an earlier frame, not this call's PTGS_EINVAL)."""
    from pathtracer_gaussiansplatting_amd import Renderer, PtgsError
    from pathtracer_gaussiansplatting_amd._abi import PTGS_EBADIDS
    W, H, n = 160, 96, 2000
    g = Y.gaussians_c2(n, seed=47)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    r = Renderer(0)
    try:
        dg = {k: _dev(v) for k, v in g.items()}
        good = torch.arange(n, dtype=torch.int32, device="cuda")
        bad = good.clone()
        bad[17] = n + 5
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        r.splat_gaussians(dict(dg, ids=bad), ubo, W, H, out)
        torch.cuda.synchronize()
        with pytest.raises(PtgsError) as ei:
            r.splat_gaussians(dict(dg, ids=good), ubo, W, H, out)
        assert ei.value.code == PTGS_EBADIDS
        r.splat_gaussians(dict(dg, ids=good), ubo, W, H, out)
        torch.cuda.synchronize()
        ref = oracle_lib.splat_gaussians(g, ubo, W, H)
        assert U.rel_l2(out.cpu().numpy(), ref["image"]) < 1e-4
    finally:
        r.close()


def test_gaussians_both_reports_are_returned_in_turn(native_lib, oracle_lib):
    """One frame that both exhausts its spill pool and carries an id >= N leaves two reports (ptgs.h,
    PTGS_EBADIDS: the order of the reports). The next call returns PTGS_EBADIDS, the call after it
    PTGS_EINCOMPLETE, the third PTGS_OK: neither report is dropped, each is returned once, and both
    reporting calls render their own frame completely (the exact frame bit for bit). On a fresh context
    the pair buffer and the pool hold 8 N + 2^20 pairs; the oracle's count for the frame is over twice that
    (asserted from the oracle, not from the library)."""
    from pathtracer_gaussiansplatting_amd import Renderer, PtgsError
    from pathtracer_gaussiansplatting_amd._abi import PTGS_EBADIDS, PTGS_EINCOMPLETE
    W, H, n = 960, 544, 3000
    g = Y.gaussians_c2(n, seed=45)
    g["scales"] *= np.float32(60.0)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    capacity = (1 << 20) + 8 * n
    K = oracle_lib.splat_gaussians(g, ubo, W, H, tight=True)["K"]  # (good ids; one dropped Gaussian: < 0.1 % fewer)
    assert K >= 2 * capacity, (K, capacity)
    dg = {k: _dev(v) for k, v in g.items()}
    good = torch.arange(n, dtype=torch.int32, device="cuda")
    bad = good.clone()
    bad[17] = n + 5
    rb = Renderer(0)
    try:
        exact = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        rb.splat_gaussians(dict(dg, ids=good), ubo, W, H, exact, want_stats=True)
    finally:
        rb.close()
    ra = Renderer(0)
    try:
        out = torch.zeros_like(exact)
        ra.splat_gaussians(dict(dg, ids=bad), ubo, W, H, out)  # incomplete, and met the bad id
        torch.cuda.synchronize()
        for code in (PTGS_EBADIDS, PTGS_EINCOMPLETE):
            out.fill_(-3.0)
            with pytest.raises(PtgsError) as ei:
                ra.splat_gaussians(dict(dg, ids=good), ubo, W, H, out)
            assert ei.value.code == code, (ei.value.code, code)
            torch.cuda.synchronize()
            assert torch.equal(out, exact), f"the call reporting {code} did not render its own frame completely"
        out.fill_(-3.0)
        ra.splat_gaussians(dict(dg, ids=good), ubo, W, H, out)  # nothing more to report
        torch.cuda.synchronize()
        assert torch.equal(out, exact)
        st = ra.splat_status()
        assert st.frames == 1 and st.incomplete_tiles > 0, (st.frames, st.incomplete_tiles)
        st = ra.splat_status()  # (counted once)
        assert st.frames == 0 and st.incomplete_tiles == 0, (st.frames, st.incomplete_tiles)
    finally:
        ra.close()


@pytest.mark.parametrize("radius", [8.0, 5.0, 2.5, 20.0])
def test_gaussians_tile_row_bands_with_chunk_bounds(native_lib, oracle_lib, radius):
    """a tile-row-restricted frame with ptgs_gaussians.chunk_bounds skips the
    256-Gaussian chunks whose conservative screen bound misses its rows before loading them. Over
    camera distances from outside the cloud to inside it (chunks straddling the near plane), every band
    of 4 keeps the oracle's keys / values / ranges / radii / tiles touched of those rows bit for bit,
    and the bands compose the full frame exactly (both front ends: frame 0 three launches, then fused)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=51)
    ubo = orbit_ubo(5, W, H, radius=radius)
    gy = (H + 15) // 16
    bands = [(0, 4), (4, 9), (9, 13), (13, gy)]
    r = Renderer(0, publish_splat_buffers=True)
    try:
        dg = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        dgb = dict(dg, chunk_bounds=r.gaussians_chunk_bounds(dg))
        full = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        r.splat_gaussians(dg, ubo, W, H, full, bg=(0.1, 0.2, 0.3), want_stats=True)
        for frame in range(2):
            comp = torch.full_like(full, -7.0)
            for rows in bands:
                st = r.splat_gaussians(dgb, ubo, W, H, comp, bg=(0.1, 0.2, 0.3), tile_rows=rows, want_stats=True)
                torch.cuda.synchronize()
                ref = oracle_lib.splat_gaussians(g, ubo, W, H, bg=(0.1, 0.2, 0.3), tile_rows=rows)
                b = r.splat_buffers()
                assert st.num_rendered == ref["K"], (rows, st.num_rendered, ref["K"])
                np.testing.assert_array_equal(_read(r, b.sorted_keys, ref["K"], np.uint64), ref["keys"])
                np.testing.assert_array_equal(_read(r, b.sorted_values, ref["K"], np.uint32), ref["vals"])
                np.testing.assert_array_equal(_read(r, b.tile_ranges, 2 * b.num_tiles, np.uint32), ref["ranges"])
                np.testing.assert_array_equal(_read(r, b.radii, n, np.int32), ref["radii"])
                np.testing.assert_array_equal(_read(r, b.tiles_touched, n, np.uint32), ref["touched"])
            assert torch.equal(comp, full), f"bands != full frame (frame {frame})"
    finally:
        r.close()


@pytest.mark.parametrize("shape", ["c2", "thin_faint"])
def test_gaussians_alpha_box_binning_is_exact(native_lib, oracle_lib, shape):
    """Timed (stream-ordered, unpublished, no stats) frames bin each Gaussian to the tiles its alpha
    box overlaps instead of the reference's 3-sigma rectangle: fewer pairs, the same image bit for bit
    (a pair outside the box has alpha < 1/255 at every pixel: the blend skips it exactly). Covered
    with C2's Gaussians and with elongated, rotated, faint ones (opacities down to 1e-3, below the
    1/255 cut: never binned) over a few camera positions."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=53)
    if shape == "thin_faint":
        rng = np.random.default_rng(7)
        g["scales"] = (g["scales"] * rng.choice([0.05, 1.0, 4.0], size=(n, 3))).astype(np.float32)
        g["opacities"] = rng.uniform(1e-3, 1.0, size=g["opacities"].shape).astype(np.float32) ** 3
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers=True)
    try:
        da = ra.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        db = {k: _dev(v) for k, v in g.items()}
        for k, ubo in enumerate([orbit_ubo(j, W, H) for j in (0, 3)] + [orbit_ubo(6, W, H, radius=3.0)]):
            for _ in range(2):  # three launches, then the fused front end
                out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
                ra.splat_gaussians(da, ubo, W, H, out, bg=(0.1, 0.2, 0.3))
                st = ra.splat_status()
                assert st.frames == 0 and st.incomplete_tiles == 0
                exact, ref = _exact(rb, db, ubo, W, H, oracle_lib, g, bg=(0.1, 0.2, 0.3))
                assert torch.equal(out, exact), f"view {k}: box-binned frame != exact"
                assert 0 < st.last_pairs < ref["K"], (st.last_pairs, ref["K"])
            print(f"view {k}: pairs {st.last_pairs} of the reference's {ref['K']}")
    finally:
        ra.close()
        rb.close()


def test_row_gather_pipeline_streams_on_one_gpu(native_lib):
    """dist.RowGatherPipeline's device path (the bench's multi-rank C2 leg): two images alternate on the
    compute stream, each frame's gather is issued on a second stream behind an event and the frame two
    later waits for it. On one GPU without a process group the gather is a no-op, so what is checked is
    the stream / event plumbing: a moving sequence through the pipeline leaves each image equal, bit for
    bit, to the same frame rendered directly."""
    from pathtracer_gaussiansplatting_amd import Renderer
    from pathtracer_gaussiansplatting_amd import dist as D
    W, H, n = 640, 360, 30_000
    g = Y.gaussians_c2(n, seed=17)
    poses = [Camera(aspect=W / H).look_at([0.3 * k, 0.1 * k, -0.4 * k], [0.0, 0.0, -8.0]) for k in range(5)]
    ubos = [make_ubo(p, U.cornell(), 0) for p in poses]
    r = Renderer(0)
    try:
        dg = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        s = torch.cuda.Stream()
        pipe = D.RowGatherPipeline(r, W, H, [(0, (H + 15) // 16)], 0, 1, stream=s)
        outs = []
        with torch.cuda.stream(s):
            for u in ubos:
                outs.append(pipe.submit(dg, u))
            pipe.wait()
        s.synchronize()
        got = [outs[-2].clone(), outs[-1].clone()]
        for img, u in zip(got, ubos[-2:]):
            ref = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            r.splat_gaussians(dg, u, W, H, ref)
            torch.cuda.synchronize()
            assert torch.equal(img, ref)
        assert outs[-1] is not outs[-2] and outs[-1] is outs[-3]  # two images alternate
    finally:
        r.close()


def _overlap_frames(W, H):
    """The moving-camera sequence of test_gaussians_moving_camera_sequence (orbit + dolly, a sudden zoom
    out that spills, back into the orbit), twice, plus a few static frames."""
    f = [orbit_ubo(k, W, H) for k in range(8)] + [orbit_ubo(8, W, H, radius=20.0)] + \
        [orbit_ubo(k, W, H, radius=20.0 + 3.0 * (k - 8)) for k in range(9, 12)] + [orbit_ubo(k, W, H) for k in (12, 13)]
    return f + f + [orbit_ubo(0, W, H)] * 4


@pytest.mark.parametrize("depth", ["3", "2", "4"])
def test_gaussians_overlapped_frames_equal_serial(native_lib, monkeypatch, depth):
    """PTGS_FLAG_SPLAT_OVERLAP (frames in flight: each call's front end on the context's second stream,
    beside the previous calls' blends, over a ring of workspaces). Every frame of a moving, spilling
    camera sequence, each rendered into its own image without any synchronisation between the calls,
    equals the serial frame bit for bit; nothing is incomplete; the frames ran the fused front end."""
    from pathtracer_gaussiansplatting_amd import Renderer
    monkeypatch.setenv("PTGS_GS_OV_DEPTH", depth)  # (read once per process: the first overlapped context)
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=31)
    frames = _overlap_frames(W, H)
    ra, rb = Renderer(0), Renderer(0)
    try:
        ra.set_splat_overlap(True)
        da = ra.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        db = rb.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        torch.cuda.synchronize()
        outs_a = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in frames]
        outs_b = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in frames]
        for k, ubo in enumerate(frames):
            ra.splat_gaussians(da, ubo, W, H, outs_a[k], bg=(0.1, 0.2, 0.3))
            if k < int(depth):  # (each ring workspace's row size reaches the host: its later frames run fused)
                torch.cuda.synchronize()
        for k, ubo in enumerate(frames):
            rb.splat_gaussians(db, ubo, W, H, outs_b[k], bg=(0.1, 0.2, 0.3))
        torch.cuda.synchronize()
        sa, sb = ra.splat_status(), rb.splat_status()
        assert sa.frames == 0 and sa.incomplete_tiles == 0, (sa.frames, sa.incomplete_tiles)
        assert sa.spilled_tiles > 0, sa.spilled_tiles
        diff = [k for k in range(len(frames)) if not torch.equal(outs_a[k], outs_b[k])]
        assert not diff, f"overlapped frames differ from the serial ones: {diff}"
        # steady state at one view (the zoom frames' large tiles sized some rows past the fused front
        # end's limit, hints the unsynchronised calls above could not see yet): the fused front end
        for _ in range(6):
            ra.splat_gaussians(da, frames[-1], W, H, outs_a[0], bg=(0.1, 0.2, 0.3))
        torch.cuda.synchronize()
        for _ in range(6):
            ra.splat_gaussians(da, frames[-1], W, H, outs_a[0], bg=(0.1, 0.2, 0.3))
        assert ra.splat_status().fused == 1
        assert torch.equal(outs_a[0], outs_b[-1])
    finally:
        ra.close()
        rb.close()


def test_gaussians_overlap_mixed_calls(native_lib, oracle_lib):
    """Overlapped frames interleaved with the calls that run serially on the caller's stream (a frame with
    stats and published buffers, a views call, the flag switched off and on): every image equals its
    serial frame, and the published buffers of the stats frame are the oracle's."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=33)
    ubos = [orbit_ubo(k, W, H) for k in range(10)]
    ra = Renderer(0, publish_splat_buffers=True)
    rb = Renderer(0)
    try:
        ra.set_splat_overlap(True)
        da = {k: _dev(v) for k, v in g.items()}
        db = {k: _dev(v) for k, v in g.items()}
        ref = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in ubos]
        for u, o in zip(ubos, ref):
            rb.splat_gaussians(db, u, W, H, o)
        out = [torch.zeros_like(o) for o in ref]
        for k in range(3):
            ra.splat_gaussians(da, ubos[k], W, H, out[k])
        st = ra.splat_gaussians(da, ubos[3], W, H, out[3], want_stats=True)  # serial, published
        b = ra.splat_buffers()
        oref = oracle_lib.splat_gaussians(g, ubos[3], W, H)
        assert st.num_rendered == oref["K"]
        np.testing.assert_array_equal(_read(ra, b.sorted_keys, oref["K"], np.uint64), oref["keys"])
        np.testing.assert_array_equal(_read(ra, b.tile_ranges, 2 * b.num_tiles, np.uint32), oref["ranges"])
        for k in (4, 5):
            ra.splat_gaussians(da, ubos[k], W, H, out[k])
        ra.splat_gaussians_views(da, [ubos[6], ubos[7]], W, H, [out[6], out[7]])
        ra.set_splat_overlap(False)
        ra.splat_gaussians(da, ubos[8], W, H, out[8])
        ra.set_splat_overlap(True)
        ra.splat_gaussians(da, ubos[9], W, H, out[9])
        torch.cuda.synchronize()
        assert ra.splat_status().frames == 0
        diff = [k for k in range(len(ubos)) if not torch.equal(out[k], ref[k])]
        assert not diff, diff
    finally:
        ra.close()
        rb.close()


def test_gaussians_overlap_runs_and_streams(native_lib):
    """The run rule of PTGS_FLAG_SPLAT_OVERLAP (ptgs.h): within a run the front ends wait on the device for
    the blend ordinals only; a call without the flag ends the run, so Gaussians rewritten on the stream
    before it are seen by the next run; calls that switch streams mid-run fall back to a marker of the new
    stream. Every image equals the serial render of the Gaussians it was called with, bit for bit."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=35)
    g2 = dict(g, colors=(1.0 - g["colors"]).astype(np.float32))  # (the rewritten set: other colours)
    ubos = [orbit_ubo(k, W, H) for k in range(12)]
    ra, rb = Renderer(0), Renderer(0)
    try:
        ra.set_splat_overlap(True)
        da = {k: _dev(v) for k, v in g.items()}
        ref1 = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in ubos]
        ref2 = [torch.zeros_like(o) for o in ref1]
        db1, db2 = {k: _dev(v) for k, v in g.items()}, {k: _dev(v) for k, v in g2.items()}
        for u, o1, o2 in zip(ubos, ref1, ref2):
            rb.splat_gaussians(db1, u, W, H, o1)
            rb.splat_gaussians(db2, u, W, H, o2)
        out = [torch.zeros_like(o) for o in ref1]
        for k in range(5):  # a run on the current stream
            ra.splat_gaussians(da, ubos[k], W, H, out[k])
        # the colours rewritten on the stream, then one call without the flag ends the run
        da["colors"].copy_(torch.from_numpy(g2["colors"]).cuda())
        ra.set_splat_overlap(False)
        ra.splat_gaussians(da, ubos[5], W, H, out[5])
        ra.set_splat_overlap(True)
        side = torch.cuda.Stream()
        for k in range(6, 12):  # a new run; calls 8 and 10 on a side stream (ordered after the others)
            if k in (8, 10):
                side.wait_stream(torch.cuda.current_stream())
                ra.splat_gaussians(da, ubos[k], W, H, out[k], stream=side)
                torch.cuda.current_stream().wait_stream(side)
            else:
                ra.splat_gaussians(da, ubos[k], W, H, out[k])
        torch.cuda.synchronize()
        assert ra.splat_status().frames == 0
        diff = [k for k in range(12) if not torch.equal(out[k], (ref1 if k < 5 else ref2)[k])]
        assert not diff, diff
    finally:
        ra.close()
        rb.close()


def test_gaussians_overlap_rejected_call_keeps_latest_frame(native_lib, oracle_lib, monkeypatch):
    """A call rejected with PTGS_EINVAL inside a run of overlapped calls changes nothing: the ring of
    workspaces does not advance, so ptgs_splat_get_buffers / ptgs_splat_get_tile_rows / last_pairs still
    describe the latest RENDERED frame (its slot rows hold the oracle's pairs of that view, not those of
    the frame ring-depth calls back), and the run goes on: the frames after it equal the serial ones.
    (Ring depth 3, the default: frame 7 is then its workspace's third frame, the first that runs fused.)"""
    from pathtracer_gaussiansplatting_amd import Renderer, PtgsError
    from pathtracer_gaussiansplatting_amd._abi import PTGS_EINVAL
    from test_splat_tight_gpu import _check_timed_rows
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=37)
    ubos = [orbit_ubo(k, W, H) for k in range(12)]
    ref7 = oracle_lib.splat_gaussians(g, ubos[7], W, H, tight=True)
    monkeypatch.setenv("PTGS_GS_OV_DEPTH", "3")  # (read when a context first overlaps)
    r, rb = Renderer(0), Renderer(0)
    try:
        r.set_splat_overlap(True)
        d = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        db = rb.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        torch.cuda.synchronize()
        outs = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in ubos]
        serial = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in ubos]
        for k in range(8):
            r.splat_gaussians(d, ubos[k], W, H, outs[k])
            if k < 4:  # (each ring workspace's row size reaches the host)
                torch.cuda.synchronize()
        with pytest.raises(PtgsError) as ei:
            r.splat_gaussians(d, ubos[8], 0, H, outs[8])  # zero width: rejected before anything is enqueued
        assert ei.value.code == PTGS_EINVAL
        torch.cuda.synchronize()
        assert _check_timed_rows(r, ref7), "frame 7 did not run the fused front end"
        last = r.splat_status().last_pairs
        assert last == ref7["K"], (last, ref7["K"])
        for k in range(8, 12):  # the run goes on, no synchronisation between the calls
            r.splat_gaussians(d, ubos[k], W, H, outs[k])
        for k, u in enumerate(ubos):
            rb.splat_gaussians(db, u, W, H, serial[k])
        torch.cuda.synchronize()
        st = r.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0, (st.frames, st.incomplete_tiles)
        diff = [k for k in range(len(ubos)) if not torch.equal(outs[k], serial[k])]
        assert not diff, f"overlapped frames differ from the serial ones: {diff}"
    finally:
        r.close()
        rb.close()


def test_gaussians_every_workspace_is_reserved_read_and_freed(native_lib, monkeypatch):
    """The three paths that visit every workspace of a context (the ring of PTGS_FLAG_SPLAT_OVERLAP at depth
    4, the view workspaces 1..3): ptgs_splat_reserve grows them all (pair_capacity is the minimum over the
    workspaces, so it reaches the reserved count only if each one was reserved), ptgs_splat_status_read sums
    them all (frames == 0), and ptgs_destroy frees them all (a second context then renders a frame equal to
    the serial one bit for bit)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    monkeypatch.setenv("PTGS_GS_OV_DEPTH", "4")  # (read when a context first overlaps)
    W, H, n = 64, 64, 2000
    g = Y.gaussians_c2(n, seed=39)
    ubos = [orbit_ubo(k, W, H) for k in range(8)]
    dg = {k: _dev(v) for k, v in g.items()}
    rb = Renderer(0)
    try:
        serial = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in ubos]
        for u, o in zip(ubos, serial):
            rb.splat_gaussians(dg, u, W, H, o)
        torch.cuda.synchronize()
    finally:
        rb.close()
    outs = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in ubos]
    views = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(4)]
    r = Renderer(0)
    try:
        r.set_splat_overlap(True)
        for k in range(6):  # every ring workspace has rendered
            r.splat_gaussians(dg, ubos[k], W, H, outs[k])
        r.splat_gaussians_views(dg, ubos[:4], W, H, views)
        torch.cuda.synchronize()
        st = r.splat_status()
        assert st.last_pairs > 0 and st.frames == 0, (st.last_pairs, st.frames)
        P = 4 * int(st.last_pairs)
        r.splat_reserve(P)
        r.splat_gaussians(dg, ubos[6], W, H, outs[6])
        r.splat_gaussians_views(dg, ubos[4:8], W, H, views)
        torch.cuda.synchronize()
        st = r.splat_status()
        assert st.pair_capacity >= P, (st.pair_capacity, P)
        assert st.frames == 0, st.frames
        # (8 pairs per Gaussian, a fresh workspace's buffer, is already above 4 x last_pairs at this size: a
        # second reserve above every workspace's capacity is the one that fails if a workspace is left out)
        P2 = 2 * int(st.pair_capacity) + 1
        r.splat_reserve(P2)
        r.splat_gaussians(dg, ubos[6], W, H, outs[6])
        r.splat_gaussians_views(dg, ubos[4:8], W, H, views)
        torch.cuda.synchronize()
        st = r.splat_status()
        assert st.pair_capacity >= P2, (st.pair_capacity, P2)
        assert st.frames == 0, st.frames
        diff = [k for k in range(7) if not torch.equal(outs[k], serial[k])]
        diff += [4 + v for v in range(4) if not torch.equal(views[v], serial[4 + v])]
        assert not diff, diff
    finally:
        r.close()
    r2 = Renderer(0)
    try:
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        r2.splat_gaussians(dg, ubos[7], W, H, out)
        torch.cuda.synchronize()
        assert torch.equal(out, serial[7])
    finally:
        r2.close()
