"""The histogram windows of the fused splat front end (splat_fused.h gs_bin_fused_kernel, the `kw` loop).
An overlapped frame (PTGS_FLAG_SPLAT_OVERLAP) runs the 256-work-item workgroup shape, whose LDS histogram
holds WINDOW = 2048 tiles: a 256-Gaussian chunk whose bounding tile rect within a band holds more tiles
walks its slice once per window, and each walk counts, reserves and scatters only that window's pairs.
The rest of the suite never leaves the first window (480x270 is 510 tiles; the 1080p overlap test's
Morton-ordered chunks bound ~100 tiles), so the scenes here are rendered in generated order (no ids):
chunks scattered over the whole frame, chunks of large Gaussians (many slices, helper workgroups) and a
few compact ones, at the smallest frame sizes where the window count changes.

test_windows_are_reached proves from the CPU oracle alone (no GPU) that each scene has the chunk rects,
the pairs beyond the first window and the tile sizes its GPU test relies on. The GPU tests compare every
overlapped frame with the oracle's pairs per tile (the frame's own slot rows), with the oracle's image
(1e-4 relative L2, the suite's 3DGS tolerance) and, bit for bit, with the same frame of a serial renderer
(512-work-item shape, whole-band histogram)."""
import numpy as np
import pytest

import scenes_util as U
from pathtracer_gaussiansplatting_amd import Camera, make_ubo
from pathtracer_gaussiansplatting_amd import synthetic as Y

WINDOW = 2048  # GsFusedShape<256>::lds_cap (splat_plan.h; a static_assert there names this file)
SLICE = 2048  # GsFusedShape<256>::slice: pairs per walked slice of a chunk
CHUNK = 256  # GS_FUSED_THREADS: Gaussians per fused workgroup
BAND_TILES = 8192  # GS_BAND_TILES
RUNS_PER_TILE = 32  # GS_FUSED_RUNS_PER_TILE: above it the policy leaves the fused front end
MAX_SCAP = 2048  # GS_FUSED_MAX_SCAP: rows follow the largest tile + 1/4, so tiles <= 1638 stay fused
RING = 4  # PTGS_OV_RING: the most workspaces a ring holds, whatever PTGS_GS_OV_DEPTH says
# A workspace runs fused from its third frame on: the call after its first finished frame sees that frame's
# row size on the host (and still runs three launches), the one after that is fused. So 2 * RING overlapped
# frames, each waited for, leave every ring workspace fused whatever the ring's depth.
PRIME = 2 * RING

SEED = 83  # (a seed whose boundary case has pairs in its 31-tile second window: test_windows_are_reached)
VIEW_C2 = ([0.0, 0.0, 0.0], [0.0, 0.0, -1.0])
VIEW_ORBIT = ([1.0, 0.3, -1.0], [0.0, 0.0, -8.0])

# name: frame, scene, views, and what the oracle must show (test_windows_are_reached): `windows` the
# window count of the widest chunk rect (exact 1 for the control, else at least), `late` the least number
# of pairs at a rect index >= WINDOW, `tile` the (exclusive low, inclusive high) bounds of the largest tile
CASES = {
    # 64x32 = 2048 tiles: every rect fits one window (nt <= kcap on the same code path)
    "control": dict(W=1024, H=512, big=12, nbig=256, views=[VIEW_C2], windows=1, late=0, tile=(0, 204)),
    # 64x33 = 2112 tiles: a second window of a few dozen tiles (the large chunk: ~16k pairs, 8 slices)
    "boundary": dict(W=1024, H=528, big=12, nbig=256, views=[VIEW_C2], windows=2, late=1, tile=(0, 204)),
    # 80x65 = 5200 tiles: three windows for the scattered chunks, three windows x ~26 slices for the large one
    "three": dict(W=1280, H=1040, big=12, nbig=256, views=[VIEW_C2], windows=3, late=1000, tile=(0, 204)),
    # 128x65 = 8320 tiles, two bands (band_rows 64): four windows in band 0, a sliver in band 1
    "two_bands": dict(W=2048, H=1040, big=12, nbig=256, views=[VIEW_C2], windows=4, late=1000, tile=(0, 204)),
    # tile rows [10, 60) of 80x65: gs_bin_fused_kernel<true, 256> (row cull), 4000 tiles in range
    "row_range": dict(W=1280, H=1040, big=12, nbig=256, views=[VIEW_C2], rows=(10, 60), windows=2, late=1000,
                      tile=(0, 204)),
    # consecutive frames with different rects
    "two_views": dict(W=1280, H=1040, big=12, nbig=256, views=[VIEW_C2, VIEW_ORBIT], windows=3, late=1000,
                      tile=(0, 204)),
    # tiles above rows sized from a sparse frame: windowed chunks at the `rel < scap` guard, spill pool
    "row_overflow": dict(W=1024, H=528, big=40, nbig=512, views=[VIEW_C2], windows=2, late=1000,
                         tile=(256, 1638)),
}


def windows_scene(seed, big, nbig):
    """Gaussians in the order they are rendered (no ids; a spatial sort would make every chunk compact).
    Chunks 0-3: small Gaussians scattered over the whole frustum (a rect about the frame, few tiles
    touched). The next nbig / 256 chunks: Gaussians `big` times larger (thousands of pairs per chunk: many
    slices, helpers). The last 3 chunks: small Gaussians sorted coarsely by position (compact rects)."""
    assert nbig % CHUNK == 0
    a = Y.gaussians_c2(4 * CHUNK, seed)
    b = Y.gaussians_c2(nbig, seed + 1)
    b["scales"] = (b["scales"] * np.float32(big)).astype(np.float32)
    c = Y.gaussians_c2(3 * CHUNK, seed + 2)
    m = c["means"]
    cell = np.floor((m[:, 1] + 2.25) / 0.75).astype(np.int64) * 8 + np.floor(m[:, 0] + 4.0).astype(np.int64)
    order = np.argsort(cell, kind="stable")
    c = {k: v[order] for k, v in c.items()}
    return {k: np.ascontiguousarray(np.concatenate([a[k], b[k], c[k]])) for k in a}


def _ubo(case, view):
    eye, at = view
    return make_ubo(Camera(aspect=case["W"] / case["H"]).look_at(eye, at), U.cornell(), 0)


_SCENES, _REFS = {}, {}


def _scene(name):
    case = CASES[name]
    key = (case["big"], case["nbig"])
    if key not in _SCENES:
        _SCENES[key] = windows_scene(SEED, *key)
    return _SCENES[key]


def _ref(oracle_lib, name, v=0):
    """The oracle's tight frame of view v of a case (computed once, shared by the tests, never written)."""
    if (name, v) not in _REFS:
        case = CASES[name]
        _REFS[name, v] = oracle_lib.splat_gaussians(_scene(name), _ubo(case, case["views"][v]), case["W"], case["H"],
                                                    tight=True, tile_rows=case.get("rows"))
    return _REFS[name, v]


def _window_stats(ref, W, H, rows=None):
    """Per (256-Gaussian chunk, band) of the oracle's pairs: the bounding tile rect and each pair's index
    k in it, as gs_bin_fused_kernel lays them out. The pairs are a subset of the rects the kernel bounds,
    so its rects are at least as large."""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    r0, r1 = (0, gy) if rows is None else (min(rows[0], gy), min(rows[1], gy))
    band_rows = max(1, min(r1 - r0, BAND_TILES // gx))
    tile = (ref["keys"].astype(np.uint64) >> np.uint64(32)).astype(np.int64)
    tx, ty = tile % gx, tile // gx
    assert ty.min() >= r0 and ty.max() < r1
    chunk = ref["vals"].astype(np.int64) // CHUNK
    band = (ty - r0) // band_rows
    nb = int(band.max()) + 1
    cb = chunk * nb + band
    n = int(cb.max()) + 1
    big = np.iinfo(np.int64).max
    bx0, by0 = np.full(n, big), np.full(n, big)
    bx1, by1 = np.full(n, -1), np.full(n, -1)
    np.minimum.at(bx0, cb, tx)
    np.minimum.at(by0, cb, ty)
    np.maximum.at(bx1, cb, tx)
    np.maximum.at(by1, cb, ty)
    used = bx1 >= 0
    rw = np.where(used, bx1 - bx0 + 1, 0)
    rh = np.where(used, by1 - by0 + 1, 0)
    k = (ty - by0[cb]) * rw[cb] + (tx - bx0[cb])
    assert (k >= 0).all() and (k < (rw * rh)[cb]).all()
    per_tile = np.diff(ref["ranges"].reshape(-1, 2).astype(np.int64), axis=1).ravel()
    tiles_in_range = (r1 - r0) * gx
    return dict(
        nt=(rw * rh)[used],  # tiles per chunk rect
        windows=-(-(rw * rh)[used] // WINDOW),
        slices=-(-np.bincount(cb, minlength=n)[used] // SLICE),
        late=int((k >= WINDOW).sum()),
        runs=len(np.unique(chunk * (gx * gy) + tile)),
        tiles=tiles_in_range,
        bands=nb,
        largest=int(per_tile.max()),
        above_256=int((per_tile > 256).sum()),
        K=int(ref["K"]),
    )


def test_windows_are_reached(oracle_lib):
    """From the reference alone: every case's chunks bound the stated number of histogram windows, enough
    pairs lie beyond the first window (the pairs a kernel that mishandled later windows would lose or
    misplace), the front-end policy keeps the frame fused (runs per tile), and the largest tile keeps the
    rows at 256 (nothing spills) except in the row-overflow case, which stays under GS_FUSED_MAX_SCAP."""
    print(f"\n{'case':<14}{'view':>5}{'tiles':>7}{'bands':>6}{'K':>9}{'max rect':>9}{'windows':>8}{'slices':>7}"
          f"{'pairs k>=2048':>14}{'runs/tile':>10}{'max tile':>9}{'tiles>256':>10}")
    for name, case in CASES.items():
        for v in range(len(case["views"])):
            s = _window_stats(_ref(oracle_lib, name, v), case["W"], case["H"], case.get("rows"))
            print(f"{name:<14}{v:>5}{s['tiles']:>7}{s['bands']:>6}{s['K']:>9}{int(s['nt'].max()):>9}"
                  f"{int(s['windows'].max()):>8}{int(s['slices'].max()):>7}{s['late']:>14}"
                  f"{s['runs'] / s['tiles']:>10.2f}{s['largest']:>9}{s['above_256']:>10}")
            if case["windows"] == 1:
                assert (s["windows"] == 1).all(), (name, v, s["nt"].max())
            else:
                assert s["windows"].max() >= case["windows"], (name, v, s["nt"].max())
            assert s["late"] >= case["late"], (name, v, s["late"])
            assert s["slices"].max() > 1, (name, v)  # (a chunk of several slices: helpers walk windows too)
            assert s["runs"] <= RUNS_PER_TILE * s["tiles"], (name, v, s["runs"], s["tiles"])
            lo, hi = case["tile"]
            assert lo < s["largest"] <= hi, (name, v, s["largest"])
    assert CASES["row_overflow"]["tile"][1] + CASES["row_overflow"]["tile"][1] // 4 <= MAX_SCAP
    assert _window_stats(_ref(oracle_lib, "two_bands"), 2048, 1040)["bands"] == 2


try:  # (the GPU tests' only; test_windows_are_reached runs without it)
    import torch
except ImportError:
    torch = None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _read(renderer, ptr, n, dtype):
    out = np.zeros(n, dtype)
    if n:
        renderer.copy_d2h(out, ptr, out.nbytes)
    return out


def _check_timed_rows(r, ref, gx, rows=None):
    """test_splat_tight_gpu._check_timed_rows (the frame's OWN pairs, read back from its fused slot rows,
    equal the oracle's per tile as a set; tile t at t * capacity, the counts in the ranges the blend wrote),
    over the frame's tile rows only: a row-restricted frame writes no other tile's range. Returns the row
    capacity (0: the frame ran three launches)."""
    ptr, cap = r.splat_tile_rows()
    if not cap:
        return 0
    b = r.splat_buffers()
    tiles = b.num_tiles
    t0, t1 = (0, tiles) if rows is None else (rows[0] * gx, rows[1] * gx)
    rng = _read(r, b.tile_ranges, 2 * tiles, np.uint32).reshape(tiles, 2).astype(np.int64)[t0:t1]
    cnt = rng[:, 1] - rng[:, 0]
    np.testing.assert_array_equal(rng[:, 0], np.arange(t0, t1, dtype=np.int64) * cap)
    ref_rng = ref["ranges"].reshape(tiles, 2).astype(np.int64)
    assert int(np.diff(ref_rng, axis=1).sum()) == int(np.diff(ref_rng[t0:t1], axis=1).sum()) == ref["K"]
    np.testing.assert_array_equal(cnt, ref_rng[t0:t1, 1] - ref_rng[t0:t1, 0])  # every tile's own pair count
    assert cnt.max() <= cap, (cnt.max(), cap)  # (no tile spilled: its whole row is the frame's)
    slots = _read(r, ptr, tiles * cap, np.uint64).reshape(tiles, cap)[t0:t1]
    got = slots[np.arange(cap)[None, :] < cnt[:, None]]  # tile-major
    got_t = np.repeat(np.arange(t0, t1, dtype=np.uint64), cnt)
    ref_keys = ref["keys"].astype(np.uint64)
    want = ((ref_keys & np.uint64(0xFFFFFFFF)) << np.uint64(32)) | ref["vals"].astype(np.uint64)
    want_t = ref_keys >> np.uint64(32)
    np.testing.assert_array_equal(np.sort(got_t), want_t)
    got = got[np.lexsort((got, got_t))]
    want = want[np.lexsort((want, want_t))]
    np.testing.assert_array_equal(got, want)
    return cap


def _serial_frames(name, dg):
    """Each view's frame from a non-overlapped renderer, three times (three launches twice: a workspace
    runs fused from the call after the one that saw a finished frame's row size; then the fused front end
    in its 512-work-item shape with a whole-band histogram): all must be the same image."""
    from pathtracer_gaussiansplatting_amd import Renderer
    case = CASES[name]
    W, H = case["W"], case["H"]
    r = Renderer(0)
    try:
        outs = []
        for view in case["views"]:
            ubo = _ubo(case, view)
            same = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
            for o in same:
                r.splat_gaussians(dg, ubo, W, H, o, tile_rows=case.get("rows"))
                torch.cuda.synchronize()  # (the row sizes reach the host)
            assert torch.equal(same[0], same[2]) and torch.equal(same[1], same[2])
            outs.append(same[2])
        st = r.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0 and st.fused == 1, (st.frames, st.incomplete_tiles, st.fused)
        return outs
    finally:
        r.close()


def _image_err(case, out, ref):
    gy = (case["H"] + 15) // 16
    r0, r1 = case.get("rows") or (0, gy)
    y0, y1 = r0 * 16, min(r1 * 16, case["H"])
    return U.rel_l2(out[y0:y1].cpu().numpy(), ref["image"][y0:y1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["control", "boundary", "three", "two_bands", "row_range", "two_views"])
def test_windowed_overlapped_frames_vs_oracle(native_lib, oracle_lib, name):
    """Overlapped frames (256-work-item front end, 2048-tile histogram windows) of a scene whose chunk
    rects need the case's window count: each frame's own slot rows hold the oracle's pairs per tile, its
    image equals the serial renderer's bit for bit and the oracle's within 1e-4; nothing spills."""
    from pathtracer_gaussiansplatting_amd import Renderer
    case = CASES[name]
    W, H, rows = case["W"], case["H"], case.get("rows")
    gx = (W + 15) // 16
    views = case["views"]
    refs = [_ref(oracle_lib, name, v) for v in range(len(views))]
    ubos = [_ubo(case, view) for view in views]
    dg = {k: _dev(v) for k, v in _scene(name).items()}
    serial = _serial_frames(name, dg)
    r = Renderer(0)
    try:
        out = torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda")
        r.splat_gaussians(dg, ubos[0], W, H, out, tile_rows=rows)  # (sizes the first workspace's rows)
        torch.cuda.synchronize()
        assert torch.equal(out, serial[0])
        r.set_splat_overlap(True)
        frame = 0
        for _ in range(PRIME):  # every ring workspace's row size reaches the host
            v = frame % len(views)
            out.fill_(-7.0)
            r.splat_gaussians(dg, ubos[v], W, H, out, tile_rows=rows)
            torch.cuda.synchronize()
            assert torch.equal(out, serial[v]), f"frame {frame} (view {v}) != serial"
            frame += 1
        for _ in range(RING + len(views) - 1):  # at least one fused frame per ring slot (and per view on each)
            v = frame % len(views)
            out.fill_(-7.0)
            r.splat_gaussians(dg, ubos[v], W, H, out, tile_rows=rows)
            torch.cuda.synchronize()
            cap = _check_timed_rows(r, refs[v], gx, rows)
            assert cap, f"frame {frame} did not run the fused front end"
            assert torch.equal(out, serial[v]), f"frame {frame} (view {v}) != serial"
            err = _image_err(case, out, refs[v])
            assert err < 1e-4, (frame, v, err)
            frame += 1
        st = r.splat_status()
        assert st.last_pairs == refs[(frame - 1) % len(views)]["K"], st.last_pairs
        assert st.frames == 0 and st.incomplete_tiles == 0 and st.spilled_tiles == 0, \
            (st.frames, st.incomplete_tiles, st.spilled_tiles)
    finally:
        r.close()


@pytest.mark.gpu
def test_windowed_row_overflow_spills_exactly(native_lib, oracle_lib, monkeypatch):
    """Windowed chunks whose tiles outgrow their rows: every ring workspace's rows are sized from sparse
    frames (256 pairs), then dense frames (largest tile > 256) run overlapped. Their windows' scatters stop
    at the row's end and the overflowing tiles complete through the spill pool (the chunk rects the
    front end published): spilled, nothing incomplete, the serial renderer's image bit for bit.
    The ring's depth is pinned to 3 so that each workspace gets exactly two sparse frames, both through
    the three launches, which publish the true largest tile (a fused frame publishes at least 256, and
    the rows after it would be 512: above this scene's tiles)."""
    from pathtracer_gaussiansplatting_amd import Renderer
    name = "row_overflow"
    case = CASES[name]
    W, H = case["W"], case["H"]
    ref = _ref(oracle_lib, name)
    ubo = _ubo(case, case["views"][0])
    dg = {k: _dev(v) for k, v in _scene(name).items()}
    sparse = {k: _dev(v) for k, v in Y.gaussians_c2(500, seed=2).items()}
    serial = _serial_frames(name, dg)[0]
    err = _image_err(case, serial, ref)
    assert err < 1e-4, err
    depth = 3
    monkeypatch.setenv("PTGS_GS_OV_DEPTH", str(depth))  # (read when a context first overlaps)
    r = Renderer(0)
    try:
        r.set_splat_overlap(True)
        tmp = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for _ in range(2 * depth):  # two sparse frames per ring workspace: its third frame runs fused, 256-pair rows
            r.splat_gaussians(sparse, ubo, W, H, tmp)
            torch.cuda.synchronize()
            assert r.splat_tile_rows()[1] == 0  # (three launches)
        st = r.splat_status()
        assert st.frames == 0 and st.spilled_tiles == 0
        outs = [torch.full((H, W, 4), -7.0, dtype=torch.float32, device="cuda") for _ in range(depth)]
        for o in outs:  # (no synchronisation: each workspace's first dense frame meets the sparse frames' rows)
            r.splat_gaussians(dg, ubo, W, H, o)
            # (a host-side query: the frame was enqueued fused, with 256-pair rows)
            assert r.splat_tile_rows()[1] == 256, r.splat_tile_rows()[1]
        st = r.splat_status()
        assert st.frames == 0 and st.incomplete_tiles == 0 and st.spilled_tiles > 0, \
            (st.frames, st.incomplete_tiles, st.spilled_tiles)
        for k, o in enumerate(outs):
            assert torch.equal(o, serial), f"dense frame {k} != serial"
    finally:
        r.close()
