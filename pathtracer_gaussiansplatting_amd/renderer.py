"""Renderer: the device-side API over libptgs.so (the drop-in for the reference's RT pipeline).

Mirrors what Engine does around the hot path (Vulkan_Engine/engine.cpp):
  upload_scene(scene)              createGlobalBindlessBuffers + buildBlas/initStaticTlas
  trace_camera(ubo, accum, spp)    vkCmdTraceRaysKHR(W,H,1) x spp + running mean (:1971, :2684-2708)
  trace_torus(...)                 torus trace (:1893-1900, :2787-2794)
  splat_points(...)                point-cloud draw (:1945-1961)
  splat_gaussians(...)             3DGS forward (absent from the reference)
  encode_srgb8(...)                rgba32f -> sRGB8 blit (:2004-2020)
Device buffers are torch tensors on the context's device (or raw device pointers as ints).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi
from ._abi import (BvhBuffers, Gaussians, RayPush, SceneBuild, SceneInfo, SceneTreeOpt, SplatBuffers, SplatStats,
                   SplatStatus, TraceStats, Ubo)


def _ptr(x) -> int:
    if x is None:
        return 0
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        if not x.is_cuda:
            raise _abi.PtgsError("expected a device tensor (got a host tensor): the renderer has no CPU path")
        if not x.is_contiguous():
            raise _abi.PtgsError("device tensor must be contiguous")
        return x.data_ptr()
    raise TypeError(f"cannot take a device pointer of {type(x)}")


def _gaussians(g: dict) -> Gaussians:
    """ptgs_gaussians of a dict of device tensors (means, scales, rotations, opacities, colors[, ids])."""
    gs = Gaussians()
    gs.means, gs.scales, gs.rotations = _ptr(g["means"]), _ptr(g["scales"]), _ptr(g["rotations"])
    gs.opacities, gs.colors = _ptr(g["opacities"]), _ptr(g["colors"])
    gs.count = int(g["means"].shape[0])
    gs.ids = _ptr(g.get("ids"))
    gs.chunk_bounds = _ptr(g.get("chunk_bounds"))
    return gs


def _stream(stream) -> int:
    if stream is None:
        try:
            import torch
            return torch.cuda.current_stream().cuda_stream
        except Exception:
            return 0
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


class Renderer:
    def __init__(self, device: int = 0, lib_path: str | None = None, publish_splat_buffers: bool = False,
                 wavefront: bool = False):
        """publish_splat_buffers: every synchronised splat (want_stats) also publishes its sorted
        keys / values for splat_buffers() (PTGS_FLAG_SPLAT_PUBLISH); "tight": and bins them like the
        stream-ordered frames (PTGS_FLAG_SPLAT_PUBLISH_TIGHT, parity tests of the timed path); wavefront:
        trace_camera runs the wavefront path tracer (PTGS_FLAG_PT_WAVEFRONT). All are kept across set_flags."""
        self.lib = _abi.load_library(lib_path)
        self._publish = _abi.FLAG_PT_WAVEFRONT if wavefront else 0
        if publish_splat_buffers:
            self._publish |= _abi.FLAG_SPLAT_PUBLISH
        if publish_splat_buffers == "tight":
            self._publish |= _abi.FLAG_SPLAT_PUBLISH_TIGHT
        h = C.c_void_p()
        rc = self.lib.ptgs_create(int(device), C.byref(h))
        _abi.check(rc, f"ptgs_create(device={device})")
        self._h = h
        self.device = device
        self.scene = None
        self.set_flags(0)

    def close(self):
        if getattr(self, "_h", None):
            self.lib.ptgs_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self) -> str:
        return (self.lib.ptgs_last_error(self._h) or b"").decode()

    def _chk(self, rc: int, what: str):
        _abi.check(rc, what, self._err())

    # ---------------------------------------------------------------- scene
    def upload_scene(self, scene) -> SceneInfo:
        d = scene.desc()
        self._chk(self.lib.ptgs_scene_upload(self._h, C.byref(d)), "ptgs_scene_upload")
        self.scene = scene
        return self.scene_info()

    def scene_info(self) -> SceneInfo:
        info = SceneInfo()
        self._chk(self.lib.ptgs_scene_get_info(self._h, C.byref(info)), "ptgs_scene_get_info")
        return info

    def scene_build(self) -> SceneBuild:
        """Which builder produced the resident tree (host SAH / GPU SAH / GPU LBVH) and the
        (leaf, fan, depth budget) try that was kept: a flagged upload may have fallen back."""
        b = SceneBuild()
        self._chk(self.lib.ptgs_scene_get_build(self._h, C.byref(b)), "ptgs_scene_get_build")
        return b

    def scene_tree_opt(self) -> SceneTreeOpt:
        """The megakernel's traversal copy of the resident tree: reinsertion-optimised (applied = 1) or the
        canonical tree's conversion, with its node count, stack need, depth, area sums and host time."""
        t = SceneTreeOpt()
        self._chk(self.lib.ptgs_scene_get_tree_opt(self._h, C.byref(t)), "ptgs_scene_get_tree_opt")
        return t

    def scene_pt_stack(self) -> tuple:
        """(LDS depth, walked need, deep) of the megakernel for the resident scene: the stack entries it keeps in
        LDS per lane, the worst-case need of the copy it walks, and whether the instantiation with the private
        overflow is launched (walked need >= LDS depth)."""
        lds, need, deep = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.lib.ptgs_scene_get_pt_stack(self._h, C.byref(lds), C.byref(need), C.byref(deep)),
                  "ptgs_scene_get_pt_stack")
        return lds.value, need.value, bool(deep.value)

    # ---------------------------------------------------------------- path tracer
    def trace_camera(self, ubo: Ubo, width: int, height: int, accum, spp: int = 1, frame_stride: int = 1,
                     mode: int = _abi.ACCUM_RUNNING_MEAN, rows: tuple | None = None, stream=None):
        if rows is None:
            rc = self.lib.ptgs_trace_camera(self._h, C.byref(ubo), width, height, _ptr(accum), spp, frame_stride,
                                            mode, _stream(stream))
        else:
            rc = self.lib.ptgs_trace_camera_rows(self._h, C.byref(ubo), width, height, rows[0], rows[1],
                                                 _ptr(accum), spp, frame_stride, mode, _stream(stream))
        self._chk(rc, "ptgs_trace_camera")

    def trace_torus(self, ubo: Ubo, push: RayPush, samples, n: int, hits, stream=None):
        rc = self.lib.ptgs_trace_torus(self._h, C.byref(ubo), C.byref(push), _ptr(samples), n, _ptr(hits),
                                       _stream(stream))
        self._chk(rc, "ptgs_trace_torus")

    def trace_depth(self, ubo: Ubo, width: int, height: int, depth, stream=None, rows=None):
        """Primary-hit view depth per pixel (+inf on a miss) into a device float[H, W] tensor; rows =
        (begin, end) pixel rows traces only those (ptgs_trace_depth_rows)."""
        if rows is not None:
            rc = self.lib.ptgs_trace_depth_rows(self._h, C.byref(ubo), width, height, int(rows[0]), int(rows[1]),
                                                _ptr(depth), _stream(stream))
            self._chk(rc, "ptgs_trace_depth_rows")
            return
        rc = self.lib.ptgs_trace_depth(self._h, C.byref(ubo), width, height, _ptr(depth), _stream(stream))
        self._chk(rc, "ptgs_trace_depth")

    # ---------------------------------------------------------------- 3DGS initialisation (§8f #3)
    def knn3_mean_dist2(self, xyz, dist2, stream=None):
        """dist2[i] = mean squared distance of point i to its 3 nearest other points (device tensors:
        xyz float32 [N, 3], dist2 float32 [N])."""
        n = int(xyz.shape[0])
        self._chk(self.lib.ptgs_knn3_mean_dist2(self._h, _ptr(xyz), n, _ptr(dist2), _stream(stream)),
                  "ptgs_knn3_mean_dist2")

    def gaussians_from_points(self, xyz, rgb=None, stream=None) -> dict:
        """Kerbl et al. create_from_pcd in post-activation form -> dict of device tensors in the
        splat_gaussians layout (means, scales, rotations, opacities, colors)."""
        import torch
        n = int(xyz.shape[0])
        dev = xyz.device
        g = {"means": torch.empty((n, 3), dtype=torch.float32, device=dev),
             "scales": torch.empty((n, 3), dtype=torch.float32, device=dev),
             "rotations": torch.empty((n, 4), dtype=torch.float32, device=dev),
             "opacities": torch.empty((n,), dtype=torch.float32, device=dev),
             "colors": torch.empty((n, 3), dtype=torch.float32, device=dev)}
        rc = self.lib.ptgs_gaussians_from_points(self._h, _ptr(xyz), _ptr(rgb), n, _ptr(g["means"]), _ptr(g["scales"]),
                                                 _ptr(g["rotations"]), _ptr(g["opacities"]), _ptr(g["colors"]),
                                                 _stream(stream))
        self._chk(rc, "ptgs_gaussians_from_points")
        return g

    # ---------------------------------------------------------------- RCCL frame reduce (§8e)
    def comm_unique_id(self) -> bytes:
        buf = (C.c_uint8 * 128)()
        self._chk(self.lib.ptgs_comm_unique_id(buf), "ptgs_comm_unique_id")
        return bytes(buf)

    def comm_create(self, unique_id: bytes, nranks: int, rank: int):
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._chk(self.lib.ptgs_comm_create(self._h, buf, nranks, rank), "ptgs_comm_create")
        self.comm_world = nranks

    def comm_destroy(self):
        self._chk(self.lib.ptgs_comm_destroy(self._h), "ptgs_comm_destroy")
        self.comm_world = 0

    def reduce_radiance(self, accum, root: int = 0, stream=None):
        rc = self.lib.ptgs_reduce_radiance(self._h, _ptr(accum), accum.numel(), root, _stream(stream))
        self._chk(rc, "ptgs_reduce_radiance")

    def allreduce_radiance(self, accum, stream=None):
        rc = self.lib.ptgs_allreduce_radiance(self._h, _ptr(accum), accum.numel(), _stream(stream))
        self._chk(rc, "ptgs_allreduce_radiance")

    def gather_rows(self, image, row_ranges, root: int = 0, stream=None):
        """Every rank's pixel rows [r0, r1) of the (H, W, 4) float32 image to root (ptgs_gather_rows);
        row_ranges: one (r0, r1) per rank, identical on every rank."""
        H, W = int(image.shape[0]), int(image.shape[1])
        world = getattr(self, "comm_world", 0)
        if len(row_ranges) != world:  # the library reads 2 x nranks entries
            raise ValueError(f"gather_rows needs one (r0, r1) per rank: {len(row_ranges)} given, world {world}")
        rr = np.asarray(row_ranges, np.uint32).reshape(-1)
        if rr.size != 2 * world:
            raise ValueError("gather_rows: every row range is a (r0, r1) pair")
        rc = self.lib.ptgs_gather_rows(self._h, _ptr(image), W, H, rr.ctypes.data, root, _stream(stream))
        self._chk(rc, "ptgs_gather_rows")

    def reduce_scatter_rows(self, image, row_ranges, stream=None):
        """ptgs_reduce_scatter_rows: afterwards this rank's pixel rows of the (H, W, 4) float32 image hold
        the SUM over the ranks of those rows; row_ranges: one (r0, r1) per rank, identical everywhere."""
        H, W = int(image.shape[0]), int(image.shape[1])
        world = getattr(self, "comm_world", 0)
        if len(row_ranges) != world:
            raise ValueError(f"reduce_scatter_rows needs one (r0, r1) per rank: {len(row_ranges)} given, world {world}")
        rr = np.asarray(row_ranges, np.uint32).reshape(-1)
        if rr.size != 2 * world:
            raise ValueError("reduce_scatter_rows: every row range is a (r0, r1) pair")
        rc = self.lib.ptgs_reduce_scatter_rows(self._h, _ptr(image), W, H, rr.ctypes.data, _stream(stream))
        self._chk(rc, "ptgs_reduce_scatter_rows")

    def set_flags(self, flags: int):
        self._flags = flags
        self._chk(self.lib.ptgs_set_flags(self._h, flags | self._publish), "ptgs_set_flags")

    def set_wavefront(self, on: bool):
        """Select the path tracer of trace_camera: wavefront stages (True) or the one-kernel path loop."""
        self._publish = (self._publish & ~_abi.FLAG_PT_WAVEFRONT) | (_abi.FLAG_PT_WAVEFRONT if on else 0)
        self.set_flags(getattr(self, "_flags", 0))

    def set_splat_overlap(self, on: bool):
        """Frames in flight for splat_gaussians (PTGS_FLAG_SPLAT_OVERLAP): the front end of each
        stream-ordered call runs on a second stream while the previous call's blend runs on the caller's.
        The Gaussians must not be rewritten on the stream between two such calls (see ptgs.h)."""
        self._publish = (self._publish & ~_abi.FLAG_SPLAT_OVERLAP) | (_abi.FLAG_SPLAT_OVERLAP if on else 0)
        self.set_flags(getattr(self, "_flags", 0))

    def stats_reset(self, stream=None):
        self._chk(self.lib.ptgs_stats_reset(self._h, _stream(stream)), "ptgs_stats_reset")

    def stats(self) -> TraceStats:
        s = TraceStats()
        self._chk(self.lib.ptgs_stats_read(self._h, C.byref(s)), "ptgs_stats_read")
        return s

    # ---------------------------------------------------------------- rasterizers
    def splat_points(self, ubo: Ubo, push: RayPush, hits, samples, n: int, width: int, height: int, rgba8, depth,
                     stream=None):
        rc = self.lib.ptgs_splat_points(self._h, C.byref(ubo), C.byref(push), _ptr(hits), _ptr(samples), n, width,
                                        height, _ptr(rgba8), _ptr(depth), _stream(stream))
        self._chk(rc, "ptgs_splat_points")

    def splat_gaussians(self, g: dict, ubo: Ubo, width: int, height: int, out, bg=(0.0, 0.0, 0.0),
                        tile_rows: tuple | None = None, want_stats: bool = False, stream=None, over=None):
        """over=(depth, under): the hybrid composite of ptgs_splat_gaussians_over (device depth[H, W],
        under RGBA32F[H, W, 4]; out may be under itself)."""
        gs = _gaussians(g)
        bgc = np.asarray(bg, np.float32)
        t0, t1 = (0, 0xFFFFFFFF) if tile_rows is None else tile_rows
        st = SplatStats()
        if over is not None:
            rc = self.lib.ptgs_splat_gaussians_over(self._h, C.byref(gs), C.byref(ubo), width, height, _ptr(over[0]),
                                                    _ptr(over[1]), t0, t1, _ptr(out),
                                                    C.byref(st) if want_stats else None, _stream(stream))
            self._chk(rc, "ptgs_splat_gaussians_over")
            return st if want_stats else None
        rc = self.lib.ptgs_splat_gaussians(self._h, C.byref(gs), C.byref(ubo), width, height, _abi.fptr(bgc), t0,
                                           t1, _ptr(out), C.byref(st) if want_stats else None, _stream(stream))
        self._chk(rc, "ptgs_splat_gaussians")
        return st if want_stats else None

    def splat_gaussians_invdepth(self, width: int, height: int, out=None, stream=None):
        """ptgs_splat_gaussians_invdepth: the expected inverse depth sum(alpha T / d) per pixel of the latest
        frame (no background term), float32 [H, W] (`out`, or a new device tensor). The frame must be what
        splat_gaussians_backward accepts (full-frame, published, want_stats=True, this size); it stays valid, so
        the call can sit between the forward and the backward. Stream-ordered; reproducible (no atomics)."""
        import torch
        if out is None:
            out = torch.empty((height, width), dtype=torch.float32, device=f"cuda:{torch.cuda.current_device()}")
        self._f32(("out", out, width * height))
        rc = self.lib.ptgs_splat_gaussians_invdepth(self._h, width, height, _ptr(out), _stream(stream))
        self._chk(rc, "ptgs_splat_gaussians_invdepth")
        return out

    def splat_gaussians_backward(self, g: dict, ubo: Ubo, width: int, height: int, dL_dout, bg=(0.0, 0.0, 0.0),
                                 want_means2d: bool = False, want_conics: bool = False, stream=None,
                                 dL_dinvdepth=None, want_view: bool = False) -> dict:
        """ptgs_splat_gaussians_backward: the gradients of the latest frame, which must be a full-frame
        splat_gaussians(g, ubo, width, height, ..., bg, want_stats=True) of a renderer that publishes
        (FLAG_SPLAT_PUBLISH). dL_dout: float32 [H, W, 4]. Returns new tensors "means", "scales" (linear),
        "rotations" (un-normalised), "opacities", "colors" and, when asked for, "means2d" (dL/d pixel
        position) and "conics" (dL/d conic a, b, c). Stream-ordered; not bit-reproducible (float atomics).
        dL_dinvdepth: float32 [H, W], the gradient with respect to splat_gaussians_invdepth's output; with it the
        call is ptgs_splat_gaussians_backward_depth (the gradients of a loss on both, in one pass).
        want_view: the call is ptgs_splat_gaussians_backward_pose (with or without dL_dinvdepth) and the result
        gains "view", a float32 device tensor [4, 4] with G[r][c] = dL/d view[r][c] in math indexing (the
        transpose of the call's column-major 16 floats); row 3 is exactly 0."""
        import torch
        n = int(g["means"].shape[0])
        self._f32(("means", g["means"], n * 3), ("scales", g["scales"], n * 3), ("rotations", g["rotations"], n * 4),
                  ("opacities", g["opacities"], n), ("colors", g["colors"], n * 3),
                  ("dL_dout", dL_dout, width * height * 4),
                  *([("dL_dinvdepth", dL_dinvdepth, width * height)] if dL_dinvdepth is not None else []))
        dev = g["means"].device
        shapes = {"means": (n, 3), "scales": (n, 3), "rotations": (n, 4), "opacities": (n,), "colors": (n, 3)}
        if want_means2d:
            shapes["means2d"] = (n, 2)
        if want_conics:
            shapes["conics"] = (n, 3)
        out = {k: torch.empty(s, dtype=torch.float32, device=dev) for k, s in shapes.items()}
        gr = _abi.GaussianGrads()
        for k, t in out.items():
            setattr(gr, k, _ptr(t))
        bgc = np.asarray(bg, np.float32)
        if want_view:
            raw = torch.empty(16, dtype=torch.float32, device=dev)
            rc = self.lib.ptgs_splat_gaussians_backward_pose(self._h, C.byref(_gaussians(g)), C.byref(ubo), width,
                                                             height, _abi.fptr(bgc), _ptr(dL_dout),
                                                             _ptr(dL_dinvdepth) or None, C.byref(gr), _ptr(raw),
                                                             _stream(stream))
            self._chk(rc, "ptgs_splat_gaussians_backward_pose")
            out["view"] = raw.view(4, 4).t()
            return out
        if dL_dinvdepth is not None:
            rc = self.lib.ptgs_splat_gaussians_backward_depth(self._h, C.byref(_gaussians(g)), C.byref(ubo), width,
                                                              height, _abi.fptr(bgc), _ptr(dL_dout),
                                                              _ptr(dL_dinvdepth), C.byref(gr), _stream(stream))
            self._chk(rc, "ptgs_splat_gaussians_backward_depth")
            return out
        rc = self.lib.ptgs_splat_gaussians_backward(self._h, C.byref(_gaussians(g)), C.byref(ubo), width, height,
                                                    _abi.fptr(bgc), _ptr(dL_dout), C.byref(gr), _stream(stream))
        self._chk(rc, "ptgs_splat_gaussians_backward")
        return out

    def splat_gaussians_views(self, g: dict, ubos, width: int, height: int, outs, bg=(0.0, 0.0, 0.0), stream=None):
        """ptgs_splat_gaussians_views: len(ubos) views of the same Gaussians in one stream-ordered call
        (outs: one RGBA32F[H, W, 4] device tensor per view)."""
        n = len(ubos)
        if len(outs) != n:
            raise ValueError("one output per view")
        gs = _gaussians(g)
        bgc = np.asarray(bg, np.float32)
        arr = (Ubo * n)(*ubos)
        optrs = (C.c_void_p * n)(*[_ptr(o) for o in outs])
        rc = self.lib.ptgs_splat_gaussians_views(self._h, C.byref(gs), n, arr, width, height, _abi.fptr(bgc), optrs,
                                                 _stream(stream))
        self._chk(rc, "ptgs_splat_gaussians_views")

    def sort_gaussians_spatial(self, g: dict, stream=None) -> dict:
        """ptgs_gaussians_sort_spatial: a copy of the device Gaussians `g` in 3D Morton order of the means
        plus "ids" (int32 tensor: the original index of each copy); splatting the copy renders exactly like
        `g` (scene preparation: synchronises)."""
        import torch
        out = {k: torch.empty_like(g[k]) for k in ("means", "scales", "rotations", "opacities", "colors")}
        n = int(g["means"].shape[0])
        out["ids"] = torch.empty(n, dtype=torch.int32, device=g["means"].device)
        rc = self.lib.ptgs_gaussians_sort_spatial(self._h, C.byref(_gaussians(g)), _ptr(out["means"]), _ptr(out["scales"]),
                                                  _ptr(out["rotations"]), _ptr(out["opacities"]), _ptr(out["colors"]),
                                                  _ptr(out["ids"]), _stream(stream))
        self._chk(rc, "ptgs_gaussians_sort_spatial")
        return out

    def gaussians_chunk_bounds(self, g: dict, stream=None):
        """ptgs_gaussians_chunk_bounds: per chunk of 256 Gaussians the box of the means and the largest
        scale (float32 tensor [chunks, 8]); put it in g["chunk_bounds"] so that tile-row-restricted
        frames skip the chunks that cannot reach their rows."""
        import torch
        n = int(g["means"].shape[0])
        out = torch.empty((max(1, (n + 255) // 256), 8), dtype=torch.float32, device=g["means"].device)
        self._chk(self.lib.ptgs_gaussians_chunk_bounds(self._h, C.byref(_gaussians(g)), _ptr(out), _stream(stream)),
                  "ptgs_gaussians_chunk_bounds")
        return out

    # ---------------------------------------------------------------- trained 3DGS checkpoints
    @staticmethod
    def _sh_degree(sh) -> int:
        k = int(sh.shape[1]) if sh.dim() == 3 else 0
        if sh.dim() != 3 or int(sh.shape[2]) != 3 or k not in (1, 4, 9, 16):
            raise _abi.PtgsError(f"sh must be [N, (d+1)^2, 3] with d in 0..3 (got {tuple(sh.shape)})")
        return (1, 4, 9, 16).index(k)

    @staticmethod
    def _f32(*named):
        """Every (name, tensor, elements) is a float32 tensor of exactly that many elements (the kernels
        index by the count alone)."""
        import torch
        for name, t, numel in named:
            if t.dtype != torch.float32 or t.numel() != numel:
                raise _abi.PtgsError(f"{name} must be float32 with {numel} elements (got {t.dtype}, {t.numel()})")

    def sh_colors(self, means, sh, camera_pos, out=None, active_degree=None, stream=None):
        """ptgs_gaussians_sh_colors: linear RGB [N, 3] of SH coefficients sh [N, (d+1)^2, 3] seen from
        camera_pos (max(SH(dir) + 0.5, 0)); active_degree (default: the stored degree d) bands are
        evaluated. Stream-ordered; writes `out` (allocated when None) and returns it."""
        import torch
        d = self._sh_degree(sh)
        n = int(means.shape[0])
        if out is None:
            out = torch.empty((n, 3), dtype=torch.float32, device=means.device)
        self._f32(("means", means, n * 3), ("sh", sh, n * (d + 1) ** 2 * 3), ("out", out, n * 3))
        cam = np.ascontiguousarray(np.asarray(camera_pos, np.float32).reshape(3))
        rc = self.lib.ptgs_gaussians_sh_colors(self._h, _ptr(means), _ptr(sh), n, d,
                                               d if active_degree is None else int(active_degree), _abi.fptr(cam),
                                               _ptr(out), _stream(stream))
        self._chk(rc, "ptgs_gaussians_sh_colors")
        return out

    def activate_gaussians(self, log_scales, opacity_logits, stream=None, out=None):
        """ptgs_gaussians_activate: (scales, opacities) = (exp(log_scales), sigmoid(opacity_logits)) of a
        checkpoint's stored values, as new tensors; out=(scales, opacities) writes there instead (the
        inputs themselves: in place)."""
        import torch
        n = int(opacity_logits.shape[0])
        sc, op = out if out is not None else (torch.empty_like(log_scales), torch.empty_like(opacity_logits))
        self._f32(("log_scales", log_scales, n * 3), ("opacity_logits", opacity_logits, n), ("scales", sc, n * 3),
                  ("opacities", op, n))
        rc = self.lib.ptgs_gaussians_activate(self._h, _ptr(log_scales), _ptr(opacity_logits), n, _ptr(sc), _ptr(op),
                                              _stream(stream))
        self._chk(rc, "ptgs_gaussians_activate")
        return sc, op

    def sh_colors_backward(self, means, sh, camera_pos, dL_dcolors, active_degree=None, dL_dmeans=None, stream=None,
                           want_means: bool = True, want_eye: bool = False):
        """ptgs_gaussians_sh_colors_backward: (dL_dsh, dL_dmeans) of sh_colors(means, sh, camera_pos,
        active_degree=...) given dL_dcolors [N, 3]. dL_dsh is a new tensor shaped like sh; the colour's
        dependence on the means (through the view direction) is ADDED to dL_dmeans [N, 3] (a zero tensor is
        allocated when None) and that tensor is returned: pass the "means" of splat_gaussians_backward.
        want_means=False skips that part (NULL at the C level) and returns (dL_dsh, None).
        want_eye=True: the call is ptgs_gaussians_sh_colors_backward_eye and the result is (dL_dsh, dL_dmeans,
        dL_deye), dL_deye a float32 device tensor [3]: the gradient with respect to camera_pos.
        Stream-ordered; reproducible from run to run (no atomics)."""
        import torch
        d = self._sh_degree(sh)
        n = int(means.shape[0])
        if not want_means:
            dL_dmeans = None
        elif dL_dmeans is None:
            dL_dmeans = torch.zeros((n, 3), dtype=torch.float32, device=means.device)
        self._f32(("means", means, n * 3), ("sh", sh, n * (d + 1) ** 2 * 3), ("dL_dcolors", dL_dcolors, n * 3),
                  *([("dL_dmeans", dL_dmeans, n * 3)] if want_means else []))
        dL_dsh = torch.empty((n, (d + 1) ** 2, 3), dtype=torch.float32, device=means.device)
        cam = np.ascontiguousarray(np.asarray(camera_pos, np.float32).reshape(3))
        if want_eye:
            dL_deye = torch.empty(3, dtype=torch.float32, device=means.device)
            rc = self.lib.ptgs_gaussians_sh_colors_backward_eye(self._h, _ptr(means), _ptr(sh), n, d,
                                                                d if active_degree is None else int(active_degree),
                                                                _abi.fptr(cam), _ptr(dL_dcolors), _ptr(dL_dsh),
                                                                _ptr(dL_dmeans) if want_means else None,
                                                                _ptr(dL_deye), _stream(stream))
            self._chk(rc, "ptgs_gaussians_sh_colors_backward_eye")
            return dL_dsh, dL_dmeans, dL_deye
        rc = self.lib.ptgs_gaussians_sh_colors_backward(self._h, _ptr(means), _ptr(sh), n, d,
                                                        d if active_degree is None else int(active_degree),
                                                        _abi.fptr(cam), _ptr(dL_dcolors), _ptr(dL_dsh),
                                                        _ptr(dL_dmeans) if want_means else None, _stream(stream))
        self._chk(rc, "ptgs_gaussians_sh_colors_backward")
        return dL_dsh, dL_dmeans

    def activate_gaussians_backward(self, scales, opacities, dL_dscales, dL_dopacities, out=None, stream=None):
        """ptgs_gaussians_activate_backward: (dL_dlog_scales, dL_dlogits) from the ACTIVATED scales and
        opacities (activate_gaussians' outputs) and the gradients with respect to them, as new tensors;
        out=(dL_dlog_scales, dL_dlogits) writes there instead (the upstream gradients themselves: in place)."""
        import torch
        n = int(opacities.shape[0])
        ds, do = out if out is not None else (torch.empty_like(dL_dscales), torch.empty_like(dL_dopacities))
        self._f32(("scales", scales, n * 3), ("opacities", opacities, n), ("dL_dscales", dL_dscales, n * 3),
                  ("dL_dopacities", dL_dopacities, n), ("dL_dlog_scales", ds, n * 3), ("dL_dlogits", do, n))
        rc = self.lib.ptgs_gaussians_activate_backward(self._h, _ptr(scales), _ptr(opacities), n, _ptr(dL_dscales),
                                                       _ptr(dL_dopacities), _ptr(ds), _ptr(do), _stream(stream))
        self._chk(rc, "ptgs_gaussians_activate_backward")
        return ds, do

    # ---------------------------------------------------------------- training loss
    def l1_dssim_loss(self, image, target, lam: float = 0.2, grad_out=None, grad_scale: float = 1.0, terms_out=None,
                      stream=None):
        """ptgs_image_loss_l1_dssim: the 3DGS training loss (1 - lam) * mean|image - target| + lam * (1 - SSIM)
        of a rendered RGBA32F frame image [H, W, 4] against target [H, W, 3 or 4] (contiguous float32 device
        tensors, values in roughly [0, 1]; channels 0..2 take part). Returns (terms, grad): terms is a float32
        device tensor [4] = (loss, l1, ssim, 0) (terms_out, or a new one) that is never read back here; grad is
        grad_out, a float32 [H, W, 4] device tensor that receives grad_scale * dloss/dimage (alpha 0, every
        element overwritten), or None when grad_out is None: only the terms are computed. Stream-ordered, no
        host wait; reproducible from run to run (no atomics). A training loop that wants no torch arithmetic
        calls this and then img.backward(grad)."""
        import torch
        if image.dim() != 3 or int(image.shape[2]) != 4:
            raise _abi.PtgsError(f"image must be [H, W, 4] (got {tuple(image.shape)})")
        h, w = int(image.shape[0]), int(image.shape[1])
        c = int(target.shape[2]) if target.dim() == 3 else 0
        if c not in (3, 4) or tuple(target.shape[:2]) != (h, w):
            raise _abi.PtgsError(f"target must be [{h}, {w}, 3 or 4] (got {tuple(target.shape)})")
        if terms_out is None:
            terms_out = torch.empty(4, dtype=torch.float32, device=image.device)
        self._f32(("image", image, h * w * 4), ("target", target, h * w * c), ("terms_out", terms_out, 4),
                  *([("grad_out", grad_out, h * w * 4)] if grad_out is not None else []))
        rc = self.lib.ptgs_image_loss_l1_dssim(self._h, _ptr(image), _ptr(target), c, w, h, float(lam),
                                               float(grad_scale), _ptr(terms_out), _ptr(grad_out) or None,
                                               _stream(stream))
        self._chk(rc, "ptgs_image_loss_l1_dssim")
        return terms_out, grad_out

    def invdepth_l1_loss(self, invdepth, target_depth, weight: float = 1.0, grad_out=None, grad_scale: float = 1.0,
                         terms_out=None, stream=None):
        """ptgs_image_loss_invdepth_l1: the L1 between a rendered inverse depth [H, W] (splat_gaussians_invdepth)
        and a VIEW DEPTH target [H, W] (trace_depth's output: +inf where nothing was hit). A pixel is supervised
        when its target is > 0 (+inf: target inverse depth 0); others (<= 0, NaN) add nothing and get gradient 0.
        Returns (terms, grad): terms a float32 device tensor [4] = (weight * mean, mean, supervised pixels, 0), the
        mean over all H W pixels, never read back here; grad is grad_out, float32 [H, W], which receives
        grad_scale * weight / (H W) * sign(invdepth - 1 / target), or None when grad_out is None. Stream-ordered,
        no host wait; reproducible (no atomics)."""
        import torch
        if invdepth.dim() != 2 or tuple(target_depth.shape) != tuple(invdepth.shape):
            raise _abi.PtgsError(f"invdepth and target_depth must both be [H, W] (got {tuple(invdepth.shape)}, "
                                 f"{tuple(target_depth.shape)})")
        h, w = int(invdepth.shape[0]), int(invdepth.shape[1])
        if terms_out is None:
            terms_out = torch.empty(4, dtype=torch.float32, device=invdepth.device)
        self._f32(("invdepth", invdepth, h * w), ("target_depth", target_depth, h * w), ("terms_out", terms_out, 4),
                  *([("grad_out", grad_out, h * w)] if grad_out is not None else []))
        rc = self.lib.ptgs_image_loss_invdepth_l1(self._h, _ptr(invdepth), _ptr(target_depth), w, h, float(weight),
                                                  float(grad_scale), _ptr(terms_out), _ptr(grad_out) or None,
                                                  _stream(stream))
        self._chk(rc, "ptgs_image_loss_invdepth_l1")
        return terms_out, grad_out

    # ---------------------------------------------------------------- densification and pruning
    def densify_accumulate(self, means2d_grad, width: int, height: int, accum, denom, max_radii, radii=None,
                           stream=None):
        """ptgs_densify_accumulate: one training view's densification statistic. means2d_grad [N, 2] is
        dL/d(pixel position) of the backward just run (splat_sh(..., means2d_grad=)); radii (int32 [N]) default
        to the published frame's own (the latest splat of this renderer, which must have N Gaussians). Visible
        Gaussians (radius > 0) add the NDC-scaled gradient norm to accum, 1 to denom and raise max_radii
        (float32 [N] each, updated in place). Stream-ordered; reproducible (no atomics)."""
        import torch
        n = int(means2d_grad.shape[0])
        self._f32(("means2d_grad", means2d_grad, n * 2), ("accum", accum, n), ("denom", denom, n),
                  ("max_radii", max_radii, n))
        if radii is None:
            b = self.splat_buffers()
            if b.num_gaussians != n or (n and not b.radii):
                raise _abi.PtgsError(f"the published frame has {b.num_gaussians} gaussians, the statistic {n}: "
                                     "densify_accumulate follows a published splat of the same Gaussians")
            rp = b.radii or 0
        else:
            if radii.dtype != torch.int32 or radii.numel() != n:
                raise _abi.PtgsError(f"radii must be int32 with {n} elements (got {radii.dtype}, {radii.numel()})")
            rp = _ptr(radii)
        rc = self.lib.ptgs_densify_accumulate(self._h, _ptr(means2d_grad), rp, n, int(width), int(height), _ptr(accum),
                                              _ptr(denom), _ptr(max_radii), _stream(stream))
        self._chk(rc, "ptgs_densify_accumulate")

    def densify_plan(self, scales, opacities, accum, denom, max_radii, *, grad_threshold: float, scale_split: float,
                     min_opacity: float, max_scale: float = 0.0, max_screen_radius: float = 0.0,
                     stream=None) -> _abi.DensifyCounts:
        """ptgs_gaussians_densify_plan: decide clone / split / prune for every Gaussian from its ACTIVATED scales
        [N, 3] and opacities [N] and the accumulated statistic, and leave the source map of the new set in the
        context for densify_apply. Waits for the stream; returns the counts (.total = the new N)."""
        n = int(opacities.shape[0])
        self._f32(("scales", scales, n * 3), ("opacities", opacities, n), ("accum", accum, n), ("denom", denom, n),
                  ("max_radii", max_radii, n))
        p = _abi.DensifyParams(float(grad_threshold), float(scale_split), float(min_opacity), float(max_scale),
                               float(max_screen_radius))
        out = _abi.DensifyCounts()
        rc = self.lib.ptgs_gaussians_densify_plan(self._h, _ptr(scales), _ptr(opacities), _ptr(accum), _ptr(denom),
                                                  _ptr(max_radii), n, C.byref(p), C.byref(out), _stream(stream))
        self._chk(rc, "ptgs_gaussians_densify_plan")
        return out

    def densify_apply(self, n_out: int, means, log_scales, rotations, scales, noise, rows=(), want_source=False,
                      stream=None):
        """ptgs_gaussians_densify_apply: the new arrays of the latest densify_plan (n_out = its .total).
        rotations [N, 4] and the ACTIVATED scales [N, 3] place the split children with noise (float32 [2, N, 3]
        standard-normal draws). rows: (tensor [N, ...], zero_new) pairs, every other per-Gaussian array
        (rotations, logits, SH, optimizer moments; zero_new: clones and children get zeros), at most 16.
        Returns (means_out, log_scales_out, [row outputs, shaped [n_out, ...]], source or None): source is the
        uint32 map (source index | kind << 30) as an int32 tensor when want_source. Stream-ordered."""
        import torch
        n, n_out = int(means.shape[0]), int(n_out)
        self._f32(("means", means, n * 3), ("log_scales", log_scales, n * 3), ("rotations", rotations, n * 4),
                  ("scales", scales, n * 3), ("noise", noise, n * 6))
        dev = means.device
        new = lambda t: torch.empty((n_out,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)  # noqa: E731
        means_out, ls_out = new(means), new(log_scales)
        if len(rows) > _abi.DENSIFY_MAX_ROWS:
            raise _abi.PtgsError(f"{len(rows)} rows: at most {_abi.DENSIFY_MAX_ROWS}")
        arr = (_abi.DensifyRows * max(1, len(rows)))()
        outs = []
        for k, (t, zero_new) in enumerate(rows):
            if t.shape[0] != n or t.numel() == 0 and n:
                raise _abi.PtgsError(f"rows[{k}] must have {n} non-empty rows (got {tuple(t.shape)})")
            self._f32((f"rows[{k}]", t, t.numel()))
            outs.append(new(t))
            arr[k].src, arr[k].dst = _ptr(t), _ptr(outs[-1])
            arr[k].width, arr[k].zero_new = (t.numel() // n if n else 1), int(bool(zero_new))
        source = torch.empty(n_out, dtype=torch.int32, device=dev) if want_source else None
        rc = self.lib.ptgs_gaussians_densify_apply(self._h, n, n_out, _ptr(means), _ptr(log_scales), _ptr(rotations),
                                                   _ptr(scales), _ptr(noise), _ptr(means_out), _ptr(ls_out), arr,
                                                   len(rows), _ptr(source), _stream(stream))
        self._chk(rc, "ptgs_gaussians_densify_apply")
        return means_out, ls_out, outs, source

    # ---------------------------------------------------------------- optimizer step
    def adam_step(self, rows, *, step: int, betas=(0.9, 0.999), eps: float = 1e-15, radii=None, masked: bool = False,
                  stream=None):
        """ptgs_gaussians_adam_step: one Adam step over every per-Gaussian array of rows in one launch. rows: a
        sequence of (param, grad, exp_avg, exp_avg_sq, lr) or (..., lr, head, lr_head), float32 device tensors
        [N, ...] of one shape per entry (at most 16 entries); the first `head` floats of each row step with
        lr_head. param, exp_avg and exp_avg_sq are updated in place through their pointers (behind autograd's
        back: pass detached leaves, after the backward). step: 1 for the first call of a run.
        masked=True steps only the Gaussians the published frame saw (radius > 0; the latest splat of this
        renderer, which must have N Gaussians, and not an overlapped frame) and leaves the others untouched;
        radii (int32 [N]) are used instead of the frame's when given, and imply masked. masked=False without
        radii is a dense Adam. Stream-ordered, no host wait; reproducible (no atomics)."""
        import torch
        rows = list(rows)
        if not rows or len(rows) > _abi.ADAM_MAX_ROWS:
            raise _abi.PtgsError(f"{len(rows)} rows: 1 .. {_abi.ADAM_MAX_ROWS}")
        n = int(rows[0][0].shape[0])
        arr = (_abi.AdamRows * len(rows))()
        for k, r in enumerate(rows):
            if len(r) not in (5, 7):
                raise _abi.PtgsError(f"rows[{k}] must be (param, grad, exp_avg, exp_avg_sq, lr[, head, lr_head])")
            p, g, m, v, lr = r[:5]
            head, lr_head = (int(r[5]), float(r[6])) if len(r) == 7 else (0, 0.0)
            if p.shape[0] != n or p.numel() == 0 and n:
                raise _abi.PtgsError(f"rows[{k}] must have {n} non-empty rows (got {tuple(p.shape)})")
            self._f32((f"rows[{k}].param", p, p.numel()), (f"rows[{k}].grad", g, p.numel()),
                      (f"rows[{k}].exp_avg", m, p.numel()), (f"rows[{k}].exp_avg_sq", v, p.numel()))
            arr[k].param, arr[k].grad, arr[k].exp_avg, arr[k].exp_avg_sq = _ptr(p), _ptr(g), _ptr(m), _ptr(v)
            arr[k].width, arr[k].head = (p.numel() // n if n else 1), head
            arr[k].lr, arr[k].lr_head = float(lr), lr_head
        if radii is not None:
            if radii.dtype != torch.int32 or radii.numel() != n:
                raise _abi.PtgsError(f"radii must be int32 with {n} elements (got {radii.dtype}, {radii.numel()})")
            rp = _ptr(radii) or None
        elif masked:
            b = self.splat_buffers()
            if b.num_gaussians != n or (n and not b.radii):
                raise _abi.PtgsError(f"the published frame has {b.num_gaussians} gaussians, the step {n}: "
                                     "a masked adam_step follows a published splat of the same Gaussians")
            rp = b.radii or None
        else:
            rp = None
        prm = _abi.AdamParams(float(betas[0]), float(betas[1]), float(eps), int(step))
        rc = self.lib.ptgs_gaussians_adam_step(self._h, n, arr, len(rows), C.byref(prm), rp, _stream(stream))
        self._chk(rc, "ptgs_gaussians_adam_step")

    def opacity_reset(self, opacity_logits, max_opacity: float = 0.01, exp_avg=None, exp_avg_sq=None, stream=None):
        """ptgs_gaussians_opacity_reset: the trainer's reset_opacity in place: every logit above
        logit(max_opacity) becomes that value, and the opacity's Adam moments (float32 [N] each, optional) are
        zeroed for every Gaussian. Stream-ordered."""
        n = int(opacity_logits.numel())
        self._f32(("opacity_logits", opacity_logits, n),
                  *([("exp_avg", exp_avg, n)] if exp_avg is not None else []),
                  *([("exp_avg_sq", exp_avg_sq, n)] if exp_avg_sq is not None else []))
        rc = self.lib.ptgs_gaussians_opacity_reset(self._h, _ptr(opacity_logits) or None, n, float(max_opacity),
                                                   _ptr(exp_avg) or None, _ptr(exp_avg_sq) or None, _stream(stream))
        self._chk(rc, "ptgs_gaussians_opacity_reset")

    # ---------------------------------------------------------------- the ends of a training run
    def checkpoint_init(self, scales, opacities, colors, sh_degree: int, out=None, stream=None):
        """ptgs_gaussians_checkpoint_init: (log_scales, opacity_logits, sh) of gaussians_from_points' activated
        scales [N, 3], opacities [N] and RGB colors [N, 3]: the logarithm, the logit and RGB2SH into the DC
        term of zeroed sh [N, (sh_degree+1)^2, 3], in one launch. New tensors, or out=(log_scales,
        opacity_logits, sh) (the first two may be scales / opacities themselves: in place). Stream-ordered."""
        import torch
        n, d = int(opacities.shape[0]), int(sh_degree)
        if not 0 <= d <= 3:
            raise _abi.PtgsError(f"sh_degree {sh_degree}: 0..3")
        k = (d + 1) ** 2
        ls, lo, sh = out if out is not None else (
            torch.empty_like(scales), torch.empty_like(opacities),
            torch.empty((n, k, 3), dtype=torch.float32, device=scales.device))
        self._f32(("scales", scales, n * 3), ("opacities", opacities, n), ("colors", colors, n * 3),
                  ("log_scales", ls, n * 3), ("opacity_logits", lo, n), ("sh", sh, n * k * 3))
        rc = self.lib.ptgs_gaussians_checkpoint_init(self._h, _ptr(scales), _ptr(opacities), _ptr(colors), n, d,
                                                     _ptr(ls), _ptr(lo), _ptr(sh), _stream(stream))
        self._chk(rc, "ptgs_gaussians_checkpoint_init")
        return ls, lo, sh

    def image_mse(self, image, target, out=None, stream=None):
        """ptgs_image_mse: the summed squared error over the rgb of image [H, W, 4] against target [H, W, 3 or 4]
        (contiguous float32 device tensors) as a float64 device tensor [1] (`out`, or a new one) that is not read
        back here: mse = sum / (3 W H), PSNR = -10 log10(mse). A fixed summation order: two runs give the same
        bits. Stream-ordered. An empty image leaves `out` as it is (a new one: 0)."""
        import torch
        if image.dim() != 3 or int(image.shape[2]) != 4:
            raise _abi.PtgsError(f"image must be [H, W, 4] (got {tuple(image.shape)})")
        h, w = int(image.shape[0]), int(image.shape[1])
        c = int(target.shape[2]) if target.dim() == 3 else 0
        if c not in (3, 4) or tuple(target.shape[:2]) != (h, w):
            raise _abi.PtgsError(f"target must be [{h}, {w}, 3 or 4] (got {tuple(target.shape)})")
        if out is None:
            out = torch.zeros(1, dtype=torch.float64, device=image.device)
        elif out.dtype != torch.float64 or out.numel() != 1:
            raise _abi.PtgsError("out must be one float64")
        self._f32(("image", image, h * w * 4), ("target", target, h * w * c))
        rc = self.lib.ptgs_image_mse(self._h, _ptr(image) or None, _ptr(target) or None, c, w, h, _ptr(out),
                                     _stream(stream))
        self._chk(rc, "ptgs_image_mse")
        return out

    def permute_sh(self, sh, ids, stream=None):
        """ptgs_gaussians_permute_sh: sh[ids] as a new tensor: the SH rows of the copy that
        sort_gaussians_spatial returned with these ids."""
        import torch
        out = torch.empty_like(sh)
        self._f32(("sh", sh, sh.numel()))
        if ids.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or ids.numel() != sh.shape[0]:
            raise _abi.PtgsError(f"ids must be {sh.shape[0]} 32-bit integers")
        rc = self.lib.ptgs_gaussians_permute_sh(self._h, _ptr(sh), self._sh_degree(sh), _ptr(ids), int(sh.shape[0]),
                                                _ptr(out), _stream(stream))
        self._chk(rc, "ptgs_gaussians_permute_sh")
        return out

    def splat_gaussians_sh(self, g: dict, ubo: Ubo, width: int, height: int, out, active_degree=None, stream=None,
                           **kwargs):
        """splat_gaussians of Gaussians whose colour is g["sh"] ([N, (d+1)^2, 3]): sh_colors from
        ubo.camera_pos into a colors tensor kept for the next call, then splat_gaussians with it on the
        same stream (other arguments as there). With set_splat_overlap(True) the cached colors are
        rewritten between overlapped calls: see INTEGRATION.md."""
        import torch
        n = int(g["means"].shape[0])
        col = getattr(self, "_sh_colors", None)
        if col is None or col.shape[0] != n or col.device != g["means"].device:
            col = self._sh_colors = torch.empty((n, 3), dtype=torch.float32, device=g["means"].device)
        self.sh_colors(g["means"], g["sh"], list(ubo.camera_pos), out=col, active_degree=active_degree, stream=stream)
        gc = {k: v for k, v in g.items() if k != "sh"}
        gc["colors"] = col
        return self.splat_gaussians(gc, ubo, width, height, out, stream=stream, **kwargs)

    def splat_status(self, stream=None) -> SplatStatus:
        """ptgs_splat_status_read: waits for `stream` and the view streams, returns and clears the
        counts since the last query: frames left incomplete (spill pool exhausted), tiles completed
        through the spill pool, tiles left incomplete; buffer capacities."""
        st = SplatStatus()
        self._chk(self.lib.ptgs_splat_status_read(self._h, C.byref(st), _stream(stream)), "ptgs_splat_status_read")
        return st

    def splat_reserve(self, pairs: int):
        """Grow every view slot's pair buffer and spill pool to at least `pairs` (frames of up to that
        many pairs are always complete)."""
        self._chk(self.lib.ptgs_splat_reserve(self._h, int(pairs)), "ptgs_splat_reserve")

    def bvh_buffers(self) -> BvhBuffers:
        """Device pointers of the uploaded 4-wide BVH nodes and leaf-order triangle records."""
        b = BvhBuffers()
        self._chk(self.lib.ptgs_scene_get_bvh(self._h, C.byref(b)), "ptgs_scene_get_bvh")
        return b

    def splat_buffers(self) -> SplatBuffers:
        b = SplatBuffers()
        self._chk(self.lib.ptgs_splat_get_buffers(self._h, C.byref(b)), "ptgs_splat_get_buffers")
        return b

    def splat_tile_rows(self) -> tuple[int, int]:
        """ptgs_splat_get_tile_rows: (device pointer, row capacity) of the latest splat's fused slot rows
        (its front end's unsorted (depth bits << 32 | gaussian) pairs, tile t at t * capacity); (0, 0) when
        that frame ran the three-launch front end."""
        p, cap = C.c_void_p(), C.c_uint32()
        self._chk(self.lib.ptgs_splat_get_tile_rows(self._h, C.byref(p), C.byref(cap)), "ptgs_splat_get_tile_rows")
        return (p.value or 0), cap.value

    def splat_stage_ms(self) -> np.ndarray:
        """[preprocess+count, colscan, scatter, large-tile sort, 0, sort+blend] ms of the last splat
        (FLAG_TIME_STAGES)."""
        out = np.zeros(6, np.float32)
        self._chk(self.lib.ptgs_splat_stage_ms(self._h, _abi.fptr(out)), "ptgs_splat_stage_ms")
        return out

    def encode_srgb8(self, rgba32f, width: int, height: int, rgba8, stream=None):
        rc = self.lib.ptgs_encode_srgb8(self._h, _ptr(rgba32f), width, height, _ptr(rgba8), _stream(stream))
        self._chk(rc, "ptgs_encode_srgb8")

    # ---------------------------------------------------------------- memory helpers
    def copy_d2h(self, dst: np.ndarray, src_ptr: int, nbytes: int):
        self._chk(self.lib.ptgs_memcpy_d2h(self._h, dst.ctypes.data, src_ptr, nbytes), "ptgs_memcpy_d2h")

    def synchronize(self):
        self._chk(self.lib.ptgs_synchronize(self._h), "ptgs_synchronize")


def torus_push(model=None, major_radius: float = 3.5, minor_radius: float = 1.0, height: float = 3.0,
               mode: int = 0) -> RayPush:
    p = RayPush()
    m = np.eye(4, dtype=np.float32).reshape(16) if model is None else np.asarray(model, np.float32).reshape(16)
    p.model[:] = [float(x) for x in m]
    p.mode = mode
    p.major_radius = major_radius
    p.minor_radius = minor_radius
    p.height = height
    return p
