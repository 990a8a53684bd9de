"""ptgs_read_gaussian_ply / load_gaussian_ply: trained-3DGS checkpoints (point_cloud.ply) written here
with numpy in the trainers' property order and read back bit for bit; query mode, capacity, the
rejections, and ptgs_read_ply on the same file (its DC-term colours: the shared parser)."""
import ctypes as C

import numpy as np
import pytest

from pathtracer_gaussiansplatting_amd import _abi, load_gaussian_ply
from pathtracer_gaussiansplatting_amd.capture import read_ply

N = 37


def _props(deg):
    n_rest = 3 * ((deg + 1) ** 2 - 1)
    return (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{j}" for j in range(n_rest)]
            + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"])


def _table(deg, seed=0, exact=False):
    """(N, properties) float32 in the trainers' column order; exact: multiples of 1/64 (ASCII round trip)."""
    rng = np.random.default_rng(seed + deg)
    t = rng.normal(0.0, 2.0, (N, len(_props(deg)))).astype(np.float32)
    if exact:
        t = (np.round(t * 64) / 64).astype(np.float32)
    return t


def _write(path, names, table, fmt="binary_little_endian", count=None, drop_tail=0):
    hdr = ["ply", f"format {fmt} 1.0", f"element vertex {len(table) if count is None else count}"]
    hdr += [f"property float {n}" for n in names] + ["end_header"]
    body = b""
    if fmt == "ascii":
        body = "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in table).encode()
    else:
        body = table.astype(">f4" if fmt == "binary_big_endian" else "<f4").tobytes()
    if drop_tail:
        body = body[:-drop_tail]
    with open(path, "wb") as f:
        f.write(("\n".join(hdr) + "\n").encode() + body)
    return str(path)


def _expect(names, table, deg):
    col = {n: table[:, i] for i, n in enumerate(names)}
    K = (deg + 1) ** 2
    sh = np.zeros((len(table), K, 3), np.float32)
    for i in range(len(table)):  # the explicit loop of the file's channel-major f_rest
        for c in range(3):
            sh[i, 0, c] = col[f"f_dc_{c}"][i]
            for k in range(1, K):
                sh[i, k, c] = col[f"f_rest_{c * (K - 1) + (k - 1)}"][i]
    return {"means": np.stack([col["x"], col["y"], col["z"]], -1),
            "log_scales": np.stack([col[f"scale_{a}"] for a in range(3)], -1),
            "rotations": np.stack([col[f"rot_{a}"] for a in range(4)], -1),
            "opacity_logits": col["opacity"].copy(), "sh": sh}


def _check(got, names, table, deg):
    exp = _expect(names, table, deg)
    assert got["sh_degree"] == deg
    for k, v in exp.items():
        assert got[k].dtype == np.float32 and got[k].shape == v.shape, k
        assert np.array_equal(got[k].view(np.uint32), np.ascontiguousarray(v).view(np.uint32)), k
    # the transpose, stated the other way round: f_rest as [c][k-1]
    if deg:
        rest = np.stack([table[:, names.index(f"f_rest_{j}")] for j in range(3 * ((deg + 1) ** 2 - 1))], -1)
        assert np.array_equal(got["sh"][:, 1:, :], rest.reshape(len(table), 3, -1).transpose(0, 2, 1))


@pytest.mark.parametrize("deg", [0, 1, 2, 3])
@pytest.mark.parametrize("fmt", ["binary_little_endian", "binary_big_endian", "ascii", "shuffled"])
def test_round_trip(native_lib, tmp_path, deg, fmt):
    names = _props(deg)
    table = _table(deg, exact=(fmt == "ascii"))
    if fmt == "shuffled":
        perm = np.random.default_rng(9).permutation(len(names))
        names = [names[j] for j in perm]
        table = np.ascontiguousarray(table[:, perm])
        fmt = "binary_little_endian"
    p = _write(tmp_path / "point_cloud.ply", names, table, fmt)
    _check(load_gaussian_ply(p), names, table, deg)


def _query(lib, path, capacity=0, arrays=False, n=N, deg=3):
    cnt, d = C.c_uint32(12345), C.c_uint32(12345)
    K = (deg + 1) ** 2
    bufs = [np.zeros(max(n, 1) * w, np.float32) for w in (3, 3, 4, 1, 3 * K)] if arrays else [None] * 5
    ptrs = [b.ctypes.data if b is not None else None for b in bufs]
    rc = lib.ptgs_read_gaussian_ply(path.encode(), *ptrs, capacity, C.byref(cnt), C.byref(d))
    return rc, cnt.value, d.value


def test_query_and_capacity(native_lib, tmp_path):
    for deg in range(4):
        p = _write(tmp_path / f"d{deg}.ply", _props(deg), _table(deg))
        assert _query(native_lib, p) == (0, N, deg)
    assert _query(native_lib, p, capacity=N - 1, arrays=True)[0] == -4  # PTGS_ERANGE
    assert _query(native_lib, p, capacity=N, arrays=True) == (0, N, 3)
    assert native_lib.ptgs_read_gaussian_ply(None, None, None, None, None, None, 0, None, None) == -1
    assert _query(native_lib, str(tmp_path / "missing.ply"))[0] == -5


def test_rejections(native_lib, tmp_path):
    names, table = _props(1), _table(1)

    def rc_of(keep_names, extra=(), **kw):
        idx = [names.index(n) for n in keep_names]
        nm = list(keep_names) + list(extra)
        tb = np.concatenate([table[:, idx], np.zeros((N, len(extra)), np.float32)], 1)
        p = _write(tmp_path / "bad.ply", nm, np.ascontiguousarray(tb), **kw)
        with pytest.raises(_abi.PtgsError) as e:
            load_gaussian_ply(p)
        return e.value.code

    assert rc_of(names, extra=["f_rest_9"]) == -5                        # ten f_rest_*
    gap = [n for n in names if n != "f_rest_3"]
    assert rc_of(gap, extra=["f_rest_9"]) == -5                          # nine, f_rest_3 missing
    assert rc_of(gap) == -5                                              # eight
    assert rc_of([n for n in names if n != "opacity"]) == -5
    assert rc_of([n for n in names if n != "rot_3"]) == -5
    assert rc_of([n for n in names if n != "scale_1"]) == -5
    assert rc_of([n for n in names if n != "f_dc_2"]) == -5
    assert rc_of(names, drop_tail=5) == -5                               # body shorter than the count
    assert rc_of(names, count=N + 1) == -5
    p = _write(tmp_path / "ok.ply", names, table)                        # and the unmutilated file loads
    assert load_gaussian_ply(p)["sh_degree"] == 1


def test_read_ply_still_gives_dc_colours(native_lib, tmp_path):
    names, table = _props(3), _table(3, seed=4)
    table[:, names.index("f_dc_0")] *= 0.5  # (a spread of in-range and clamped colours)
    p = _write(tmp_path / "point_cloud.ply", names, table)
    xyz, nrm, rgb = read_ply(p)
    col = {n: table[:, i] for i, n in enumerate(names)}
    assert np.array_equal(xyz, np.stack([col["x"], col["y"], col["z"]], -1))
    assert np.array_equal(nrm, np.stack([col["nx"], col["ny"], col["nz"]], -1))
    dc = np.stack([col[f"f_dc_{c}"] for c in range(3)], -1).astype(np.float64)
    v = np.floor((0.5 + 0.28209479177387814 * dc) * 255.0 + 0.5)
    assert np.array_equal(rgb, np.clip(v, 0, 255).astype(np.uint8))
    assert 0 < (rgb == 0).mean() < 1 and (rgb == 255).any()
