"""Densification and pruning without a GPU: the sequential numpy reference (tests/densify_ref.py) against
hand-written expectations, csrc/splat_densify_math.h built for the host (the fused one-pass rule the kernels call)
against the reference bit for bit, the three new structs against their ctypes mirrors, and the exports."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import densify_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
K = lambda i, kind: np.uint32(i | (kind << D.KIND_SHIFT))  # noqa: E731


@pytest.fixture(scope="module")
def densify_bin(tmp_path_factory):
    """csrc/splat_densify_math.h compiled for the host (stand-alone, ASan + UBSan linked in)."""
    exe = str(tmp_path_factory.mktemp("dn") / "densify_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "pathtracer_gaussiansplatting_amd", "csrc"),
           os.path.join(ROOT, "tests", "native", "densify_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _views(n, seed=3):
    """Three views of different sizes, a third of the Gaussians invisible in each."""
    rng = np.random.default_rng(seed)
    out = []
    for W, H in ((60, 44), (800, 600), (1, 7)):
        radii = rng.integers(1, 50, n).astype(np.int32)
        radii[rng.random(n) < 1 / 3] = 0
        radii[rng.random(n) < 0.05] = -1  # (never produced by the rasterizer; not visible either)
        out.append((W, H, rng.normal(0.0, 1e-3, (n, 2)).astype(F), radii))
    return out


def _run_host(exe, tmp_path, case, views=()):
    n = case["n"]
    blob = D.pack(case) + np.uint32(len(views)).tobytes()
    for W, H, g2d, radii in views:
        blob += np.asarray([W, H], np.uint32).tobytes() + g2d.tobytes() + radii.tobytes()
    (tmp_path / "in.bin").write_bytes(blob)
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0, (r.returncode, r.stderr)
    raw = np.fromfile(tmp_path / "out.bin", np.uint32)
    names = ("survivors", "clones", "split_sources", "pruned_originals", "pruned_children", "total")
    counts = dict(zip(names, (int(v) for v in raw[:6])))
    t = counts["total"]
    at = 6
    take = lambda count: raw[at:at + count]  # noqa: E731
    out = {"counts": counts, "source": take(t).copy()}
    at += t
    out["means"] = take(3 * t).view(F).reshape(t, 3)
    at += 3 * t
    out["log_scales"] = take(3 * t).view(F).reshape(t, 3)
    at += 3 * t
    out["rows"] = []
    for a, _ in case["rows"]:
        w = a.reshape(n, -1).shape[1] if n else 1
        out["rows"].append(take(t * w).view(F).reshape(t, w))
        at += t * w
    out["stats"] = tuple(raw[at + k * n:at + (k + 1) * n].view(F) for k in range(3))
    assert at + 3 * n == raw.size
    return out


def _same(got, ref):
    assert got["counts"] == ref["counts"]
    assert np.array_equal(got["source"], ref["source"])
    for k in ("means", "log_scales"):  # bit for bit (compared as integers: a NaN would not hide)
        assert np.array_equal(got[k].view(np.uint32), ref[k].view(np.uint32)), k
    assert len(got["rows"]) == len(ref["rows"])
    for a, b in zip(got["rows"], ref["rows"]):
        assert np.array_equal(a.view(np.uint32), b.reshape(a.shape).view(np.uint32))


def test_reference_on_the_hand_case():
    c = D.hand_case()
    r = D.densify_and_prune(c)
    assert r["counts"] == {"survivors": 3, "clones": 1, "split_sources": 1, "pruned_originals": 1,
                           "pruned_children": 2, "total": 6}
    assert list(r["source"]) == [K(0, 0), K(1, 0), K(5, 0), K(1, 1), K(2, 2), K(2, 3)]
    # the unit quaternion is the identity exactly, so a child sits at mean + scales * noise
    want = np.array([[0, 1, 2], [3, 4, 5], [15, 16, 17], [3, 4, 5], [6.5, 7.5, 8.5], [5, 6, 7]], F)
    assert np.array_equal(r["means"], want)
    ls = np.full((6, 3), F(-1), F)
    ls[4:] = F(-1) - F(0.4700036)
    assert np.array_equal(r["log_scales"], ls)
    assert np.array_equal(r["rows"][0][:, 0], np.array([10, 11, 15, 11, 12, 12], F))  # copied from the source
    assert np.array_equal(r["rows"][1], np.array([[1, 2], [3, 4], [11, 12], [0, 0], [0, 0], [0, 0]], F))  # zero for new


def test_reference_accumulate_by_hand():
    g2d = np.array([[0.75, 2.0], [0.75, 2.0], [1.0, 1.0]], F)
    radii = np.array([7, 0, 2], np.int32)
    z = np.zeros(3, F)
    a, d, m = D.accumulate(g2d, radii, 8, 4, z, z, z + F(5))  # 0.5 W = 4, 0.5 H = 2: (3, 4) -> 5
    assert np.array_equal(a, np.array([5, 0, np.sqrt(F(20))], F))
    assert np.array_equal(d, np.array([1, 0, 1], F)) and np.array_equal(m, np.array([7, 5, 5], F))


def test_main_case_has_every_fate_and_the_threshold_rows():
    n = 1000
    c = D.make_case(n)
    r = D.densify_and_prune(c)
    print(r["counts"])
    assert D.fates_present(r["counts"], n), r["counts"]
    src, kind = r["source"] & np.uint32((1 << D.KIND_SHIFT) - 1), r["source"] >> np.uint32(D.KIND_SHIFT)
    fate = lambda i: sorted(int(k) for k in kind[src == i])  # noqa: E731
    S = D.SPECIAL
    assert fate(S["avg_eq_threshold"]) == [0, 1]  # avg == grad_threshold is hot
    assert fate(S["smax_eq_split"]) == [0, 1]  # smax == scale_split clones, does not split
    assert fate(S["opacity_eq_min"]) == [0]  # o == min_opacity is kept
    assert fate(S["radius_eq_max"]) == [0]  # r == max_screen_radius is kept
    assert fate(S["denom_zero"]) == [0]  # never seen: not hot whatever accum holds
    assert fate(S["zero_quaternion"]) == [2, 3]
    assert fate(S["child_scale_eq_max"]) == [2, 3]  # smax / 1.6 == max_scale is kept
    i = S["zero_quaternion"]
    for k in (0, 1):  # R = identity
        at = np.flatnonzero((src == i) & (kind == 2 + k))[0]
        assert np.array_equal(r["means"][at], c["means"][i] + c["scales"][i] * c["noise"][k][i])


CASES = {"n1-survive": lambda: D.single("survive"), "n1-clone": lambda: D.single("clone"),
         "n1-split": lambda: D.single("split"), "n1-pruned": lambda: D.single("pruned"),
         "hand": D.hand_case, "n257": lambda: D.make_case(257), "main-n1000": lambda: D.make_case(1000),
         "n6145": lambda: D.make_case(6145, widths=(4,), zero_widths=(3,)),
         "all-pruned": lambda: D.make_case(300, mix="pruned"), "all-split": lambda: D.make_case(300, mix="split"),
         "nothing-hot": lambda: D.make_case(300, thresholds=D.NOTHING_HOT, special=False),
         "sh-widths": lambda: D.make_case(129, widths=(3, 12, 27, 48, 1, 4), zero_widths=(3, 12, 27, 48, 1, 4))}


@pytest.mark.parametrize("name", list(CASES))
def test_fused_rule_on_the_host_matches_the_sequence(densify_bin, tmp_path, name):
    """accumulate, plan and apply through splat_densify_math.h (one pass over the sources) equal the trainer's
    sequence bit for bit: counts, source map and every output array."""
    c = CASES[name]()
    ref = D.densify_and_prune(c)
    views = _views(c["n"])
    got = _run_host(densify_bin, tmp_path, c, views)
    _same(got, ref)
    n = c["n"]
    if name == "all-pruned":
        assert ref["counts"]["total"] == 0
    if name == "all-split":
        assert ref["counts"]["total"] == 2 * n and ref["counts"]["split_sources"] == n
    if name == "nothing-hot":
        assert ref["counts"]["total"] == n and np.array_equal(ref["means"], c["means"])
        for a, (b, _) in zip(ref["rows"], c["rows"]):
            assert np.array_equal(a, b)  # the moments too
    if name.startswith("n1-"):
        want = {"survive": (1, 0, 0, 0, 0, 1), "clone": (1, 1, 0, 0, 0, 2), "split": (0, 0, 1, 0, 0, 2),
                "pruned": (0, 0, 0, 1, 0, 0)}[name[3:]]
        assert tuple(ref["counts"].values()) == want
    stats = tuple(np.zeros(n, F) for _ in range(3))
    for W, H, g2d, radii in views:
        stats = D.accumulate(g2d, radii, W, H, *stats)
    for a, b in zip(got["stats"], stats):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert n < 3 or (stats[1] > 0).any() and (stats[1] < 3).any()


def test_struct_layouts_match_the_ctypes_mirrors(densify_bin):
    from pathtracer_gaussiansplatting_amd import _abi
    r = subprocess.run([densify_bin, "layout"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    mirrors = {"ptgs_densify_params": _abi.DensifyParams, "ptgs_densify_counts": _abi.DensifyCounts,
               "ptgs_densify_rows": _abi.DensifyRows}
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 3
    for line in lines:
        w = line.split()
        st = mirrors[w[0]]
        assert C.sizeof(st) == int(w[1]), w[0]
        fields = dict(zip(w[2::2], (int(v) for v in w[3::2])))
        assert list(fields) == [f[0] for f in st._fields_], w[0]
        for name, off in fields.items():
            assert getattr(st, name).offset == off, (w[0], name)


def test_densify_entry_points_are_exported(native_lib):
    for name in ("ptgs_densify_accumulate", "ptgs_gaussians_densify_plan", "ptgs_gaussians_densify_apply"):
        assert hasattr(native_lib, name)
    # a null context is rejected before anything else is read
    assert native_lib.ptgs_densify_accumulate(None, None, None, 1, 1, 1, None, None, None, None) == -1
    assert native_lib.ptgs_gaussians_densify_plan(None, None, None, None, None, None, 1, None, None, None) == -1
    assert native_lib.ptgs_gaussians_densify_apply(None, 1, 1, None, None, None, None, None, None, None, None, 0, None,
                                                   None) == -1


def test_python_layer_is_exported():
    import pathtracer_gaussiansplatting_amd as P
    assert callable(P.densify_and_prune) and callable(P.DensifyStats)
    for m in ("densify_accumulate", "densify_plan", "densify_apply"):
        assert callable(getattr(P.Renderer, m))
