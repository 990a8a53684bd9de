"""The reference of densification and pruning (ptgs_densify_accumulate, ptgs_gaussians_densify_plan / _apply) in
numpy float32, and the cases of its tests.

densify_and_prune() is written as the trainer's SEQUENCE (Kerbl et al., densify_and_prune with the new Gaussians
inheriting the parent's screen radius): clone and concatenate, split and concatenate and remove the parents, then
one prune mask over everything. The library evaluates a fused one-pass rule (include/ptgs/ptgs.h); this file
deliberately does not, so the two formulations check each other. Every float operation is a float32 numpy
operation in the contract's order; no transcendental is evaluated (activated scales / opacities are inputs).
"""
import numpy as np

F = np.float32
KIND_SHIFT = 30
ORIGINAL, CLONE, CHILD0, CHILD1 = 0, 1, 2, 3
SPLIT_DIV = F(1.6)
LOG_SPLIT = F(0.4700036)

# the thresholds of the cases
THRESHOLDS = dict(grad_threshold=F(0.0002), scale_split=F(0.05), min_opacity=F(0.005), max_scale=F(0.5),
                  max_screen_radius=F(40.0))
NOTHING_HOT = dict(grad_threshold=F(1e9), scale_split=F(0.05), min_opacity=F(0.0), max_scale=F(0.0),
                   max_screen_radius=F(0.0))


def accumulate(g2d, radii, W, H, accum, denom, max_radii):
    """One view's statistic: new (accum, denom, max_radii)."""
    vis = radii > 0
    gx = g2d[:, 0] * (F(0.5) * F(W))
    gy = g2d[:, 1] * (F(0.5) * F(H))
    norm = np.sqrt(gx * gx + gy * gy)
    assert norm.dtype == F
    return (np.where(vis, accum + norm, accum).astype(F), np.where(vis, denom + F(1), denom).astype(F),
            np.where(vis, np.maximum(max_radii, radii.astype(F)), max_radii).astype(F))


def rotation(q):
    """[n, 3, 3] of (w, x, y, z) / len, the entries in the contract's order; len == 0: the identity."""
    w, x, y, z = (q[:, k] for k in range(4))
    n = np.sqrt(((w * w + x * x) + y * y) + z * z)
    zero = n == 0
    n1 = np.where(zero, F(1), n)
    w, x, y, z = w / n1, x / n1, y / n1, z / n1
    one, two = F(1), F(2)
    R = np.empty((len(q), 3, 3), F)
    R[:, 0, 0] = one - two * (y * y + z * z)
    R[:, 0, 1] = two * (x * y - w * z)
    R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z)
    R[:, 1, 1] = one - two * (x * x + z * z)
    R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y)
    R[:, 2, 1] = two * (y * z + w * x)
    R[:, 2, 2] = one - two * (x * x + y * y)
    R[zero] = np.eye(3, dtype=F)
    return R


def _cat(table, new):
    return {k: np.concatenate([table[k], new[k]]) for k in table}


def _take(table, mask):
    return {k: v[mask] for k, v in table.items()}


def densify_and_prune(case, thresholds=None):
    """The trainer's sequence on a case of make_case(). Returns {"means", "log_scales", "rows" (list), "source"
    (uint32: source index | kind << 30), "counts" (dict)}."""
    th = dict(case["thresholds"] if thresholds is None else thresholds)
    n = len(case["means"])
    accum, denom = case["accum"], case["denom"]
    with np.errstate(divide="ignore", invalid="ignore"):
        grads = np.where(denom > 0, accum / np.where(denom > 0, denom, F(1)), F(0)).astype(F)
    table = {"means": case["means"], "log_scales": case["log_scales"], "rotations": case["rotations"],
             "scales": case["scales"], "opacities": case["opacities"], "radii": case["max_radii"],
             "src": np.arange(n, dtype=np.uint32), "kind": np.zeros(n, np.uint32)}
    zero_new = []
    for k, (a, z) in enumerate(case["rows"]):
        table[f"row{k}"] = a.reshape(n, -1)
        zero_new.append(f"row{k}") if z else None

    def new_rows(t, kind):
        t = dict(t)
        for name in zero_new:
            t[name] = np.zeros_like(t[name])
        t["kind"] = np.full(len(t["src"]), kind, np.uint32)
        return t

    # densify_and_clone
    smax = table["scales"].max(axis=1)
    mask = (grads >= th["grad_threshold"]) & (smax <= th["scale_split"])
    table = _cat(table, new_rows(_take(table, mask), CLONE))
    # densify_and_split: the gradients padded with zeros for what the clone step appended
    padded = np.zeros(len(table["src"]), F)
    padded[:n] = grads
    smax = table["scales"].max(axis=1)
    mask = (padded >= th["grad_threshold"]) & (smax > th["scale_split"])
    parents = _take(table, mask)
    R = rotation(parents["rotations"])
    children = []
    for k in (0, 1):
        c = new_rows(parents, CHILD0 + k)
        v = parents["scales"] * case["noise"][k][parents["src"]]
        rv = (R[:, :, 0] * v[:, 0:1] + R[:, :, 1] * v[:, 1:2]) + R[:, :, 2] * v[:, 2:3]
        c["means"] = parents["means"] + rv
        c["scales"] = parents["scales"] / SPLIT_DIV
        c["log_scales"] = parents["log_scales"] - LOG_SPLIT
        assert c["means"].dtype == F and c["scales"].dtype == F and c["log_scales"].dtype == F
        children.append(c)
    table = _cat(_cat(table, children[0]), children[1])
    table = _take(table, ~np.concatenate([mask, np.zeros(2 * int(mask.sum()), bool)]))
    # the prune mask over everything
    prune = table["opacities"] < th["min_opacity"]
    if th["max_screen_radius"] > 0:
        prune |= table["radii"] > th["max_screen_radius"]
    if th["max_scale"] > 0:
        prune |= table["scales"].max(axis=1) > th["max_scale"]
    gone = _take(table, prune)
    table = _take(table, ~prune)
    kind = table["kind"]
    counts = {"survivors": int((kind == ORIGINAL).sum()), "clones": int((kind == CLONE).sum()),
              "split_sources": int((kind == CHILD0).sum()),
              "pruned_originals": int((gone["kind"] == ORIGINAL).sum()),
              "pruned_children": int((gone["kind"] >= CHILD0).sum()), "total": len(kind)}
    assert int((kind == CHILD1).sum()) == counts["split_sources"]
    rows = [table[f"row{k}"].reshape((len(kind),) + a.shape[1:]) for k, (a, _) in enumerate(case["rows"])]
    return {"means": table["means"], "log_scales": table["log_scales"], "rows": rows,
            "source": (table["src"] | (kind << np.uint32(KIND_SHIFT))).astype(np.uint32), "counts": counts}


SPECIAL = {"avg_eq_threshold": 0, "smax_eq_split": 1, "opacity_eq_min": 2, "radius_eq_max": 3, "denom_zero": 4,
           "zero_quaternion": 5, "child_scale_eq_max": 6}


def make_case(n, seed=0, widths=(4, 1, 48), zero_widths=(3, 48), thresholds=None, mix="main", special=True):
    """A case of n Gaussians: parameters, statistic, noise and rows (arrays of `widths` floats per Gaussian that
    are copied, then of `zero_widths` that are zero for new Gaussians: the moments). mix: "main" (every fate),
    "split" (everything split), "pruned" (everything pruned). special (n >= 8, main): rows 0..6 sit exactly on the
    thresholds (SPECIAL)."""
    th = dict(THRESHOLDS if thresholds is None else thresholds)
    rng = np.random.default_rng(7000 + 13 * n + seed)
    u = lambda lo, hi, size: rng.uniform(lo, hi, size).astype(F)  # noqa: E731
    cls = rng.choice(3, n, p=[0.5, 0.3, 0.2])  # small, large, huge
    hot = rng.random(n) < 0.5
    if mix == "split":
        cls[:], hot[:] = 1, True
    smax = np.where(cls == 0, u(0.005, 0.045, n), np.where(cls == 1, u(0.06, 0.45, n), u(0.9, 2.0, n))).astype(F)
    scales = (smax[:, None] * u(0.3, 1.0, (n, 3))).astype(F)
    scales[np.arange(n), rng.integers(0, 3, n)] = smax
    opacities = np.where(rng.random(n) < 0.15, u(0.0, 0.004, n), u(0.01, 0.99, n)).astype(F)
    max_radii = np.where(rng.random(n) < 0.05, u(41.0, 90.0, n), np.floor(u(0.0, 39.0, n))).astype(F)
    denom = np.floor(u(0.0, 6.0, n)).astype(F)
    avg = np.where(hot, u(3e-4, 1e-3, n), u(0.0, 1e-4, n)).astype(F)
    if mix == "split":
        opacities, max_radii, denom = u(0.01, 0.99, n), np.floor(u(0.0, 39.0, n)).astype(F), np.full(n, 2, F)
    if mix == "pruned":
        opacities = u(0.0, 0.004, n)
    accum = (avg * denom).astype(F)
    means = rng.normal(0.0, 1.0, (n, 3)).astype(F)
    rotations = rng.normal(0.0, 1.0, (n, 4)).astype(F)
    if special and mix == "main" and n >= 8:
        S = SPECIAL
        good = [S["avg_eq_threshold"], S["smax_eq_split"], S["opacity_eq_min"], S["radius_eq_max"], S["denom_zero"],
                S["zero_quaternion"], S["child_scale_eq_max"]]
        opacities[good], max_radii[good], denom[good] = F(0.5), F(3), F(2)
        scales[good] = F(0.01)
        accum[good] = F(0)
        accum[S["avg_eq_threshold"]] = th["grad_threshold"] * F(2)  # (/ 2: exact) -> hot, small: a clone
        accum[S["smax_eq_split"]] = F(1)
        scales[S["smax_eq_split"]] = (F(0.01), th["scale_split"], F(0.02))  # hot, == scale_split: a clone
        opacities[S["opacity_eq_min"]] = th["min_opacity"]  # not below: survives
        max_radii[S["radius_eq_max"]] = th["max_screen_radius"]  # not above: survives
        accum[S["denom_zero"]], denom[S["denom_zero"]] = F(5), F(0)  # never seen: average 0, survives
        accum[S["zero_quaternion"]] = F(1)
        scales[S["zero_quaternion"]] = (F(0.2), F(0.1), F(0.3))  # hot, large: split with R = identity
        rotations[S["zero_quaternion"]] = F(0)
        accum[S["child_scale_eq_max"]] = F(1)
        scales[S["child_scale_eq_max"]] = (F(0.1), th["max_scale"] * SPLIT_DIV, F(0.1))  # children at max_scale: kept
    case = {"n": n, "thresholds": th, "means": means, "rotations": rotations, "scales": scales,
            "log_scales": rng.normal(-3.0, 1.0, (n, 3)).astype(F), "opacities": opacities, "accum": accum,
            "denom": denom, "max_radii": max_radii, "noise": rng.normal(0.0, 1.0, (2, n, 3)).astype(F)}
    case["rows"] = [(rng.normal(0.0, 1.0, (n, w)).astype(F), False) for w in widths]
    case["rows"] += [(rng.normal(0.0, 1.0, (n, w)).astype(F), True) for w in zero_widths]
    return case


def single(fate):
    """N = 1 with the given fate: "survive", "clone", "split", "pruned"."""
    c = make_case(1, special=False)
    hot = fate in ("clone", "split")
    c["accum"][:], c["denom"][:] = (F(0.002) if hot else F(0)), F(2)
    c["scales"][0] = (F(0.2), F(0.1), F(0.3)) if fate == "split" else (F(0.01), F(0.02), F(0.03))
    c["opacities"][:] = F(0.001) if fate == "pruned" else F(0.5)
    c["max_radii"][:] = F(3)
    return c


def hand_case():
    """Six Gaussians, one of each fate and one never seen; expectations written by hand in
    test_densify_ref.py."""
    th = dict(THRESHOLDS)
    c = {"n": 6, "thresholds": th,
         "means": np.arange(18, dtype=F).reshape(6, 3),
         "rotations": np.tile(np.array([1, 0, 0, 0], F), (6, 1)),
         "log_scales": np.full((6, 3), F(-1), F),
         "scales": np.array([[0.01, 0.02, 0.03],   # 0: cold, small, opaque: survives
                             [0.01, 0.02, 0.03],   # 1: hot, small: survives and is cloned
                             [0.25, 0.125, 0.0625],  # 2: hot, large: split
                             [0.01, 0.02, 0.03],   # 3: transparent: pruned
                             [1.0, 2.0, 4.0],      # 4: hot, huge: split, the children pruned (4 / 1.6 > 0.5)
                             [0.01, 0.02, 0.03]], F),  # 5: never seen (denom 0): survives
         "opacities": np.array([0.5, 0.5, 0.5, 0.001, 0.5, 0.5], F),
         "accum": np.array([0.0001, 0.001, 0.001, 0.0, 0.001, 7.0], F),
         "denom": np.array([1, 1, 1, 1, 1, 0], F),
         "max_radii": np.array([3, 3, 3, 3, 3, 0], F),
         "noise": np.zeros((2, 6, 3), F)}
    c["noise"][0, 2] = (2, 4, 8)
    c["noise"][1, 2] = (-4, -8, -16)
    c["rows"] = [(np.arange(6, dtype=F).reshape(6, 1) + F(10), False), (np.arange(12, dtype=F).reshape(6, 2) + F(1), True)]
    return c


def fates_present(counts, n):
    """The five fates each at 5 % of n or more (the main case's precondition)."""
    return all(counts[k] >= 0.05 * n for k in ("survivors", "clones", "split_sources", "pruned_originals",
                                                "pruned_children"))


def pack(case):
    """The case as the host program's input file: a header of u32 (n, n_rows, then width and zero_new per row),
    the five thresholds, then the arrays."""
    head = [case["n"], len(case["rows"])]
    for a, z in case["rows"]:
        head += [a.reshape(case["n"], -1).shape[1] if case["n"] else 1, int(z)]
    th = case["thresholds"]
    blob = np.asarray(head, np.uint32).tobytes()
    blob += np.asarray([th["grad_threshold"], th["scale_split"], th["min_opacity"], th["max_scale"],
                        th["max_screen_radius"]], F).tobytes()
    for k in ("means", "log_scales", "rotations", "scales", "opacities", "accum", "denom", "max_radii", "noise"):
        blob += np.ascontiguousarray(case[k], F).tobytes()
    for a, _ in case["rows"]:
        blob += np.ascontiguousarray(a, F).tobytes()
    return blob
