"""The reference of the optimizer step (ptgs_gaussians_adam_step, ptgs_gaussians_opacity_reset) in numpy float32,
and the cases of its tests.

Every float operation is a float32 numpy operation in the order of the contract in include/ptgs/ptgs.h: np.float32
scalars and arrays throughout, no float64 promotion. The scalars the host derives come from Python doubles exactly
as the contract writes them.
"""
import math

import numpy as np

F = np.float32


def scalars(beta1, beta2, step):
    """(beta1, beta2, ob1, ob2, bc1, bc2s) as float32."""
    b1, b2 = F(beta1), F(beta2)
    ob1, ob2 = F(1) - b1, F(1) - b2
    bc1 = F(1.0 - float(b1) ** int(step))
    bc2s = F(math.sqrt(1.0 - float(b2) ** int(step)))
    for x in (ob1, ob2, bc1, bc2s):
        assert type(x) is F
    return b1, b2, ob1, ob2, bc1, bc2s


def row(param, grad, exp_avg, exp_avg_sq, lr, head=0, lr_head=0.0):
    """One entry of the table: the four arrays as [n, width] float32, the rates as float32."""
    n = param.shape[0]
    a = [np.ascontiguousarray(x, F).reshape(n, -1) for x in (param, grad, exp_avg, exp_avg_sq)]
    assert all(x.shape == a[0].shape for x in a) and 0 <= head <= a[0].shape[1]
    return {"param": a[0], "grad": a[1], "exp_avg": a[2], "exp_avg_sq": a[3], "lr": F(lr), "head": int(head),
            "lr_head": F(lr_head)}


def adam_step(rows, *, step, beta1=0.9, beta2=0.999, eps=1e-15, radii=None):
    """One step over every row of the table; radii (int32 [n]) masks, None is dense. Returns the table after
    the step (new arrays; the gradients are shared)."""
    b1, b2, ob1, ob2, bc1, bc2s = scalars(beta1, beta2, step)
    eps = F(eps)
    out = []
    with np.errstate(all="ignore"):
        for r in rows:
            p, g, m, v = r["param"], r["grad"], r["exp_avg"], r["exp_avg_sq"]
            width = p.shape[1]
            ss, ss_head = r["lr"] / bc1, r["lr_head"] / bc1
            assert type(ss) is F and type(ss_head) is F
            rate = np.where(np.arange(width) < r["head"], ss_head, ss).astype(F)[None, :]
            m1 = (b1 * m) + (ob1 * g)
            v1 = (b2 * v) + ((ob2 * g) * g)
            d = (np.sqrt(v1) / bc2s) + eps
            p1 = p - (rate * (m1 / d))
            for x in (m1, v1, d, p1):
                assert x.dtype == F
            if radii is not None:
                vis = (np.asarray(radii) > 0)[:, None]
                p1, m1, v1 = np.where(vis, p1, p), np.where(vis, m1, m), np.where(vis, v1, v)
            out.append({**r, "param": p1, "exp_avg": m1, "exp_avg_sq": v1})
    return out


def reset_cap(max_opacity):
    mo = float(F(max_opacity))
    return F(math.log(mo / (1.0 - mo)))


def opacity_reset(logits, max_opacity=0.01, exp_avg=None, exp_avg_sq=None):
    """(logits', exp_avg', exp_avg_sq'): logit' = logit > cap ? cap : logit (a NaN stays), zeroed moments."""
    cap = reset_cap(max_opacity)
    with np.errstate(all="ignore"):
        out = np.where(logits > cap, cap, logits).astype(F)
    z = lambda a: None if a is None else np.zeros_like(a)  # noqa: E731
    return out, z(exp_avg), z(exp_avg_sq)


# ---------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------
# the reference trainer's rates: position 0.00016 (x extent 1), scaling 0.005, rotation 0.001, opacity 0.05 (the trainer's
# 0.025 since its sparse-Adam change; either serves), f_dc 0.0025 and f_rest 0.0025 / 20
TRAINER_LR = {48: (0.0025 / 20, 3, 0.0025), 27: (0.0025 / 20, 3, 0.0025), 3: (0.00016, 0, 0.0), 1: (0.05, 0, 0.0),
              4: (0.001, 0, 0.0)}


def gradients(rng, shape):
    """N(0, 1e-3) with 30 % exact zeros."""
    g = rng.normal(0.0, 1e-3, shape).astype(F)
    g[rng.random(shape) < 0.3] = 0
    return g


def make_rows(n, widths=(48, 3, 1, 4, 27), seed=1, heads=None, lrs=None, warm=True):
    """A table of one row per width: parameters N(0, 1), the gradients above; warm: moments as after some steps
    (positive exp_avg_sq, a quarter of its entries exactly zero together with their exp_avg)."""
    rng = np.random.default_rng(seed)
    rows = []
    for k, w in enumerate(widths):
        lr, head, lr_head = TRAINER_LR.get(w, (0.001, 0, 0.0))
        if heads is not None:
            head = heads[k]
            lr_head = 0.0025 if head else 0.0
        if lrs is not None:
            lr = lrs[k]
        p = rng.normal(0.0, 1.0, (n, w)).astype(F)
        g = gradients(rng, (n, w))
        if warm:
            m = rng.normal(0.0, 1e-3, (n, w)).astype(F)
            v = (rng.random((n, w)) * 1e-6).astype(F)
            cold = rng.random((n, w)) < 0.25
            m[cold] = 0
            v[cold] = 0
        else:
            m, v = np.zeros((n, w), F), np.zeros((n, w), F)
        rows.append(row(p, g, m, v, lr, head, lr_head))
    return rows


def make_radii(n, kind, seed=5):
    """third: a third invisible (0) and a few -1; none; all; alternate: visible and invisible in turn."""
    rng = np.random.default_rng(seed)
    radii = rng.integers(1, 50, n).astype(np.int32)
    if kind == "third":
        radii[rng.random(n) < 1 / 3] = 0
        radii[rng.random(n) < 0.05] = -1
        if n > 2:
            radii[0], radii[1] = 3, -1
    elif kind == "none":
        radii[:] = 0
        radii[::3] = -1
    elif kind == "alternate":
        radii[1::2] = 0
    else:
        assert kind == "all"
    return radii


def reset_case(n, seed=9):
    """Logits around the cap of 0.01: on it, one ulp below, one ulp above, a NaN, +-Inf, the rest N(-4.6, 2)."""
    rng = np.random.default_rng(seed)
    cap = reset_cap(0.01)
    x = rng.normal(float(cap), 2.0, n).astype(F)
    special = [cap, np.nextafter(cap, F(-np.inf)), np.nextafter(cap, F(np.inf)), F(np.nan), F(np.inf), F(-np.inf), F(0)]
    for k, s in enumerate(special[:n]):
        x[(k * 37) % n if n >= 7 * 37 else k] = s
    if n == 1:
        x[0] = np.nextafter(cap, F(np.inf))
    return x, (rng.normal(0, 1e-3, n).astype(F)), (rng.random(n) * 1e-6).astype(F)


def pack(rows, *, step, steps=1, beta1=0.9, beta2=0.999, eps=1e-15, radii=None):
    """The case file of tests/native/adam_host.cpp."""
    n = rows[0]["param"].shape[0]
    blob = np.asarray([n, len(rows), step, steps, radii is not None], np.uint32).tobytes()
    blob += np.asarray([beta1, beta2, eps], F).tobytes()
    for r in rows:
        blob += np.asarray([r["param"].shape[1], r["head"]], np.uint32).tobytes()
        blob += np.asarray([r["lr"], r["lr_head"]], F).tobytes()
    if radii is not None:
        blob += np.asarray(radii, np.int32).tobytes()
    for r in rows:
        for k in ("param", "grad", "exp_avg", "exp_avg_sq"):
            blob += r[k].tobytes()
    return blob
