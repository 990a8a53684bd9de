"""Float64 reference of the 3DGS training loss (ptgs_image_loss_l1_dssim, contract in include/ptgs/ptgs.h):

    loss = (1 - lam) * mean|a - b| + lam * (1 - mean SSIM(a, b))

with the 11 x 11 Gaussian window (sigma 1.5), zero padding of 5 and no renormalisation at the border, and its
analytic gradient with respect to the image. The convolution is the direct 121-tap 2-D form (the kernels and
the host restatement are separable). The inputs are the float32 arrays the kernels see, upcast, so sign(a - b)
is decided identically. eager() is the same loss through torch's F.conv2d and autograd on the CPU, in float64
(a check of this file) or float32 (the scale of float32 rounding that the tolerances are derived from).
"""
import numpy as np

WIN, HALO = 11, 5
C1, C2 = 0.01 ** 2, 0.03 ** 2


def window():
    k = np.arange(WIN, dtype=np.float64)
    g = np.exp(-((k - HALO) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def conv(x):
    """Correlation of the last two axes of x with w = g (x) g, zero padding of 5: 121 shifted adds."""
    g = window()
    H, W = x.shape[-2:]
    pad = np.zeros(x.shape[:-2] + (H + 2 * HALO, W + 2 * HALO), np.float64)
    pad[..., HALO:HALO + H, HALO:HALO + W] = x
    out = np.zeros(x.shape, np.float64)
    for i in range(WIN):
        for j in range(WIN):
            out += (g[i] * g[j]) * pad[..., i:i + H, j:j + W]
    return out


def parts(image, target):
    """What does not depend on lam: l1, ssim, sign(a - b) and G, the last two [H, W, 3]."""
    a = np.moveaxis(np.asarray(image)[..., :3].astype(np.float64), -1, 0)
    b = np.moveaxis(np.asarray(target)[..., :3].astype(np.float64), -1, 0)
    mu1, mu2, e11, e22, e12 = conv(np.stack([a, b, a * a, b * b, a * b]))
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A = 2.0 * mu1 * mu2 + C1
    B = 2.0 * s12 + C2
    Cc = mu1 * mu1 + mu2 * mu2 + C1
    D = s1 + s2 + C2
    m = A * B / (Cc * D)
    d_s1 = -m / D
    d_s12 = 2.0 * A / (Cc * D)
    d_mu1 = 2.0 * mu2 * B / (Cc * D) - 2.0 * mu1 * m / Cc - 2.0 * mu1 * d_s1 - mu2 * d_s12
    c_mu1, c_s1, c_s12 = conv(np.stack([d_mu1, d_s1, d_s12]))
    G = c_mu1 + 2.0 * a * c_s1 + b * c_s12
    return {"l1": float(np.abs(a - b).mean()), "ssim": float(m.mean()), "n": a.size,
            "sign": np.moveaxis(np.sign(a - b), 0, -1), "G": np.moveaxis(G, 0, -1)}


def combine(p, lam=0.2, grad_scale=1.0):
    """(loss, l1, ssim, grad [H, W, 4]) of parts() for one lam and grad_scale."""
    loss = (1.0 - lam) * p["l1"] + lam * (1.0 - p["ssim"])
    g3 = grad_scale * ((1.0 - lam) / p["n"] * p["sign"] - lam / p["n"] * p["G"])
    grad = np.zeros(g3.shape[:2] + (4,), np.float64)
    grad[..., :3] = g3
    return loss, p["l1"], p["ssim"], grad


def loss_and_grad(image, target, lam=0.2, grad_scale=1.0):
    return combine(parts(image, target), lam, grad_scale)


def loss_only(image, target, lam=0.2):
    """The loss alone, for finite differences (image and target float64)."""
    a = np.moveaxis(np.asarray(image, np.float64)[..., :3], -1, 0)
    b = np.moveaxis(np.asarray(target, np.float64)[..., :3], -1, 0)
    mu1, mu2, e11, e22, e12 = conv(np.stack([a, b, a * a, b * b, a * b]))
    s1, s2, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    m = (2.0 * mu1 * mu2 + C1) * (2.0 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    return (1.0 - lam) * np.abs(a - b).mean() + lam * (1.0 - m.mean())


def eager(image, target, lam=0.2, grad_scale=1.0, dtype="float64"):
    """The F.conv2d formulation on the CPU with torch autograd: (loss, l1, ssim, grad [H, W, 4]) as float64
    numpy values of a computation carried out in `dtype`."""
    import torch
    import torch.nn.functional as F
    dt = getattr(torch, dtype)
    g = torch.from_numpy(window()).to(dt)
    w = (g[:, None] * g[None, :]).expand(3, 1, WIN, WIN).contiguous()
    img = torch.from_numpy(np.ascontiguousarray(image)).to(dt).requires_grad_(True)
    a = img[..., :3].permute(2, 0, 1)[None]
    b = torch.from_numpy(np.ascontiguousarray(np.asarray(target)[..., :3])).to(dt).permute(2, 0, 1)[None]

    def cv(x):
        return F.conv2d(x, w, padding=HALO, groups=3)

    mu1, mu2 = cv(a), cv(b)
    s1, s2, s12 = cv(a * a) - mu1 * mu1, cv(b * b) - mu2 * mu2, cv(a * b) - mu1 * mu2
    m = (2 * mu1 * mu2 + C1) * (2 * s12 + C2) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s1 + s2 + C2))
    l1, ssim = (a - b).abs().mean(), m.mean()
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    (loss * grad_scale).backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), img.grad.double().numpy()


def make_inputs(H, W, C=3, seed=0):
    """(image [H, W, 4], target [H, W, C]) float32: target = rand, image = clamp(target + 0.1 randn, 0, 1.2), and
    a flat 0.5 block pasted into both, shifted by half its size in the target, so the two blocks partly overlap:
    windows where both variances vanish, and pixels with a - b exactly 0. The alpha channels are noise."""
    rng = np.random.default_rng([seed, H, W])
    t3 = rng.random((H, W, 3), dtype=np.float32)
    a3 = np.clip(t3 + np.float32(0.1) * rng.standard_normal((H, W, 3), dtype=np.float32), 0.0, 1.2).astype(np.float32)
    bh, bw = max(1, H // 2), max(1, W // 2)
    y0, x0 = H // 4, W // 4
    a3[y0:y0 + bh, x0:x0 + bw] = 0.5
    t3[y0 + (bh + 1) // 2:y0 + (bh + 1) // 2 + bh, x0 + (bw + 1) // 2:x0 + (bw + 1) // 2 + bw] = 0.5
    image = np.concatenate([a3, rng.random((H, W, 1), dtype=np.float32)], axis=2)
    target = t3 if C == 3 else np.concatenate([t3, rng.random((H, W, 1), dtype=np.float32)], axis=2)
    return np.ascontiguousarray(image), np.ascontiguousarray(target)


def rel_l2(x, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(np.asarray(x, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def rel(x, ref):
    return abs(float(x) - float(ref)) / max(abs(float(ref)), 1e-300)
