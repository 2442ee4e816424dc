"""Binary64 reference of the fused L1 + D-SSIM loss (csrc/gsr_loss.hip) and a per-pixel checker for its kernels.

`ssim_l1_ref` evaluates the loss, the SSIM map, the three derivative maps the forward writes for the backward
(d_mu = dm/dmu1, d_eaa = dm/dE[a^2], d_eab = dm/dE[ab], the kernel's folded form) and the gradient with respect to the
image, in binary64.  Two windows:
  "separable"  the kernel's definition: zero-padded 11-tap row pass, then column pass, with the binary32 taps of
               make_window() promoted to binary64;
  "reference"  the 11x11 window of loss_utils._window (the binary32 outer product g g^T, rounded), promoted to binary64.
The two are not the same function: a rank-1 set of taps cannot reproduce the rounded 2-D window.

`rows=(y0, y1)` evaluates a row band: the outputs of rows [y0, y1) from input rows [y0 - 10, y1 + 10), maps for rows
[y0 - 5, y1 + 5) clipped to the image.  Every output element is computed by the same elementwise operations in the same
order as in a full-image evaluation, so a band is bit for bit the same rows of the full image.

`yardstick32` is the same separable algebra in plain binary32 (row pass, then column pass, taps added in order, products
formed once, the kernel's expression order, no FMA contraction): what binary32 reaches on the same inputs.

`check_loss` holds a device result to the yardstick, pixel by pixel:
    e_p = |g_dev - g_64| / (eps32 * S_p),   S_p = |k_ssim| (K|d_mu| + 2|a| K|d_eaa| + |b| K|d_eab|) + |k_l1|
the float64 sum of the absolute values of pixel p's gradient summands.  Near convergence the SSIM gradient is a sum of
terms near 1/C2 that cancel almost completely; a tensor-wide bound relative to max|g| then says nothing, this one stays
tight in every regime (a = b included).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = float(np.finfo(np.float32).eps)         # 2^-23
HALO = 5                                        # window radius
KC1 = float(np.float32(np.float32(0.01) * np.float32(0.01)))   # the kernel's kC1 = 0.01f * 0.01f
KC2 = float(np.float32(np.float32(0.03) * np.float32(0.03)))

# Caps of check_loss: the device may be this many times the yardstick's p50 / p99 / max, with absolute floors (in units of
# eps32 * magnitude).  The floors matter where the yardstick is exact on most pixels (a = b gives p50 = 0).
CAP_P50, CAP_P99, CAP_MAX = 4.0, 4.0, 8.0
FLOOR_P50, FLOOR_P99, FLOOR_MAX = 1.0, 8.0, 32.0
# Sums of |a - b| and of SSIM: |dev - f64| <= c * eps32 * sum|terms|, c = max(CAP_SUM * yardstick's ratio, SUM_FLOOR).
# The yardstick's ratio is that of the float64 sum of its binary32 per-pixel terms.  SUM_FLOOR covers the device's
# own binary32 summation (per-thread rows, block trees, the finish kernel's strided partial sums).
CAP_SUM = 4.0
SUM_FLOOR = 16.0


def kernel_taps() -> np.ndarray:
    """make_window() of csrc/gsr_loss.hip: exp in binary64 rounded to binary32, divided by their binary32 running sum."""
    g = [np.float32(math.exp(-float((i - 5) * (i - 5)) / (2.0 * 1.5 * 1.5))) for i in range(11)]
    s = np.float32(0.0)
    for v in g:
        s = np.float32(s + v)
    return np.array([np.float32(v / s) for v in g], dtype=np.float32)


def reference_window() -> np.ndarray:
    """loss_utils._window(11, 1): the binary32 outer product of the reference's taps, [11, 11]."""
    import loss_utils
    return loss_utils._window(11, 1)[0, 0].numpy()


def _as_t(x, dtype):
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))).detach().cpu().to(dtype)


def _ext_rows(x, y0, y1, pad):
    """Rows [y0 - pad, y1 + pad) of x [C, H, W], zero outside the image."""
    C, H, W = x.shape
    out = torch.zeros((C, y1 - y0 + 2 * pad, W), dtype=x.dtype)
    lo, hi = max(0, y0 - pad), min(H, y1 + pad)
    if hi > lo:
        out[:, lo - (y0 - pad):hi - (y0 - pad)] = x[:, lo:hi]
    return out


def _hpass(x, g):
    """Zero-padded 11-tap pass along the last axis, taps added in order from 0 (the kernel's `t = 0; t += g[i] * v[i]`)."""
    W = x.shape[-1]
    xp = F.pad(x, (HALO, HALO))
    out = torch.zeros_like(x)
    for i in range(11):
        out = out + g[i] * xp[..., i:i + W]
    return out


def _vpass(x, g):
    """11-tap pass along rows: [C, R, W] -> [C, R - 10, W] (the input carries its own 5-row halo)."""
    R = x.shape[1] - 2 * HALO
    out = torch.zeros((x.shape[0], R, x.shape[2]), dtype=x.dtype)
    for i in range(11):
        out = out + g[i] * x[:, i:i + R]
    return out


def _conv2d(x, w2):
    """The 11x11 window applied directly (121 taps): [C, R, W] -> [C, R - 10, W], zero-padded columns."""
    R, W = x.shape[1] - 2 * HALO, x.shape[2]
    xp = F.pad(x, (HALO, HALO))
    out = torch.zeros((x.shape[0], R, W), dtype=x.dtype)
    for i in range(11):
        for j in range(11):
            out = out + w2[i][j] * xp[:, i:i + R, j:j + W]
    return out


def _coefficients(C, H, W, lam, up, dtype):
    """k_ssim, k_l1 of k_loss_bwd.  binary32: the kernel's own float arithmetic; binary64: exact -lam up / n, (1 - lam) up / n."""
    if dtype == torch.float32:
        f = np.float32
        inv = f(1.0) / (f(C) * f(H) * f(W))
        return float(-f(lam) * inv * f(up)), float((f(1.0) - f(lam)) * inv * f(up))
    n = float(C) * H * W
    return -lam * up / n, (1.0 - lam) * up / n


class LossResult:
    """Fields (CPU tensors of the evaluation dtype, rows of the band):
    grad, ssim_map [C, y1 - y0, W]; d_mu, d_eaa, d_eab [C, me - mb, W] for map rows [mb, me) = [y0 - 5, y1 + 5) within the
    image; l1_sum, ssim_sum, l1_abs, ssim_abs (python floats over the band; *_abs = sum of |terms|); loss (whole image only).
    binary64 only: S (the gradient's magnitude S_p), T_mu / T_eaa / T_eab (each map's float64 magnitude of its own terms)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)


def _evaluate(a, b, lam, up, rows, dtype, window, consts, fault=None):
    a, b = _as_t(a, torch.float32), _as_t(b, torch.float32)       # the device's inputs are binary32
    C, H, W = a.shape
    y0, y1 = (0, H) if rows is None else (int(rows[0]), int(rows[1]))
    assert 0 <= y0 <= y1 <= H
    lam, up = float(np.float32(lam)), float(np.float32(up))       # the kernel receives both as binary32
    C1, C2 = consts if consts is not None else (KC1, KC2)
    if window == "separable":
        g = [float(v) for v in kernel_taps()]

        def K(x):
            return _vpass(_hpass(x, g), g)
    elif window == "reference":
        assert dtype == torch.float64
        w2 = [[float(v) for v in r] for r in reference_window()]

        def K(x):
            return _conv2d(x, w2)
    else:
        raise ValueError(window)
    if fault == "seam_tap":
        # planted fault: the outermost tap of the row pass is dropped for the pixels on a 32-px tile seam (x % 32 == 0)
        K_ok = K
        seam = (torch.arange(W) % 32 == 0)

        def K(x):
            gd = [0.0] + g[1:]
            return torch.where(seam, _vpass(_hpass(x, gd), g), K_ok(x))
    A, B = _ext_rows(a, y0, y1, 2 * HALO).to(dtype), _ext_rows(b, y0, y1, 2 * HALO).to(dtype)
    mu1, mu2 = K(A), K(B)                                         # rows [y0 - 5, y1 + 5)
    eaa, ebb, eab = K(A * A), K(B * B), K(A * B)
    s1, s2, s12 = eaa - mu1 * mu1, ebb - mu2 * mu2, eab - mu1 * mu2
    A1, A2 = 2.0 * mu1 * mu2 + C1, 2.0 * s12 + C2
    B1, B2 = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    inv = 1.0 / (B1 * B2)
    m = A1 * A2 * inv
    d_mu = 2.0 * mu2 * (A2 - A1) * inv - 2.0 * mu1 * m * (B2 - B1) * inv
    d_eaa = -m / B2
    d_eab = 2.0 * A1 * inv
    if fault == "map_ulp":
        d_eab = (d_eab.double() * (1.0 + 2.0 ** -16)).to(dtype)  # planted fault: one map off by a factor 1 + 2^-16
    # maps exist inside the image only (the backward's window sees zeros beyond it)
    yy = torch.arange(y0 - HALO, y1 + HALO)
    inside = ((yy >= 0) & (yy < H)).view(1, -1, 1)
    if fault == "slab_halo":
        inside = inside & ((yy >= y0) & (yy < y1)).view(1, -1, 1)   # planted fault: halo map rows outside the slab zeroed
    zero = torch.zeros((), dtype=dtype)
    maps = [torch.where(inside, d, zero) for d in (d_mu, d_eaa, d_eab)]
    k_ssim, k_l1 = _coefficients(C, H, W, lam, up, dtype)
    acc = [K(d) for d in maps]
    ac, bc = A[:, 2 * HALO:2 * HALO + y1 - y0], B[:, 2 * HALO:2 * HALO + y1 - y0]
    diff = ac - bc
    sgn = torch.sign(diff)
    if fault == "sign_tie":
        sgn = torch.where(diff >= 0, 1.0, -1.0).to(dtype)          # planted fault: sign(0) = +1
    grad = k_ssim * (acc[0] + 2.0 * ac * acc[1] + bc * acc[2]) + k_l1 * sgn
    if fault == "small_g":
        # planted fault: a 1e-3 relative error only where |g| < 1e-3 max|g|
        gm = float(grad.abs().max())
        grad = torch.where(grad.abs() < 1e-3 * gm, grad * (1.0 + 1e-3), grad)
    ssim_map = m[:, HALO:HALO + y1 - y0]
    l1 = diff.abs()
    mb, me = max(0, y0 - HALO), min(H, y1 + HALO)
    sl = slice(mb - (y0 - HALO), me - (y0 - HALO))
    n = float(C) * H * W
    r = LossResult(grad=grad, ssim_map=ssim_map, d_mu=maps[0][:, sl], d_eaa=maps[1][:, sl], d_eab=maps[2][:, sl],
                   map_rows=(mb, me), rows=(y0, y1), lam=lam, up=up, n=n,
                   l1_sum=float(l1.double().sum()), ssim_sum=float(ssim_map.double().sum()),
                   l1_abs=float(l1.double().sum()), ssim_abs=float(ssim_map.double().abs().sum()))
    if rows is None or (y0, y1) == (0, H):
        r.loss = (1.0 - lam) * r.l1_sum / n + lam * (1.0 - r.ssim_sum / n)
    if dtype == torch.float64:
        absK = [K(d.abs()) for d in maps]
        r.S = abs(k_ssim) * (absK[0] + 2.0 * ac.abs() * absK[1] + bc.abs() * absK[2]) + abs(k_l1)
        # each map's terms, with A2 = 2 s12 + C2 and B2 = s1 + s2 + C2 taken as the sums of their terms' magnitudes (A2, and
        # with it m and d_eaa, cancels to zero where s12 = -C2 / 2)
        A2m, B2m = 2.0 * s12.abs() + C2, s1.abs() + s2.abs() + C2
        T_mu = (2.0 * mu2).abs() * (A2m + A1.abs()) * inv.abs() + (2.0 * mu1).abs() * (A1 * A2m * inv).abs() * (B2m + B1.abs()) * inv.abs()
        T_eaa = (A1 * A2m * inv / B2).abs()
        r.T_mu, r.T_eaa, r.T_eab = T_mu[:, sl], T_eaa[:, sl], d_eab.abs()[:, sl]
    return r


def ssim_l1_ref(a, b, lam=0.2, up=1.0, window="separable", rows=None, consts=None) -> LossResult:
    """The loss (1 - lam) mean|a - b| + lam (1 - mean SSIM) and its pieces in binary64 (module docstring).  a, b: [C, H, W]
    binary32 arrays or tensors, any C.  consts: (C1, C2), default the kernel's binary32 constants."""
    return _evaluate(a, b, lam, up, rows, torch.float64, window, consts)


def yardstick32(a, b, lam=0.2, up=1.0, rows=None, fault=None) -> LossResult:
    """The kernel's separable algebra in plain binary32 (no FMA contraction, the kernel's expression order).
    fault: a planted fault for the checker's self-test ("seam_tap", "slab_halo", "small_g", "sign_tie", "map_ulp")."""
    return _evaluate(a, b, lam, up, rows, torch.float32, "separable", None, fault)


def ref_sums(a, b, band=256):
    """Whole-image sums (l1_sum, ssim_sum, ssim_abs) in binary64 and the yardstick's binary32 sums, band by band (forward
    only, for frames too large to hold the float64 planes): returns (f64 dict, yardstick dict)."""
    H = a.shape[1]
    f64 = dict(l1_sum=0.0, ssim_sum=0.0, ssim_abs=0.0)
    ys = dict(l1_sum=0.0, ssim_sum=0.0)
    for y0 in range(0, H, band):
        y1 = min(H, y0 + band)
        r = _forward_band(a, b, y0, y1, torch.float64)
        f64["l1_sum"] += float(r[0].sum())
        f64["ssim_sum"] += float(r[1].sum())
        f64["ssim_abs"] += float(r[1].abs().sum())
        r = _forward_band(a, b, y0, y1, torch.float32)
        ys["l1_sum"] += float(r[0].sum())
        ys["ssim_sum"] += float(r[1].sum())
    f64["l1_abs"] = f64["l1_sum"]
    return f64, ys


def _forward_band(a, b, y0, y1, dtype):
    a, b = _as_t(a, torch.float32), _as_t(b, torch.float32)
    g = [float(v) for v in kernel_taps()]

    def K(x):
        return _vpass(_hpass(x, g), g)
    A, B = _ext_rows(a, y0, y1, HALO).to(dtype), _ext_rows(b, y0, y1, HALO).to(dtype)
    mu1, mu2 = K(A), K(B)
    eaa, ebb, eab = K(A * A), K(B * B), K(A * B)
    s1, s2, s12 = eaa - mu1 * mu1, ebb - mu2 * mu2, eab - mu1 * mu2
    m = (2.0 * mu1 * mu2 + KC1) * (2.0 * s12 + KC2) * (1.0 / ((mu1 * mu1 + mu2 * mu2 + KC1) * (s1 + s2 + KC2)))
    return (A[:, HALO:-HALO] - B[:, HALO:-HALO]).abs(), m


# ---------------------------------------------------------------------------------------------------------------- checker

def _ratios(dev, want, scale):
    """|dev - want| / (eps32 * scale) per element; equal values give 0 where scale is 0, unequal or non-finite ones inf."""
    dev = _as_t(dev, torch.float64)
    want = want.double()
    d = (dev - want).abs()
    scale = scale.double()
    r = torch.where(scale > 0, d / (EPS32 * scale.clamp_min(1e-300)), torch.where(d == 0, 0.0, math.inf))
    return torch.where(torch.isfinite(dev), r, torch.full_like(r, math.inf)).flatten()


def _pct(r):
    if r.numel() == 0:
        return (0.0, 0.0, 0.0)
    r = r.double().numpy()
    if not np.isfinite(r).all():
        return (math.inf, math.inf, math.inf)
    p50, p99 = np.percentile(r, [50.0, 99.0])
    return (float(p50), float(p99), float(r.max()))


def _within(dev_stats, ys_stats):
    caps = (max(CAP_P50 * ys_stats[0], FLOOR_P50), max(CAP_P99 * ys_stats[1], FLOOR_P99), max(CAP_MAX * ys_stats[2], FLOOR_MAX))
    return all(d <= c for d, c in zip(dev_stats, caps)), caps


def per_pixel(dev, ref, ystick, field="grad"):
    """(device p50/p99/max, yardstick p50/p99/max) of field's normalised error; field: grad, d_mu, d_eaa or d_eab."""
    scale = {"grad": "S", "d_mu": "T_mu", "d_eaa": "T_eaa", "d_eab": "T_eab"}[field]
    want, s = getattr(ref, field), getattr(ref, scale)
    return _pct(_ratios(getattr(dev, field), want, s)), _pct(_ratios(getattr(ystick, field), want, s))


def sum_ratio(dev_sum, f64_sum, f64_abs):
    return abs(float(dev_sum) - f64_sum) / (EPS32 * max(f64_abs, 1e-300)) if f64_abs > 0 else (0.0 if dev_sum == f64_sum else math.inf)


def check_loss(dev, ref, ystick, label="", maps=True, sums=True, report=None):
    """Hold `dev` (an object with grad, and d_mu / d_eaa / d_eab / l1_sum / ssim_sum as requested, rows as `ref`) to the
    binary32 yardstick, against binary64 `ref`.  Raises AssertionError naming every field that fails; returns
    {field: (device stats, yardstick stats)}.  report: a list the rows of the per-pixel table are appended to."""
    out, bad = {}, []
    fields = ["grad"] + (["d_mu", "d_eaa", "d_eab"] if maps else [])
    for f in fields:
        d, y = per_pixel(dev, ref, ystick, f)
        ok, caps = _within(d, y)
        out[f] = (d, y)
        if not ok:
            bad.append(f"{f}: device p50/p99/max {d[0]:.3g}/{d[1]:.3g}/{d[2]:.3g} > caps {caps[0]:.3g}/{caps[1]:.3g}/{caps[2]:.3g}"
                       f" (yardstick {y[0]:.3g}/{y[1]:.3g}/{y[2]:.3g})")
    if sums:
        for f, fa in (("l1_sum", "l1_abs"), ("ssim_sum", "ssim_abs")):
            rd = sum_ratio(getattr(dev, f), getattr(ref, f), getattr(ref, fa))
            ry = sum_ratio(getattr(ystick, f), getattr(ref, f), getattr(ref, fa))
            cap = max(CAP_SUM * ry, SUM_FLOOR)
            out[f] = (rd, ry)
            if not rd <= cap:
                bad.append(f"{f}: device {rd:.3g} eps32 * sum|terms| > cap {cap:.3g} (yardstick {ry:.3g})")
    if report is not None:
        report.append((label, out))
    assert not bad, f"{label}: " + "; ".join(bad)
    return out


def format_row(label, out):
    parts = []
    for f, v in out.items():
        if f.endswith("_sum"):
            parts.append(f"{f} {v[0]:.2f}|{v[1]:.2f}")
        else:
            d, y = v
            parts.append(f"{f} {d[0]:.2f}/{d[1]:.2f}/{d[2]:.1f}|{y[0]:.2f}/{y[1]:.2f}/{y[2]:.1f}")
    return f"{label:<40s} " + "  ".join(parts)


# ---------------------------------------------------------------------------------------------------------------- inputs

def smooth_pair(C, H, W, sigma, seed=0):
    """A smooth image b in (0.1, 0.9) (a few low-frequency waves per channel) and a = b + sigma N(0, 1), both binary32."""
    g = torch.Generator().manual_seed(seed)
    y = torch.linspace(0.0, 1.0, H, dtype=torch.float64).view(-1, 1)
    x = torch.linspace(0.0, 1.0, W, dtype=torch.float64).view(1, -1)
    planes = []
    for _ in range(C):
        p = torch.zeros(H, W, dtype=torch.float64)
        for _k in range(3):
            fy, fx, ph = (torch.rand(3, generator=g, dtype=torch.float64) * torch.tensor([6.0, 6.0, 6.28], dtype=torch.float64)).tolist()
            p += torch.sin(fy * 3.14159 * y + fx * 3.14159 * x + ph)
        planes.append(0.5 + 0.4 * p / 3.0)
    b = torch.stack(planes).float()
    a = b if sigma == 0 else (b.double() + sigma * torch.randn(C, H, W, generator=g, dtype=torch.float64)).float()
    return a.contiguous(), b.contiguous()
