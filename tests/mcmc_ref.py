"""Binary64 restatement of the MCMC strategy's four rules, in numpy, and the error rules the kernels, their host
twins and the package's torch path are held to.  Written from the rules as stated, not from the kernels: the relocation sum is the
double sum over (i, k) with exact integer binomials, where csrc/gsr_math.h collapses it to one sum.

  relocation   o' = 1 - (1 - o)^(1/N),  D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k (k+1)^(-1/2) o'^(k+1),
               opacity_raw' = logit(clamp(o', min_opacity, 1 - 2^-23)),  scaling_raw' = scaling_raw + log(o / D);  N clamped to
               1 .. 51; N = 1 is the identity (the inputs as they are)
  noise        xyz + R(q^) diag(s^2) R(q^)^T (xi g(o) c),  g(o) = 1 / (1 + exp(100 o - 0.5)),  q^ = q / max(|q|, 1e-12)
  reg grads    grad_opacity + lambda_o / P o (1 - o),   grad_scaling + lambda_s / (3 P) s
"""
import math

import numpy as np

MAX_RATIO = 51
F64 = np.float64


def sigmoid(x):
    """Binary64 sigmoid without overflow: 1 / (1 + exp(-x)) for x >= 0, exp(x) / (1 + exp(x)) below."""
    x = np.asarray(x, F64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def clamp_ratio(N):
    return np.clip(np.asarray(N, np.int64), 1, MAX_RATIO)


def relocated_opacity(o_minus, N):
    """o' = 1 - (1 - o)^(1/N) from 1 - o, through expm1 so that a small o keeps its digits."""
    return -np.expm1(np.log(o_minus) / N)


def denominator(o1, N):
    """D for an array o' and one integer N: the double sum as stated."""
    o1 = np.asarray(o1, F64)
    D = np.zeros_like(o1)
    for i in range(1, N + 1):
        for k in range(i):
            D = D + math.comb(i - 1, k) * (-1.0) ** k / math.sqrt(k + 1) * o1 ** (k + 1)
    return D


def relocation(opacity_raw, scaling_raw, N, min_opacity):
    """opacity_raw [n], scaling_raw [n,3], N [n] integers (any >= 1) -> (opacity_raw' [n], scaling_raw' [n,3]) in binary64.
    min_opacity is taken at binary32 precision, as the C ABI passes it."""
    x = np.asarray(opacity_raw, F64).reshape(-1)
    ls = np.asarray(scaling_raw, F64).reshape(-1, 3)
    N = clamp_ratio(np.broadcast_to(N, x.shape))
    lo, hi = float(np.float32(min_opacity)), 1.0 - 2.0 ** -23
    out_o, out_s = x.copy(), ls.copy()
    for n in np.unique(N):
        if n == 1:
            continue
        m = N == n
        o, om = sigmoid(x[m]), sigmoid(-x[m])
        o1 = relocated_opacity(om, int(n))
        D = denominator(o1, int(n))
        oc = np.clip(o1, lo, hi)
        # logit of the clamped value; unclamped, 1 - o' = (1 - o)^(1/N) is known without a subtraction
        logit = np.where(o1 < lo, math.log(lo) - math.log1p(-lo),
                         np.where(o1 > hi, math.log(hi) - math.log1p(-hi), np.log(oc) - np.log(om) / n))
        out_o[m] = logit
        out_s[m] = ls[m] + np.log(o / D)[:, None]
    return out_o, out_s


def multiplicity(sampled, P):
    """N_j = 1 + occurrences of sampled[j] in sampled (unclamped)."""
    sampled = np.asarray(sampled, np.int64)
    return 1 + np.bincount(sampled, minlength=P)[sampled]


def gate(o):
    """g(o) = 1 / (1 + exp(100 o - 0.5))."""
    return sigmoid(-(100.0 * np.asarray(o, F64) - 0.5))


def rotmat(q):
    q = np.asarray(q, F64)
    n = np.maximum(np.sqrt((q * q).sum(1, keepdims=True)), 1e-12)
    r, x, y, z = (q / n).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)


def noise_delta(scaling_raw, rotation_raw, opacity_raw, noise, c):
    R = rotmat(rotation_raw)
    s2 = np.exp(2.0 * np.asarray(scaling_raw, F64))
    g = gate(sigmoid(np.asarray(opacity_raw, F64).reshape(-1)))
    w = np.asarray(noise, F64) * (g * float(c))[:, None]
    v = np.einsum("pji,pj->pi", R, w) * s2
    return np.einsum("pij,pj->pi", R, v)


def noise(xyz, scaling_raw, rotation_raw, opacity_raw, xi, c):
    return np.asarray(xyz, F64) + noise_delta(scaling_raw, rotation_raw, opacity_raw, xi, c)


def noise_bound(xyz, scaling_raw, opacity_raw, xi, c):
    """|out - ref| <= 1e-4 S_i + 1.2e-7 |xyz_ij|,  S_i = c g(o_i) |xi_i| max_j s_ij^2.  First term: g inherits 100 x the binary32
    sigmoid's absolute error (2e-7): 2e-5 relative; the covariance product a few 1e-6 of max s^2; together ~3e-5, bound 3x that.
    Second term: the rounding of the final add."""
    g = gate(sigmoid(np.asarray(opacity_raw, F64).reshape(-1)))
    S = abs(float(c)) * g * np.sqrt((np.asarray(xi, F64) ** 2).sum(1)) * np.exp(2.0 * np.asarray(scaling_raw, F64)).max(1)
    return 1e-4 * S[:, None] + 1.2e-7 * np.abs(np.asarray(xyz, F64))


def reg_delta(opacity_raw, scaling_raw, lam_o, lam_s):
    """(d opacity [P], d scaling [P,3]): what the rule adds to the two gradients."""
    x = np.asarray(opacity_raw, F64).reshape(-1)
    P = x.shape[0]
    return float(lam_o) / P * sigmoid(x) * sigmoid(-x), float(lam_s) / (3 * P) * np.exp(np.asarray(scaling_raw, F64))


# ---- error rules ----------------------------------------------------------------------------------------------------------------------
def check_relocation(out_o, out_s, ref_o, ref_s, what=""):
    """|out - ref| <= 2.4e-7 max(1, |ref|): binary64 arithmetic (error < 1e-12) and one rounding to binary32 (0.5 ulp); 2 ulp."""
    worst = 0.0
    for name, out, ref in (("opacity", out_o, ref_o), ("scaling", out_s, ref_s)):
        out, ref = np.asarray(out, F64).reshape(-1), np.asarray(ref, F64).reshape(-1)
        assert out.shape == ref.shape, (what, name, out.shape, ref.shape)
        assert np.isfinite(out).all(), f"{what} {name}: non-finite output"
        ratio = np.abs(out - ref) / (2.4e-7 * np.maximum(1.0, np.abs(ref)))
        k = int(ratio.argmax()) if ratio.size else 0
        assert ratio.size == 0 or ratio[k] <= 1.0, f"{what} {name}[{k}]: {out[k]!r} vs {ref[k]!r} ({ratio[k]:.2f} x the bound)"
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
    return worst


def check_noise(out, xyz, scaling_raw, rotation_raw, opacity_raw, xi, c, what=""):
    out = np.asarray(out, F64)
    assert np.isfinite(out).all(), f"{what}: non-finite xyz"
    ref = noise(xyz, scaling_raw, rotation_raw, opacity_raw, xi, c)
    ratio = np.abs(out - ref) / np.maximum(noise_bound(xyz, scaling_raw, opacity_raw, xi, c), 1e-300)
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    assert ratio[k] <= 1.0, f"{what} row {k[0]} col {k[1]}: {out[k]!r} vs {ref[k]!r} ({ratio[k]:.2f} x the bound)"
    return float(ratio.max())


def check_reg(delta, ref, grad_in, what=""):
    """|delta - ref| <= 1e-6 |ref| + 1.2e-7 |grad_in|, delta = grad_out - grad_in."""
    delta, ref, grad_in = (np.asarray(a, F64).reshape(-1) for a in (delta, ref, grad_in))
    assert np.isfinite(delta).all(), f"{what}: non-finite gradient"
    bound = 1e-6 * np.abs(ref) + 1.2e-7 * np.abs(grad_in)
    ratio = np.abs(delta - ref) / np.maximum(bound, 1e-300)
    k = int(ratio.argmax())
    assert ratio[k] <= 1.0, f"{what}[{k}]: {delta[k]!r} vs {ref[k]!r} ({ratio[k]:.2f} x the bound)"
    return float(ratio.max())


# ---- shared inputs ----------------------------------------------------------------------------------------------------------------------
def quaternions(P, rng):
    """Unnormalised quaternions of norm 1e-3 .. 1e3 (log-uniform); row 0 (P > 1: row 1) has norm 0."""
    q = rng.standard_normal((P, 4))
    q /= np.sqrt((q * q).sum(1, keepdims=True))
    q *= 10.0 ** rng.uniform(-3, 3, (P, 1))
    q[min(1, P - 1)] = 0.0
    return q.astype(np.float32)


def noise_inputs(P, seed):
    """float32 arrays (xyz, scaling_raw, rotation_raw, opacity_raw [P,1], xi): logits in [-30, 30] with every fourth row near
    o = 0.005 (logit -5.29 +- 1: the gate is not saturated there), log-scales in [-8, 3], the quaternion set above."""
    rng = np.random.default_rng(seed)
    logit = rng.uniform(-30, 30, P)
    near = np.arange(P) % 4 == 0
    logit[near] = math.log(0.005 / 0.995) + rng.uniform(-1, 1, int(near.sum()))
    if P > 2:
        logit[2] = 30.0                                       # o = 1 in binary32: the exponential overflows, g = 0
    xyz = rng.uniform(-3, 3, (P, 3))
    xyz[np.abs(xyz) < 1e-3] = 0.5
    return (xyz.astype(np.float32), rng.uniform(-8, 3, (P, 3)).astype(np.float32), quaternions(P, rng),
            logit.astype(np.float32).reshape(P, 1), rng.standard_normal((P, 3)).astype(np.float32))


def relocation_inputs(P, seed):
    """float32 (opacity_raw [P,1], scaling_raw [P,3]) with o spread over [0.005, 0.99999] (uniform in the logit)."""
    rng = np.random.default_rng(seed)
    lo, hi = math.log(0.005 / 0.995), math.log(0.99999 / 0.00001)
    return rng.uniform(lo, hi, (P, 1)).astype(np.float32), rng.uniform(-8, 3, (P, 3)).astype(np.float32)
