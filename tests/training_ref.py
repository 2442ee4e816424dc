"""float64 restatements of the training-side kernels (csrc/gsr_optim.hip, csrc/gsr_activations.hip), each with the per-element
error scale its float32 kernel is held to, and the seeded inputs that tests/test_training_ref.py (CPU) and
tests/test_gpu_training_kernels.py (GPU) share.  Plain torch in float64: no GPU is needed and no kernel of the package is imported.

Every input is the float32 value the kernel reads, widened to float64.  The scalars the C code rounds to float32 are rounded the same
way here (beta1, beta2, eps, lr, 1.f - beta, float(lr / bc1), float(1 / sqrt(bc2)), kNormalizeEps = 1e-12f), so what is left between
a kernel and its restatement is the kernel's own float32 arithmetic.  A bound reads |got - ref64| <= K * u * S per element, u = 2^-24;
every scale S has a floor of one smallest normal float32, so a flushed subnormal is not reported as a defect.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126                     # smallest normal float32
ADAM_ITEM = 4096                       # floats per work item of k_adam_multi
NORMALIZE_EPS = float(np.float32(1e-12))

# Ceilings: the roundings (each at most u, relative) of the kernels' expressions without contraction.
#   m' = m + (g - m)(1 - b1): the difference, the product and the sum, each at most u S_m: 3.
#   v' = v b2 + ((1 - b2) g) g: four roundings of non-negative terms: 4.
#   p' = p - st (m' / (sqrt(v') ib + eps)): the last rounding is u |p'|; the update carries m' (3, which is why U is built on S_m), v' through
#        the root (4 / 2), the root, the product with ib, the sum with eps, the quotient, the product with st, and the roundings of
#        float(lr / bc1) and float(1 / sqrt(bc2)): 12.
#   activations forward: the 4 * finfo.eps of tests/test_gpu_model.py.  backward: g s rounds once; g (1 - o) o three times; the
#   quaternion's n (2.5 u) enters cubed behind a 4-term dot product (4), 1 / n_c, three products, a quotient and the final fma: 16.
#   densify: gx gx + gy gy (2 / 2 through the root), the root and the sum, relative to a non-negative result: 3.
CEIL = {"adam_m": 3, "adam_v": 4, "adam_p": 12, "act_fwd": 8, "d_scaling": 1, "d_opacity": 3, "d_rotation": 16, "densify_accum": 3}

# Asserted K = ceil(2 x the worst ratio measured on an MI355X), capped at the ceiling.  The measurements are tabulated in the docstring of
# tests/test_gpu_training_kernels.py.
K = {"adam_m": 3, "adam_v": 4, "adam_p": 8, "act_fwd": 7, "d_scaling": 1, "d_opacity": 3, "d_rotation": 16, "densify_accum": 3}

ADAM_SIZES = (1, 3, 4, 5, 4095, 4096, 4097, 4098, 8194)
ADAM_ROW_LENS = (4, 5, 12, 27, 48)
ADAM_STEPS = (1, 2, 7, 10 ** 6)
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-15
ADAM_WRAP_PLAIN = 4096 * 256 * 4 + 1024 + 3                # gsr_adam_step: 1025 work items and a 3-float tail
ADAM_WRAP_SPLIT = (155_401, 27)                            # gsr_adam_step_split: 4 195 827 floats, 3-float tail
# (n, row_len, split, step, lr, lr_tail, seed) of one launch: eight tensors, one of them empty, each with its own step count and learning
# rates; tail-only items in the middle of the item list
ADAM_EIGHT = [(4098, 0, 0, 1, 0.01, 0.01, 1), (0, 0, 0, 2, 0.02, 0.02, 2), (1, 0, 0, 7, 0.03, 0.03, 3), (8194, 0, 0, 10 ** 6, 0.04, 0.04, 4),
              (4095, 0, 0, 3, 0.05, 0.05, 5), (153 * 27, 27, 3, 5, 0.0025, 0.000125, 6), (821 * 5, 5, 4, 2, 0.06, 0.001, 7), (3, 0, 0, 1000, 0.07, 0.07, 8)]
ACT_SIZES = (1, 2, 3, 6, 1000, 2_098_179)                  # the last: all three block ranges wrap, P % 4 = 3, 3P % 4 = 1
DENSIFY_SIZES = (1, 255, 256, 257, 1000)


def f32(x) -> float:
    return float(np.float32(x))


def adam_splits(row_len):
    return sorted({0, 1, 3, row_len - 1, row_len})


def adam_split_rows(row_len):
    """Rows of a split tensor whose n crosses the end of the first work item."""
    return ADAM_ITEM // row_len + 2


def adam_scalars(lr, lr_tail, step, b1, b2, eps, round_derived=True):
    """The kernel arguments as gsr_adam_step* derive them.  round_derived=False keeps lr / bc1 and 1 / sqrt(bc2) in float64, as
    torch.optim.Adam has them."""
    b1f, b2f = f32(b1), f32(b2)
    bc1, bc2 = 1.0 - math.pow(b1f, float(step)), 1.0 - math.pow(b2f, float(step))
    head, tail, inv = f32(lr) / bc1, f32(lr_tail) / bc1, 1.0 / math.sqrt(bc2)
    if round_derived:
        head, tail, inv = f32(head), f32(tail), f32(inv)
    return SimpleNamespace(b2=b2f, omb1=float(np.float32(1) - np.float32(b1)), omb2=float(np.float32(1) - np.float32(b2)), eps=f32(eps),
                           head=head, tail=tail, inv=inv, bc1=bc1, bc2=bc2)


def adam_step64(p, g, m, v, lr, lr_tail, step, row_len, split, b1, b2, eps, index0=0, round_derived=True):
    """One Adam step on flat views of (p, g, m, v): ((p', m', v'), (S_m, S_v, (|p'|, U))), float64 on the inputs' device.
    row_len = 0: one learning rate; else element i (+ index0, for a chunk of a larger tensor) is column (i % row_len) and columns below `split`
    step with lr, the others with lr_tail.  S_m = |m| + |g - m| (1 - b1); S_v = v'; U is the update with S_m in place of |m'|."""
    s = adam_scalars(lr, lr_tail, step, b1, b2, eps, round_derived)
    p, g, m, v = (t.detach().reshape(-1).double() for t in (p, g, m, v))
    m1 = m + (g - m) * s.omb1
    v1 = v * s.b2 + s.omb2 * g * g
    if row_len:
        col = (torch.arange(p.numel(), device=p.device, dtype=torch.int64) + index0) % row_len
        st = torch.where(col < split, torch.tensor(s.head, dtype=torch.float64, device=p.device), torch.tensor(s.tail, dtype=torch.float64, device=p.device))
    else:
        st = s.head
    den = v1.sqrt() * s.inv + s.eps
    p1 = p - st * (m1 / den)
    S_m = (m.abs() + (g - m).abs() * s.omb1).clamp_min(TINY)
    return (p1, m1, v1), (S_m, v1.clamp_min(TINY), (p1.abs(), (st * S_m / den).clamp_min(TINY)))


def activations64(scaling, rotation, opacity):
    """(exp, normalize, sigmoid) and their scales exp(x), |v_i| / n_c, sigmoid(x)."""
    x, q, o = (t.detach().double() for t in (scaling, rotation, opacity))
    nc = q.norm(dim=-1, keepdim=True).clamp_min(NORMALIZE_EPS)
    vals = (x.exp(), q / nc, torch.sigmoid(o))
    return vals, (vals[0].clamp_min(TINY), (q.abs() / nc).clamp_min(TINY), vals[2].clamp_min(TINY))


def activations_backward64(scales, rotation, opacities, g_scales, g_rotations, g_opacities):
    """The backward of k_act_bwd on what it reads (the forward's scales and opacities, the raw quaternion): values and scales
    |g s|, |g (1 - o) o| and |g_i| / n_c + |v_i| sum_j |v_j g_j| / (n n_c^2), the second term only where n >= eps."""
    s, q, o, gs, gq, go = (t.detach().double() for t in (scales, rotation, opacities, g_scales, g_rotations, g_opacities))
    n = q.norm(dim=-1, keepdim=True)
    nc = n.clamp_min(NORMALIZE_EPS)
    live = n >= NORMALIZE_EPS
    safe = torch.where(n > 0, n, torch.ones_like(n))
    k = torch.where(live, (q * gq).sum(-1, keepdim=True) / (safe * nc * nc), torch.zeros_like(n))
    k_abs = torch.where(live, (q * gq).abs().sum(-1, keepdim=True) / (safe * nc * nc), torch.zeros_like(n))
    vals = (gs * s, gq / nc - q * k, go * (1.0 - o) * o)
    scl = (vals[0].abs().clamp_min(TINY), (gq.abs() / nc + q.abs() * k_abs).clamp_min(TINY), vals[2].abs().clamp_min(TINY))
    return vals, scl


def densify_stats64(radii, vs_grad, max_radii2D, accum, denom):
    """k_densify_stats: where radii > 0, max_radii2D = max(., float32(radii)), accum += |grad.xy|, denom += 1; other rows as they were.
    Returns the three results (float64, flat) and the scale of accum (its non-negative result)."""
    vis = radii.reshape(-1) > 0
    r = radii.reshape(-1).to(torch.float32).double()                 # (float)r: 2^24 + 1 rounds to 2^24
    mr, acc, den = (t.detach().reshape(-1).double() for t in (max_radii2D, accum, denom))
    gx, gy = vs_grad.detach()[:, 0].double(), vs_grad.detach()[:, 1].double()
    norm = torch.where(vis, (gx * gx + gy * gy).sqrt(), torch.zeros_like(gx))      # a hidden row's gradient is not read
    mr1 = torch.where(vis, torch.maximum(mr, r), mr)
    acc1 = torch.where(vis, acc + norm, acc)
    den1 = torch.where(vis, den + 1.0, den)
    return (mr1, acc1, den1), acc1.abs().clamp_min(TINY)


def worst(got, ref, scale) -> float:
    """max |got - ref| / (u scale); NaN if got holds one where ref does not."""
    return float(((got.detach().reshape(-1).double() - ref.reshape(-1)).abs() / (U * scale.reshape(-1))).max())


def worst_p(got, ref, scales) -> float:
    """The Adam parameter's bound u |p'| + K u U solved for K: max (|got - ref| - u |p'|)+ / (u U)."""
    absp, upd = scales
    err = (got.detach().reshape(-1).double() - ref.reshape(-1)).abs()
    over = torch.where(torch.isnan(err), err, (err - U * absp.reshape(-1)).clamp_min(0.0))
    return float((over / (U * upd.reshape(-1))).max())


def bits_equal(a, b) -> bool:
    return a.shape == b.shape and bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---- the seeded inputs the CPU and the GPU tests share ---------------------------------------------------------------------------
def adam_state(n, seed):
    """A mid-training state of n floats on the host: p ~ N(0, 1), g ~ N(0, 1), m ~ 0.1 N, v = (0.03 N)^2.  From 8 floats on, the first three
    and the last three elements are planted: g = m = v = 0;  g = 0, v = 0, m != 0;  |g| = 1e3."""
    gen = torch.Generator().manual_seed(seed)
    p, g = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    m, v = 0.1 * torch.randn(n, generator=gen), (0.03 * torch.randn(n, generator=gen)) ** 2
    if n >= 8:
        for base in (0, n - 3):
            g[base] = m[base] = v[base] = 0.0
            g[base + 1] = v[base + 1] = 0.0
            m[base + 1] = 0.05 if base else -0.05
            g[base + 2] = -1e3 if base else 1e3
    return p, g, m, v


def adam_cases():
    """(n, row_len, split, step, lr, lr_tail, seed): every small one-tensor case of the CPU and the GPU tests: the work-item geometry of
    k_adam_multi with one learning rate, and split tensors [rows, row_len] whose n crosses an item end."""
    cases = []
    for n in ADAM_SIZES:
        for step in ADAM_STEPS:
            cases.append((n, 0, 0, step, 0.01, 0.01, 7 * n + step % 97))
    for row_len in ADAM_ROW_LENS:
        for split in adam_splits(row_len):
            for step in ADAM_STEPS:
                cases.append((adam_split_rows(row_len) * row_len, row_len, split, step, 0.0025, 0.000125, 1000 * row_len + 10 * split + step % 97))
    return cases


def adam_planted(n):
    """Indices of the elements with g = m = v = 0."""
    return [0, n - 3] if n >= 8 else []


def activation_inputs(P, seed):
    """Raw (scaling, rotation, opacity) and the three incoming gradients, on the host.  The edge rows are those of
    tests/test_gpu_model.py::_raw plus a quaternion of mixed magnitudes."""
    g = torch.Generator().manual_seed(seed)
    scaling = (torch.randn(P, 3, generator=g) * 2.0 - 3.0)
    rotation = torch.randn(P, 4, generator=g)
    opacity = torch.randn(P, 1, generator=g) * 4.0
    if P >= 8:
        rotation[0] = 0.0                                   # |q| = 0: normalize divides by eps, gradient g / eps
        rotation[1] = torch.tensor([1e-13, 0.0, 0.0, 0.0])   # below eps
        rotation[2] = torch.tensor([3e-12, 0.0, 0.0, 0.0])   # just above eps
        rotation[3] = torch.tensor([1e10, -1e10, 1e10, 1e10])
        opacity[4], opacity[5] = 40.0, -40.0                # saturated sigmoid
        scaling[6] = torch.tensor([-30.0, 0.0, 20.0])
        rotation[7] = torch.tensor([1e-6, 1.0, -1e3, 1e6])
    gen = torch.Generator().manual_seed(seed + 1)
    grads = [torch.randn(P, c, generator=gen) for c in (3, 4, 1)]
    return (scaling, rotation, opacity), grads


def densify_inputs(P, seed):
    """(radii, viewspace gradient, max_radii2D, xyz_gradient_accum, denom) on the host: radii with negatives, zeros, positives and 2^24 + 1;
    NaN in every hidden row's gradient and in column 2 of every row; non-trivial prior contents."""
    g = torch.Generator().manual_seed(seed)
    radii = torch.randint(-3, 40, (P,), generator=g, dtype=torch.int64).to(torch.int32)
    radii[P - 1] = 2 ** 24 + 1
    if P >= 4:
        radii[0], radii[1], radii[2] = -7, 0, 2 ** 24 + 1
    grad = torch.randn(P, 3, generator=g)
    grad[:, 2] = float("nan")
    grad[radii <= 0] = float("nan")
    max_radii = torch.rand(P, generator=g) * 50.0
    if P >= 4:
        max_radii[2] = 3e7                                   # above float32(2^24 + 1): the prior stays
    accum = torch.rand(P, 1, generator=g) * 3.0
    denom = torch.randint(0, 100, (P, 1), generator=g).float()
    return radii, grad, max_radii, accum, denom
