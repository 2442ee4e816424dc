"""The MCMC densification strategy's four operations on the raw parameter tensors ("3D Gaussian Splatting as Markov Chain Monte
Carlo"; gsplat's MCMCStrategy): the relocation rule, the row edit that applies it, the position noise, the regulariser gradient.
DESIGN section 16; C ABI: include/gsrast.h gsr_mcmc_*.

Device tensors run the HIP kernels (csrc/gsr_mcmc.hip); host tensors, and `native=False`, take the same rules as torch ops (the
relocation rule in binary64, cast at the end).  `native=True` on host tensors raises: there is no silent fallback.  Every native
in-place write bumps the tensor's autograd version (the activation cache of scene.GaussianModel keys on versions).
"""
from __future__ import annotations

import math

import torch

MAX_RATIO = 51                     # GSR_MCMC_MAX_RATIO
NOISE_K, NOISE_X0 = 100.0, 0.995   # g(o) = sigmoid(-k ((1 - o) - x0)) = 1 / (1 + exp(100 o - 0.5))
ROLES = ("copy", "opacity", "scaling")


def _use_native(native, t: torch.Tensor, what: str) -> bool:
    if native is None:
        return t.is_cuda
    if native and not t.is_cuda:
        raise RuntimeError(f"{what}: native=True needs device tensors (the HIP kernels have no CPU path)")
    return bool(native)


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 tensor, got {t.dtype} (contiguous: {t.is_contiguous()})")
    return t


def relocation_torch(opacity_raw, scaling_raw, sampled, min_opacity):
    """The rule in binary64 torch ops -> (new_opacity_raw [n], new_scaling_raw [n,3]) float32."""
    P = opacity_raw.shape[0]
    x = opacity_raw.detach().reshape(P).double()
    counts = torch.bincount(sampled, minlength=P)[sampled]
    N = (1 + counts).clamp(max=MAX_RATIO).double()
    xs = x[sampled]
    o, om = torch.sigmoid(xs), torch.sigmoid(-xs)
    log_om1 = torch.log(om) / N
    o1 = -torch.expm1(log_om1)
    D, c, pw = torch.zeros_like(o1), torch.ones_like(o1), torch.ones_like(o1)
    for j in range(1, MAX_RATIO + 1):
        c = c * (N - j + 1).clamp(min=0) / j          # C(N, j): zero from j = N + 1 on
        pw = pw * o1
        D = D + (c * pw / math.sqrt(j) if j & 1 else -(c * pw / math.sqrt(j)))
    lo = float(torch.tensor(min_opacity, dtype=torch.float32))
    hi = 1.0 - 2.0 ** -23
    logit = torch.where(o1 < lo, torch.full_like(o1, math.log(lo) - math.log1p(-lo)),
                        torch.where(o1 > hi, torch.full_like(o1, math.log(hi) - math.log1p(-hi)), torch.log(o1) - log_om1))
    new_s = scaling_raw.detach()[sampled].double() + torch.log(o / D)[:, None]
    return logit.float(), new_s.float()


def compute_relocation(opacity_raw, scaling_raw, sampled, min_opacity, native=None):
    """sampled [n] int64: one entry per Gaussian that becomes a copy of that source.  Returns (new_opacity_raw [n],
    new_scaling_raw [n,3]) for the sources, from their current values, with N = min(51, 1 + occurrences in `sampled`).
    Nothing is written."""
    if not 0.0 < float(min_opacity) < 1.0:
        raise ValueError(f"compute_relocation: min_opacity = {min_opacity} is outside (0, 1)")
    if sampled.dtype != torch.int64 or sampled.dim() != 1:
        raise TypeError(f"compute_relocation: sampled must be a [n] int64 tensor, got {sampled.dtype} {tuple(sampled.shape)}")
    if _use_native(native, opacity_raw, "compute_relocation"):
        from . import _native
        return _native.mcmc_relocation(_f32c(opacity_raw.detach(), "opacity_raw"), _f32c(scaling_raw.detach(), "scaling_raw"),
                                       sampled.contiguous(), float(min_opacity))
    return relocation_torch(opacity_raw, scaling_raw, sampled, min_opacity)


def relocate_rows(tensors, sampled, dead, new_opacity_raw, new_scaling_raw, native=None):
    """tensors: tuples (param [P, ...], exp_avg or None, exp_avg_sq or None, role), role in ROLES.  Source rows `sampled` take the new
    values ("opacity": new_opacity_raw, "scaling": new_scaling_raw, "copy": unchanged); with `dead` ([n] int64, rows disjoint from
    the sources) row dead[j] of every tensor becomes the updated row sampled[j] and the sources' moments are zeroed; with dead = None
    only the new values are written.  In place."""
    if not tensors or sampled.numel() == 0:
        return
    for p, m, v, role in tensors:
        if role not in ROLES:
            raise ValueError(f"relocate_rows: role {role!r} is none of {ROLES}")
        if (m is None) != (v is None):
            raise ValueError("relocate_rows: exp_avg and exp_avg_sq are both given or both None")
    P = int(tensors[0][0].shape[0])
    if _use_native(native, tensors[0][0], "relocate_rows"):
        from . import _native
        items = [(_f32c(p.detach(), "param"), None if m is None else _f32c(m, "exp_avg"), None if v is None else _f32c(v, "exp_avg_sq"), role)
                 for p, m, v, role in tensors]
        _native.mcmc_relocate_rows(items, P, sampled.contiguous(), None if dead is None else dead.contiguous(),
                                   _f32c(new_opacity_raw, "new_opacity_raw"), _f32c(new_scaling_raw, "new_scaling_raw"))
        for p, m, v, role in tensors:
            written = [p] if (dead is not None or role != "copy") else []
            if dead is not None and m is not None:
                written += [m, v]
            for t in written:
                torch.autograd.graph.increment_version(t)
        return
    with torch.no_grad():
        for p, m, v, role in tensors:
            if role == "opacity":
                p[sampled] = new_opacity_raw.reshape(-1, *p.shape[1:])
            elif role == "scaling":
                p[sampled] = new_scaling_raw
            if dead is not None:
                p[dead] = p[sampled]
                if m is not None:
                    m[sampled] = 0
                    v[sampled] = 0


def position_noise_torch(scaling_raw, rotation_raw, opacity_raw, noise, c):
    """The noise rule as torch ops in the tensors' dtype -> delta [P,3]."""
    o = torch.sigmoid(opacity_raw.reshape(-1, 1))
    g = 1.0 / (1.0 + torch.exp(NOISE_K * o - (NOISE_K * (1.0 - NOISE_X0))))
    q = rotation_raw / rotation_raw.norm(dim=1, keepdim=True).clamp_min(1e-12)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    s2 = torch.exp(scaling_raw) ** 2
    w = noise * (g * c)
    v = torch.bmm(R.transpose(1, 2), w.unsqueeze(-1)).squeeze(-1) * s2
    delta = torch.bmm(R, v.unsqueeze(-1)).squeeze(-1)
    return torch.where(g > 0, delta, torch.zeros_like(delta))        # an overflowed exp: exactly zero, whatever s^2 is


def inject_position_noise(xyz, scaling_raw, rotation_raw, opacity_raw, noise, c, native=None):
    """xyz += R diag(s^2) R^T (noise g(o) c), in place.  noise [P,3]: the caller's standard-normal draw; c: host scalar."""
    if noise.shape != xyz.shape:
        raise ValueError(f"inject_position_noise: noise {tuple(noise.shape)} is not shaped like xyz {tuple(xyz.shape)}")
    if xyz.shape[0] == 0:
        return
    if _use_native(native, xyz, "inject_position_noise"):
        from . import _native
        _native.mcmc_inject_noise(_f32c(xyz.detach(), "xyz"), _f32c(scaling_raw.detach(), "scaling_raw"), _f32c(rotation_raw.detach(), "rotation_raw"),
                                  _f32c(opacity_raw.detach(), "opacity_raw"), _f32c(noise, "noise"), float(c))
        torch.autograd.graph.increment_version(xyz)
        return
    with torch.no_grad():
        xyz.add_(position_noise_torch(scaling_raw.detach(), rotation_raw.detach(), opacity_raw.detach(), noise, float(c)))


def add_regularizer_grads(opacity_raw, scaling_raw, lambda_opacity, lambda_scale, grad_opacity, grad_scaling, native=None):
    """grad_opacity += lambda_opacity / P o (1 - o),  grad_scaling += lambda_scale / (3 P) s, in place: the gradients of
    lambda_opacity mean(o) + lambda_scale mean(s) on the raw tensors.  Either gradient may be None.  The loss value is not computed."""
    some = grad_opacity if grad_opacity is not None else grad_scaling
    if some is None or some.shape[0] == 0:
        return
    P = some.shape[0]
    if _use_native(native, some, "add_regularizer_grads"):
        from . import _native
        _native.mcmc_reg_grads(None if grad_opacity is None else _f32c(opacity_raw.detach(), "opacity_raw"),
                               None if grad_scaling is None else _f32c(scaling_raw.detach(), "scaling_raw"),
                               float(lambda_opacity), float(lambda_scale),
                               None if grad_opacity is None else _f32c(grad_opacity, "grad_opacity"),
                               None if grad_scaling is None else _f32c(grad_scaling, "grad_scaling"))
        for t in (grad_opacity, grad_scaling):
            if t is not None:
                torch.autograd.graph.increment_version(t)
        return
    with torch.no_grad():
        if grad_opacity is not None:
            x = opacity_raw.detach()
            grad_opacity.add_((torch.sigmoid(x) * torch.sigmoid(-x)).reshape(grad_opacity.shape) * (float(lambda_opacity) / P))
        if grad_scaling is not None:
            grad_scaling.add_(torch.exp(scaling_raw.detach()) * (float(lambda_scale) / (3 * P)))
