"""Normal maps for surface regularisation: the normal-consistency term that 2DGS, Gaussian Opacity Fields, RaDe-GS, PGSR, DN-Splatter
and gsplat's 2DGS trainer share.  Three ops, each one HIP launch forward and one backward (csrc/gsr_normals.hip, DESIGN section 23;
C ABI: include/gsrast_normals.h):

  gaussian_normals          per-Gaussian normals in the view space: the shortest axis, turned to the camera
  depth_to_normal           the normal map implied by the rendered depth (the maps of depth_alpha=True)
  normal_consistency_loss   mean(1 - alpha <N, n>), fused: the depth normals n are never stored

fp32 contiguous device tensors run the kernels; everything else, and `native=False`, takes the same rule as torch ops (`*_torch`, in
the tensors' own dtype).  `native=True` on host tensors raises: there is no silent fallback.  The native gradients are sums in an
order the program fixes: the same inputs give the same bits.

Conventions: row-vector matrices (p_view = p @ V[:3,:3] + V[3,:3]); fx = W / (2 tanfovx), fy = H / (2 tanfovy); pixel (x, y) has its
centre at x + 0.5, so px = x + 0.5 - W/2 and py = y + 0.5 - H/2; the view space is x right, y down, z forward; quaternions are
(w, x, y, z) with upstream's build_rotation.  Normals point at the camera: a fronto-parallel surface gives (0, 0, -1).
"""
from __future__ import annotations

import numpy as np
import torch

ALPHA_MIN = 1.0 / 255.0          # the blend's own alpha cut-off


def _use_native(native, t: torch.Tensor, what: str) -> bool:
    on_gpu = t.is_cuda and t.dtype == torch.float32
    if native is None:
        return on_gpu
    if native and not on_gpu:
        raise RuntimeError(f"{what}: native=True needs fp32 device tensors (the HIP kernels have no CPU path)")
    return bool(native)


def _same(what: str, first_name: str, first: torch.Tensor, **others) -> None:
    """One device, one float dtype, contiguous: loud, not a quiet copy or a trip through the twin."""
    for name, t in ((first_name, first),) + tuple(others.items()):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
        if not t.dtype.is_floating_point or t.dtype != first.dtype or t.device != first.device:
            raise ValueError(f"{what}: {name} is {t.dtype} on {t.device}, {first_name} {first.dtype} on {first.device}: "
                             "one device and one float dtype expected")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous")


def _refuse_camera_grad(what: str, *tensors) -> None:
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise ValueError(f"{what}: the camera is read as a constant and receives no gradient; a viewmatrix or campos that requires grad "
                         "is not supported (detach them)")


# ---- per-Gaussian normals ------------------------------------------------------------------------------------------------------------

def _check_gaussians(what, scales, rotations, means3D, viewmatrix, campos):
    if scales.dim() != 2 or scales.shape[1] != 3:
        raise ValueError(f"{what}: scales [P,3] expected, got {tuple(scales.shape)}")
    P = scales.shape[0]
    if tuple(rotations.shape) != (P, 4):
        raise ValueError(f"{what}: rotations [P,4] expected for P = {P}, got {tuple(rotations.shape)}")
    if tuple(means3D.shape) != (P, 3):
        raise ValueError(f"{what}: means3D [P,3] expected for P = {P}, got {tuple(means3D.shape)}")
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix [4,4] expected, got {tuple(viewmatrix.shape)}")
    if campos.numel() != 3:
        raise ValueError(f"{what}: campos [3] expected, got {tuple(campos.shape)}")
    _same(what, "scales", scales, rotations=rotations, means3D=means3D, viewmatrix=viewmatrix, campos=campos)
    _refuse_camera_grad(what, viewmatrix, campos)


def shortest_axis(scales):
    """argmin over the three scales, ties to the lowest index, as the kernel takes it."""
    k = (scales[:, 1] < scales[:, 0]).long()
    return torch.where(scales[:, 2] < scales.gather(1, k[:, None])[:, 0], torch.full_like(k, 2), k)


def gaussian_normals_torch(scales, rotations, means3D, viewmatrix, campos):
    """The rule as torch ops in the tensors' dtype, differentiable in `rotations` through autograd."""
    _check_gaussians("gaussian_normals_torch", scales, rotations, means3D, viewmatrix, campos)
    u = rotations / rotations.norm(dim=1, keepdim=True)
    r, x, y, z = u.unbind(1)
    R = torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), 1).view(-1, 3, 3)
    k = shortest_axis(scales.detach())
    n_w = R.gather(2, k[:, None, None].expand(-1, 3, 1))[:, :, 0]
    facing_away = (n_w.detach() * (means3D.detach() - campos.detach().reshape(1, 3))).sum(1) > 0
    n_w = torch.where(facing_away[:, None], -n_w, n_w)
    return n_w @ viewmatrix.detach()[:3, :3]


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scales, rotations, means3D, viewmatrix, campos):
        from . import _native
        inputs = (scales, rotations, means3D, viewmatrix, campos)
        if ctx.needs_input_grad[1]:
            ctx.save_for_backward(*inputs)                   # the backward recomputes the axis and the sign: nothing else is kept
        return _native.gaussian_normals_forward(*inputs)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        if not ctx.needs_input_grad[1]:
            return None, None, None, None, None
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.float().contiguous()
        return None, _native.gaussian_normals_backward(*ctx.saved_tensors, grad_out), None, None, None


def gaussian_normals(scales, rotations, means3D, viewmatrix, campos, native=None):
    """-> [P,3], the Gaussians' normals in the view space.  Per Gaussian: k = argmin_j scales[p, j] (ties to the lowest j), n_w = column k
    of R(q / |q|), turned to the camera (n_w = -n_w when <n_w, means3D_p - campos> > 0; exactly 0 does not flip), out = n_w @ V[:3,:3].
    `scales` may be scales or log-scales and `rotations` raw or unit quaternions, so one op serves forward and forward_raw callers.
    Differentiable in `rotations` only (k and the sign are piecewise constant: `scales` and `means3D` receive None); the camera is a
    constant, and a viewmatrix or campos that requires grad is a ValueError."""
    _check_gaussians("gaussian_normals", scales, rotations, means3D, viewmatrix, campos)
    if _use_native(native, scales, "gaussian_normals"):
        return _GaussianNormals.apply(scales.detach(), rotations, means3D.detach(), viewmatrix.detach(), campos.detach().reshape(3))
    return gaussian_normals_torch(scales, rotations, means3D, viewmatrix, campos)


# ---- depth normals and the consistency loss ------------------------------------------------------------------------------------------

def _check_maps(what, depth, alpha, tanfovx, tanfovy, alpha_min, normal_map=None):
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[0] != 1):
        raise ValueError(f"{what}: depth [1,H,W] or [H,W] expected, got {tuple(depth.shape)}")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if alpha.dim() not in (2, 3) or tuple(alpha.shape[-2:]) != (H, W) or alpha.numel() != H * W:
        raise ValueError(f"{what}: alpha [1,H,W] or [H,W] expected for H, W = {H}, {W}, got {tuple(alpha.shape)}")
    others = {"alpha": alpha}
    if normal_map is not None:
        if tuple(normal_map.shape) != (3, H, W):
            raise ValueError(f"{what}: normal_map [3,H,W] expected for H, W = {H}, {W}, got {tuple(normal_map.shape)}")
        others["normal_map"] = normal_map
    _same(what, "depth", depth, **others)
    if not (tanfovx > 0 and tanfovy > 0 and alpha_min > 0 and np.isfinite([tanfovx, tanfovy, alpha_min]).all()):
        raise ValueError(f"{what}: tanfovx = {tanfovx}, tanfovy = {tanfovy}, alpha_min = {alpha_min}: positive and finite expected")
    return H, W


def _focal(n, tanfov, dtype):
    """n / (2 tanfov) as the kernel rounds it in binary32, or in binary64."""
    if dtype == torch.float32:
        return float(np.float32(n) / (np.float32(2.0) * np.float32(tanfov)))
    return n / (2.0 * tanfov)


def depth_to_normal_torch(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN):
    """The rule as torch ops in the tensors' dtype (shifted slices of the depth and the closed form of the kernel), differentiable in
    `depth` and `alpha` through autograd."""
    H, W = _check_maps("depth_to_normal_torch", depth, alpha, tanfovx, tanfovy, alpha_min)
    d2, a2 = depth.reshape(H, W), alpha.reshape(H, W)
    dt, dev = depth.dtype, depth.device
    valid = (a2 >= float(np.float32(alpha_min))) & (d2 > 0)                    # (the cut-off is a binary32 number in every dtype)
    one = torch.ones_like(d2)
    z = torch.where(valid, d2, one) / torch.where(valid, a2, one)              # (a placeholder of 1 where invalid: never used)
    if H < 3 or W < 3:                                                         # every pixel is on the border
        return torch.zeros(3, H, W, dtype=dt, device=dev) + 0 * z.sum()
    ok = valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
    zl, zr, zu, zd = z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
    Dx, Sx, Dy, Sy = zr - zl, zr + zl, zd - zu, zd + zu
    px = (torch.arange(1, W - 1, dtype=dt, device=dev) + 0.5 - 0.5 * W).view(1, W - 2)
    py = (torch.arange(1, H - 1, dtype=dt, device=dev) + 0.5 - 0.5 * H).view(H - 2, 1)
    a, b = Sy * Dx, Sx * Dy
    m = torch.stack((_focal(W, tanfovx, dt) * a, _focal(H, tanfovy, dt) * b, -(Sx * Sy + px * a + py * b)))
    n = m / m.square().sum(0, keepdim=True).sqrt()
    n = torch.where(ok[None], n, torch.zeros_like(n))
    return torch.nn.functional.pad(n, (1, 1, 1, 1))


def normal_consistency_loss_torch(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN):
    """The loss as torch ops in the tensors' dtype: depth_to_normal_torch and the mean of 1 - alpha.detach() <N, n>."""
    H, W = _check_maps("normal_consistency_loss_torch", depth, alpha, tanfovx, tanfovy, alpha_min, normal_map)
    if H * W == 0:
        raise ValueError("normal_consistency_loss: an image without pixels has no mean")
    n = depth_to_normal_torch(depth, alpha, tanfovx, tanfovy, alpha_min)
    return (1 - alpha.detach().reshape(H, W) * (normal_map * n).sum(0)).mean()


class _DepthToNormal(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, alpha, tanfovx, tanfovy, alpha_min):
        from . import _native
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(depth, alpha)
        ctx.consts = (tanfovx, tanfovy, alpha_min)
        return _native.depth_normal_forward(depth, alpha, tanfovx, tanfovy, alpha_min)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        want = tuple(ctx.needs_input_grad[:2])
        if not any(want):
            return None, None, None, None, None
        depth, alpha = ctx.saved_tensors
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.float().contiguous()
        return _native.depth_normal_backward(depth, alpha, *ctx.consts, grad_out, want) + (None, None, None)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normal_map, depth, alpha, tanfovx, tanfovy, alpha_min):
        from . import _native
        if any(ctx.needs_input_grad[:3]):
            ctx.save_for_backward(normal_map, depth, alpha)
        ctx.consts = (tanfovx, tanfovy, alpha_min)
        return _native.normal_consistency_forward(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        want = tuple(ctx.needs_input_grad[:3])
        if not any(want):
            return None, None, None, None, None, None
        normal_map, depth, alpha = ctx.saved_tensors
        grads = _native.normal_consistency_backward(normal_map, depth, alpha, *ctx.consts, grad_out.float().reshape(1).contiguous(), want)
        return grads + (None, None, None)


def depth_to_normal(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN, native=None):
    """-> [3,H,W], the normal map implied by a rendered depth.  `depth` and `alpha` are the [1,H,W] (or [H,W]) maps of depth_alpha=True
    (`depth` the unnormalised weighted sum).  A pixel is valid when alpha >= alpha_min and depth > 0, and then z = depth / alpha.  The
    output at (x, y) is non-zero only at an interior pixel whose four axis neighbours are valid:
        m = (fx Sy Dx, fy Sx Dy, -(Sx Sy + px Sy Dx + py Sx Dy)),  n = m / |m|
    with Dx, Sx the difference and sum of z at (x+1, y) and (x-1, y), and Dy, Sy likewise along y; +0.0 everywhere else, where no
    gradient flows.  Differentiable in `depth` and `alpha`; the native backward is a gather without atomics."""
    _check_maps("depth_to_normal", depth, alpha, tanfovx, tanfovy, alpha_min)
    if _use_native(native, depth, "depth_to_normal"):
        return _DepthToNormal.apply(depth, alpha, float(tanfovx), float(tanfovy), float(alpha_min))
    return depth_to_normal_torch(depth, alpha, tanfovx, tanfovy, alpha_min)


def normal_consistency_loss(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN, native=None):
    """-> the 0-dim loss (1 / (H W)) sum_p (1 - alpha_p <N_p, n_p>): N = normal_map [3,H,W], the rendered alpha-weighted normals (not
    normalised), n the map of depth_to_normal (never stored on the native path; a pixel without one adds 1), alpha a constant as a
    factor (2DGS's rend_alpha.detach()) and differentiated through z.  Differentiable in `normal_map`, `depth` and `alpha`."""
    H, W = _check_maps("normal_consistency_loss", depth, alpha, tanfovx, tanfovy, alpha_min, normal_map)
    if H * W == 0:
        raise ValueError("normal_consistency_loss: an image without pixels has no mean")
    if _use_native(native, depth, "normal_consistency_loss"):
        return _NormalConsistency.apply(normal_map, depth, alpha, float(tanfovx), float(tanfovy), float(alpha_min))
    return normal_consistency_loss_torch(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min)


def surface_depth(depth, alpha, median, depth_ratio):
    """2DGS's depth_ratio mix as a depth map of the kind `depth` is: (1 - r) depth + r alpha median, UNNORMALISED (depth = sum w z, median
    = the rasterizer's median_depth map, a plain depth), so that depth_to_normal, normal_consistency_loss and TSDFVolume.integrate take
    it beside the same alpha unchanged: their z = D / alpha is (1 - r) mean + r median.  Plain torch ops, differentiable in all three
    maps.  r = 0 returns `depth` itself; r outside [0, 1] is a ValueError.  2DGS uses r = 1 for bounded scenes, 0 for unbounded ones."""
    r = float(depth_ratio)
    if not 0.0 <= r <= 1.0:
        raise ValueError(f"surface_depth: depth_ratio {r} outside [0, 1]")
    if r == 0.0:
        return depth
    if depth.shape != alpha.shape or depth.shape != median.shape:
        raise ValueError(f"surface_depth: depth {tuple(depth.shape)}, alpha {tuple(alpha.shape)}, median {tuple(median.shape)}: one shape expected")
    if r == 1.0:
        return alpha * median
    return (1.0 - r) * depth + r * (alpha * median)
