"""The depth-distortion loss: Mip-NeRF 360's regulariser in the squared form that 2DGS trains with (and gsplat's 2DGS trainer, RaDe-GS
and PGSR after it).  Per pixel, over the splats the colour composites, with w_i = alpha_i T_i and a per-splat depth value m_i:

    D = sum_{i<j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,    A = sum w_i,  M1 = sum w_i m_i,  M2 = sum w_i m_i^2

A is the alpha map of depth_alpha=True; M1 and M2 are two linear channels, which `extra_colors` blends inside the colour frame with
gradients.  Three ops (csrc/gsr_distortion.hip; C ABI: include/gsrast_distortion.h):

  depth_moments      per Gaussian (m, m^2, 0): the rows to pass as extra_colors
  distortion_map     D per pixel from the rendered moments map ("extra") and "alpha"
  distortion_loss    mean(D), fused: the map is never stored

fp32 device tensors run the kernels; everything else, and `native=False`, takes the same rule as torch ops (`*_torch`, in the tensors'
own dtype).  `native=True` on host tensors raises: there is no silent fallback.  Non-contiguous inputs are made contiguous.  The native
sums have an order the program fixes: the same inputs give the same bits.

The depth value: z is the view depth of means3D under viewmatrix (row-vector convention, z = (p @ V[:3,:3] + V[3,:3])[2]: the quantity
the depth map blends).  mapping="ndc" (the default, 2DGS's choice): m = far (z - near) / ((far - near) z), the depth of the projection
matrix, in [0, 1) - which bounds the cancellation of A M2 - M1^2 in binary32; mapping="linear" (gsplat's): m = z.
Where z <= near (ndc) or z <= 0 (linear), m = +0.0 and no gradient flows; the frame culls such a Gaussian anyway.
"""
from __future__ import annotations

import numpy as np
import torch

from .normals import _refuse_camera_grad, _use_native

NEAR, FAR = 0.2, 100.0           # 2DGS's planes
MAPPINGS = ("ndc", "linear")


# ---- per-Gaussian depth moments --------------------------------------------------------------------------------------------------------

def _check_moments(what, means3D, viewmatrix, near, far, mapping):
    for name, t in (("means3D", means3D), ("viewmatrix", viewmatrix)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if means3D.dim() != 2 or means3D.shape[1] != 3:
        raise ValueError(f"{what}: means3D [P,3] expected, got {tuple(means3D.shape)}")
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix [4,4] expected, got {tuple(viewmatrix.shape)}")
    if not means3D.dtype.is_floating_point or viewmatrix.dtype != means3D.dtype:
        raise ValueError(f"{what}: means3D is {means3D.dtype}, viewmatrix {viewmatrix.dtype}: one float dtype expected")
    if viewmatrix.device != means3D.device:
        raise ValueError(f"{what}: means3D is on {means3D.device}, viewmatrix on {viewmatrix.device}: one device expected")
    if mapping not in MAPPINGS:
        raise ValueError(f"{what}: mapping = {mapping!r}: one of {', '.join(repr(m) for m in MAPPINGS)}")
    near, far = float(near), float(far)
    if not (near > 0 and far > near and np.isfinite(far)):
        raise ValueError(f"{what}: near = {near}, far = {far}: 0 < near < far, finite, expected")
    _refuse_camera_grad(what, viewmatrix)
    return near, far


def _planes(near, far, dtype):
    """near, far as the kernel holds them: binary32 numbers in every dtype but binary64's own."""
    if dtype == torch.float64:
        return near, far
    return float(np.float32(near)), float(np.float32(far))


def depth_moments_torch(means3D, viewmatrix, near=NEAR, far=FAR, mapping="ndc"):
    """The rule as torch ops in the tensors' dtype, differentiable in `means3D` through autograd."""
    near, far = _check_moments("depth_moments_torch", means3D, viewmatrix, near, far, mapping)
    near, far = _planes(near, far, means3D.dtype)
    V = viewmatrix.detach()
    z = means3D[:, 0] * V[0, 2] + means3D[:, 1] * V[1, 2] + means3D[:, 2] * V[2, 2] + V[3, 2]
    front = z.detach() > (near if mapping == "ndc" else 0.0)
    zs = torch.where(front, z, torch.ones_like(z))                       # (a placeholder of 1 where culled: never used)
    m = (far * (zs - near)) / ((far - near) * zs) if mapping == "ndc" else zs
    m = torch.where(front, m, torch.zeros_like(m))
    return torch.stack((m, m * m, torch.zeros_like(m)), 1)


class _DepthMoments(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, viewmatrix, mapping, near, far):
        from . import _native
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(means3D, viewmatrix)               # the backward recomputes z and m: nothing else is kept
        ctx.consts = (mapping, near, far)
        return _native.depth_moments_forward(means3D, viewmatrix, mapping, near, far)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.float().contiguous()
        return _native.depth_moments_backward(*ctx.saved_tensors, *ctx.consts, grad_out), None, None, None, None


def depth_moments(means3D, viewmatrix, near=NEAR, far=FAR, mapping="ndc", native=None):
    """-> [P,3] = (m, m^2, +0.0) per Gaussian, the rows to render as `extra_colors` beside depth_alpha=True: the "extra" map is then
    (M1, M2, 0).  m by `mapping` from the view depth z of means3D (module docstring); near and far are read under either mapping
    (0 < near < far).  Differentiable in `means3D`; the camera is a constant, and a viewmatrix that requires grad is a ValueError."""
    near, far = _check_moments("depth_moments", means3D, viewmatrix, near, far, mapping)
    if _use_native(native, means3D, "depth_moments"):
        from ._native import DISTORTION_MAPPINGS
        return _DepthMoments.apply(means3D.contiguous(), viewmatrix.detach().contiguous(), DISTORTION_MAPPINGS[mapping], near, far)
    return depth_moments_torch(means3D, viewmatrix, near, far, mapping)


# ---- the map and the loss ---------------------------------------------------------------------------------------------------------------

def _check_maps(what, moments_map, alpha):
    for name, t in (("moments_map", moments_map), ("alpha", alpha)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if moments_map.dim() != 3 or moments_map.shape[0] != 3:
        raise ValueError(f"{what}: moments_map [3,H,W] expected, got {tuple(moments_map.shape)}")
    H, W = int(moments_map.shape[1]), int(moments_map.shape[2])
    if alpha.dim() not in (2, 3) or tuple(alpha.shape[-2:]) != (H, W) or alpha.numel() != H * W:
        raise ValueError(f"{what}: alpha [1,H,W] or [H,W] expected for H, W = {H}, {W}, got {tuple(alpha.shape)}")
    if not moments_map.dtype.is_floating_point or alpha.dtype != moments_map.dtype:
        raise ValueError(f"{what}: moments_map is {moments_map.dtype}, alpha {alpha.dtype}: one float dtype expected")
    if alpha.device != moments_map.device:
        raise ValueError(f"{what}: moments_map is on {moments_map.device}, alpha on {alpha.device}: one device expected")
    return H, W


def distortion_map_torch(moments_map, alpha):
    """The rule as torch ops in the tensors' dtype: A M2 - M1^2, [1,H,W], differentiable through autograd."""
    H, W = _check_maps("distortion_map_torch", moments_map, alpha)
    return (alpha.reshape(H, W) * moments_map[1] - moments_map[0] * moments_map[0])[None]


def distortion_loss_torch(moments_map, alpha):
    """The loss as torch ops in the tensors' dtype: the mean of distortion_map_torch."""
    H, W = _check_maps("distortion_loss_torch", moments_map, alpha)
    if H * W == 0:
        raise ValueError("distortion_loss: an image without pixels has no mean")
    return distortion_map_torch(moments_map, alpha).mean()


class _DistortionMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, moments_map, alpha):
        from . import _native
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(moments_map, alpha)
        return _native.distortion_map_forward(moments_map, alpha)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        want = tuple(ctx.needs_input_grad)
        if not any(want):
            return None, None
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.float().contiguous()
        return _native.distortion_map_backward(*ctx.saved_tensors, grad_out, want)


class _DistortionLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, moments_map, alpha):
        from . import _native
        if any(ctx.needs_input_grad):
            ctx.save_for_backward(moments_map, alpha)
        return _native.distortion_loss_forward(moments_map, alpha)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        want = tuple(ctx.needs_input_grad)
        if not any(want):
            return None, None
        return _native.distortion_loss_backward(*ctx.saved_tensors, grad_out.float().reshape(1).contiguous(), want)


def distortion_map(moments_map, alpha, native=None):
    """-> [1,H,W], D = fma(A, M2, -(M1 M1)) per pixel, not clamped (a slightly negative value from binary32 cancellation stays, so the
    gradient is the formula's): M1, M2 = planes 0 and 1 of `moments_map` [3,H,W] (the "extra" map of a frame whose extra_colors are
    depth_moments(...); plane 2 is never read), A = `alpha` [1,H,W] or [H,W].  Differentiable in both: dA = g M2, dM1 = -2 g M1,
    dM2 = g A, plane 2's gradient +0.0."""
    _check_maps("distortion_map", moments_map, alpha)
    if _use_native(native, moments_map, "distortion_map"):
        return _DistortionMap.apply(moments_map.contiguous(), alpha.contiguous())
    return distortion_map_torch(moments_map, alpha)


def distortion_loss(moments_map, alpha, native=None):
    """-> the 0-dim loss mean(D) over the H W pixels, D as in distortion_map (never stored on the native path: sums of 1 024 pixels
    in binary32, then those in binary64, every order fixed).  Differentiable in `moments_map` and `alpha`."""
    H, W = _check_maps("distortion_loss", moments_map, alpha)
    if H * W == 0:
        raise ValueError("distortion_loss: an image without pixels has no mean")
    if _use_native(native, moments_map, "distortion_loss"):
        return _DistortionLoss.apply(moments_map.contiguous(), alpha.contiguous())
    return distortion_loss_torch(moments_map, alpha)
