"""The per-image bilateral grid between the rasterizer and the loss (gsplat's lib_bilagrid, `use_bilateral_grid`): every training
image owns a [12, L, Gy, Gx] grid of 3x4 affine colour transforms indexed by pixel position and luma; the rendered image goes through
its grid before the loss, so that per-image exposure, white balance and vignetting are not baked into the Gaussians.  DESIGN section
17; C ABI: include/gsrast.h gsr_bilagrid_*.

Device tensors run the HIP kernels (csrc/gsr_bilagrid.hip); host tensors, and `native=False`, take the same rule as torch ops
(grid_sample on a 5-D input and the affine product).  `native=True` on host tensors raises: there is no silent fallback.  The native
gradients are sums in an order the program fixes: the same inputs give the same bits, which torch's grid_sample backward does not offer.
"""
from __future__ import annotations

import torch
from torch import nn
from torch.nn import functional as F

GRAY = (0.299, 0.587, 0.114)


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


def _check_shapes(grids, image, idx, what):
    if grids.dim() != 5 or grids.shape[1] != 12:
        raise ValueError(f"{what}: grids must be [N, 12, L, Gy, Gx], got {tuple(grids.shape)}")
    if image is not None and (image.dim() != 3 or image.shape[0] != 3):
        raise ValueError(f"{what}: image must be [3, H, W], got {tuple(image.shape)}")
    if idx is not None and not 0 <= int(idx) < grids.shape[0]:
        raise IndexError(f"{what}: idx = {idx} is outside [0, {grids.shape[0]})")


def slice_apply_torch(grids, image, idx):
    """The rule as torch ops in the tensors' dtype: grid_sample(bilinear, border, align_corners=True) of grids[idx] at (x, y, luma)
    and the affine product.  grids [N,12,L,Gy,Gx], image [3,H,W] -> [3,H,W]."""
    _check_shapes(grids, image, idx, "slice_apply_torch")
    _, H, W = image.shape
    dt, dev = image.dtype, image.device
    x = ((torch.arange(W, dtype=dt, device=dev) + 0.5) / W).view(1, W).expand(H, W)
    y = ((torch.arange(H, dtype=dt, device=dev) + 0.5) / H).view(H, 1).expand(H, W)
    gray = GRAY[0] * image[0] + GRAY[1] * image[1] + GRAY[2] * image[2]
    coords = (torch.stack((x, y, gray), -1) - 0.5) * 2.0                                 # [0, 1] -> grid_sample's [-1, 1]
    A = F.grid_sample(grids[int(idx)][None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A.view(3, 4, H, W)
    return (A[:, :3] * image[None]).sum(1) + A[:, 3]


def total_variation_loss_torch(grids):
    """gsplat's total_variation_loss: the sum over the three grid axes of the mean squared forward difference; an axis of size 1
    adds 0 (the mean of nothing is not taken)."""
    _check_shapes(grids, None, None, "total_variation_loss")
    tv = grids.reshape(-1)[:0].sum()                      # zero, and a function of grids whatever their shape
    for dim in (4, 3, 2):
        if grids.shape[dim] > 1:
            tv = tv + torch.diff(grids, dim=dim).square().mean()
    return tv


class _SliceApply(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids, image, idx):
        from . import _native
        ctx.save_for_backward(grids, image)
        ctx.idx = idx
        return _native.bilagrid_forward(grids, image, idx)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        grids, image = ctx.saved_tensors
        want_grids, want_image = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_grids or want_image):
            return None, None, None
        if grad_out.dtype != torch.float32 or not grad_out.is_contiguous():
            grad_out = grad_out.float().contiguous()
        dgrids, dimage = _native.bilagrid_backward(grids, image, ctx.idx, grad_out, want_grids, want_image)
        return dgrids, dimage, None


class _TotalVariation(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grids):
        from . import _native
        ctx.save_for_backward(grids)
        return _native.bilagrid_tv_forward(grids)

    @staticmethod
    def backward(ctx, grad_out):
        from . import _native
        (grids,) = ctx.saved_tensors
        return _native.bilagrid_tv_backward(grids, grad_out.float().reshape(1).contiguous())


def slice_apply(grids, image, idx, native=None):
    """image [3,H,W] through grid `idx` of grids [N,12,L,Gy,Gx] -> [3,H,W], differentiable in both (the gradient of grids is dense:
    zero rows for the other images)."""
    _check_shapes(grids, image, idx, "slice_apply")
    if _use_native(native, image, "slice_apply"):
        if grids.device != image.device:
            raise ValueError(f"slice_apply: grids are on {grids.device}, the image on {image.device}")
        return _SliceApply.apply(_f32c(grids, "grids"), _f32c(image, "image"), int(idx))
    return slice_apply_torch(_f32c(grids, "grids"), _f32c(image, "image"), idx)


def total_variation_loss(grids, native=None):
    """The total variation of all grids, a 0-dim tensor."""
    _check_shapes(grids, None, None, "total_variation_loss")
    if _use_native(native, grids, "total_variation_loss"):
        return _TotalVariation.apply(_f32c(grids, "grids"))
    return total_variation_loss_torch(_f32c(grids, "grids"))


class BilateralGrid(nn.Module):
    """`num` grids of shape [12, grid_w (luma), grid_y, grid_x], initialised to the identity transform (gsplat's BilateralGrid: the
    parameter has its name and layout, so a state_dict moves both ways)."""

    def __init__(self, num, grid_x=16, grid_y=16, grid_w=8):
        super().__init__()
        self.grid_width, self.grid_height, self.grid_guidance = int(grid_x), int(grid_y), int(grid_w)
        eye = torch.eye(4, dtype=torch.float32)[:3].reshape(1, 12, 1, 1, 1)
        self.grids = nn.Parameter(eye.repeat(int(num), 1, self.grid_guidance, self.grid_height, self.grid_width).contiguous())

    def forward(self, image, idx, native=None):
        return slice_apply(self.grids, image, idx, native)

    def tv_loss(self, native=None):
        return total_variation_loss(self.grids, native)


def bilateral_grid_lr(lr, it, iterations, warmup=1000, start_factor=0.01, final_factor=0.01):
    """The grid's learning rate at iteration `it` (counted from 0): gsplat's ChainedScheduler of LinearLR(start_factor, warmup) and
    ExponentialLR(final_factor ** (1 / iterations)) as one closed form."""
    warm = start_factor + (1.0 - start_factor) * min(max(it, 0), warmup) / warmup
    return lr * warm * final_factor ** (it / iterations)
