"""Mip-Splatting's 3D smoothing filter: every Gaussian is low-passed in world space by the highest sampling rate at which any training
camera saw it (csrc/gsr_filter3d.hip; the C ABI: include/gsrast.h, gsr_filter3d_*).  The world-space half of
Mip-Splatting's anti-aliasing; the screen-space half is `antialiasing` (antialias.py).

compute_filter_3d: for camera c with row-vector view matrix V, image W x H and focal lengths fx = W / (2 tan(FoVx / 2)), fy likewise,

    (x, y, z) = xyz_p @ V[:3,:3] + V[3,:3]
    valid(p,c) = z > 0.2  and  |x fx| <= 0.65 W z  and  |y fy| <= 0.65 H z        (-0.15 W <= x/z fx + W/2 <= 1.15 W, times z)
    d_p = min over the valid cameras of z;  a Gaussian no camera saw takes the maximum d over the others
    filter_p = d_p sqrt(0.2) / max_c fx_c                                            -> filter_3D [P,1]

apply_filter_3d: s' = sqrt(s^2 + f^2) per axis, o' = o sqrt(prod s^2 / prod s'^2) (upstream's get_scaling_with_3D_filter and
get_opacity_with_3D_filter).  raw=True: log-scales and logits in, log-scales and logits out, the mode GaussianRasterizer.forward_raw
takes.  A row with f == 0 passes through bit for bit.  Differentiable in opacities and scales; the filter is a buffer.

`native=None`: fp32 tensors on a GPU take the HIP kernels, everything else the torch twins below (the CPU path, and the baseline of
the GPU tests).  On a GPU a missing kernel is an error, never a quiet fall-back.
"""
import math

import numpy as np
import torch

NEAR_CUT = 0.2              # include/gsr_constants.h GSR_NEAR_CUT
VARIANCE = 0.2              # GSR_F3D_VARIANCE
MARGIN = 0.15               # GSR_F3D_MARGIN
AXIS_SWITCH = 40.0          # csrc/gsr_filter3d_math.h kF3dAxisSwitch: log f - u beyond which 1 + (f/s)^2 is (f/s)^2
EXP_SWITCH = -87.0          # kF3dExpSwitch: the log-scale under which exp(-u) is taken in two halves (alone it overflows at -88.7)


def camera_intrinsics(cam):
    """(fx, fy, W, H) of a camera as binary32 values (python floats)."""
    W, H = int(cam.image_width), int(cam.image_height)
    fx = np.float32(W / (2.0 * math.tan(cam.FoVx * 0.5)))
    fy = np.float32(H / (2.0 * math.tan(cam.FoVy * 0.5)))
    return float(fx), float(fy), float(W), float(H)


def camera_table(cameras, device):
    """-> (table [C,16] fp32 on `device`, max focal fx).  One stack of the view matrices where they live, one copy of the
    intrinsics: no per-camera device traffic."""
    if len(cameras) == 0:
        raise ValueError("compute_filter_3d: cameras is empty")
    V = torch.stack([torch.as_tensor(c.world_view_transform).detach() for c in cameras]).to(device=device, dtype=torch.float32)
    if tuple(V.shape[1:]) != (4, 4):
        raise ValueError(f"compute_filter_3d: cameras: world_view_transform must be [4,4], got {tuple(V.shape[1:])}")
    intr = torch.tensor([camera_intrinsics(c) for c in cameras], dtype=torch.float32).to(device)
    table = torch.cat((V[:, :, :3].transpose(1, 2).reshape(len(cameras), 12), intr), 1).contiguous()
    return table, max(camera_intrinsics(c)[0] for c in cameras)


def filter_scale(focal_max, dtype=torch.float32):
    """sqrt(0.2) / F as the kernels round it (binary32), or in binary64."""
    if dtype == torch.float32:
        return float(np.float32(np.sqrt(np.float32(VARIANCE))) / np.float32(focal_max))
    return math.sqrt(VARIANCE) / focal_max


def compute_filter_3d_torch(xyz, cameras):
    """The rule as a loop of torch ops over the cameras (any device, any float dtype): upstream's compute_3D_filter."""
    xyz = xyz.detach()
    P, dt = xyz.shape[0], xyz.dtype
    # 0.65 W as the kernel rounds it in binary32 (two roundings), or in the tensor's own precision
    half_extent = (lambda n: float(np.float32(0.5 + MARGIN) * np.float32(n))) if dt == torch.float32 else (lambda n: (0.5 + MARGIN) * n)
    d = torch.full((P,), float("inf"), dtype=dt, device=xyz.device)
    focal_max = 0.0
    for cam in cameras:
        fx, fy, W, H = camera_intrinsics(cam)
        focal_max = max(focal_max, fx)
        V = torch.as_tensor(cam.world_view_transform).detach().to(device=xyz.device, dtype=dt)
        x, y, z = (xyz[:, 0] * V[0, j] + xyz[:, 1] * V[1, j] + xyz[:, 2] * V[2, j] + V[3, j] for j in range(3))
        valid = (z > NEAR_CUT) & ((x * fx).abs() <= half_extent(W) * z) & ((y * fy).abs() <= half_extent(H) * z)
        d = torch.where(valid & (z < d), z, d)
    seen = d < float("inf")
    if P and not bool(seen.any()):
        raise ValueError("compute_filter_3d: no Gaussian is seen by any camera")
    if P:
        d = torch.where(seen, d, d[seen].max())
    return (d * filter_scale(focal_max, dt)).reshape(P, 1)


def apply_filter_3d_torch(opacities, scales, filter_3D, raw=False):
    """The application as torch ops (any device, any float dtype), differentiable through autograd, in the kernels' forms
    (csrc/gsr_filter3d_math.h)."""
    P = scales.shape[0]
    f = filter_3D.detach().reshape(P, 1).to(scales.dtype)
    o = opacities.reshape(P, 1)
    on = f > 0
    fs = torch.where(on, f, torch.ones_like(f))
    if raw:
        lf = torch.log(fs)
        t = lf - scales
        far = t > AXIS_SWITCH
        deep = scales < EXP_SWITCH                                              # exp(-u) in two halves
        half = torch.exp(-0.5 * torch.where(deep, scales, torch.zeros_like(scales)).clamp(min=-170.0))
        w = torch.where(deep, (fs * half) * half, fs * torch.exp(-scales.clamp(min=EXP_SWITCH)))
        w = torch.where(far, torch.zeros_like(w), w)
        g = torch.where(far, -t, -0.5 * torch.log1p(w * w))                     # log(s / s') per axis
        # the value is u - g; its derivative r = s^2 / s'^2 is written out, as the kernel's backward has it: autograd's own would
        # be 1 - (1 - r), which loses r's digits where the filter dominates
        r = torch.where(far, torch.exp(-2 * t.clamp(min=0)), 1 / (1 + w * w)).detach()
        s_out = torch.where(far, lf.expand_as(scales), scales - g).detach() + (scales - scales.detach()) * r
        lc = g.sum(1, keepdim=True)
        qc = -torch.expm1(lc)
        neg = o <= 0
        lo = o.clamp(max=0.0)
        hi = o.clamp(min=0.0)
        low = lo + lc - torch.log1p(torch.exp(lo) * qc)
        # e^-l; beyond l = 80 as e^(40 - l) e^-40, so that its gradient never passes through a subnormal (the kernel's dl)
        e = torch.where(hi > 80, torch.exp((40 - hi).clamp(max=0.0)) * math.exp(-40.0), torch.exp(-hi.clamp(max=80.0)))
        high = lc - torch.log(e + torch.where(qc == 0, torch.ones_like(qc), qc))
        o_out = torch.where(qc == 0, o, torch.where(neg, low, high))
    else:
        big = scales >= fs
        m, n = torch.where(big, scales, fs), torch.where(big, fs, scales)
        q = n / m
        root = torch.sqrt(1 + q * q)
        s_out = m * root
        rho = torch.where(big, torch.ones_like(q), q) / root
        o_out = o * (rho[:, 0:1] * rho[:, 1:2] * rho[:, 2:3])
    s_out = torch.where(on, s_out, scales)
    o_out = torch.where(on, o_out, o)
    return o_out.reshape(opacities.shape), s_out


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities, scales, filter_3D, raw):
        from . import _native
        inputs = tuple(t.contiguous() for t in (opacities, scales, filter_3D))
        o_out, s_out = _native.filter3d_apply_forward(*inputs, raw)
        if any(ctx.needs_input_grad[:2]):
            ctx.save_for_backward(*inputs)               # the backward recomputes from the inputs: the forward keeps no more
        ctx.raw = raw
        ctx.set_materialize_grads(False)
        return o_out, s_out

    @staticmethod
    def backward(ctx, g_o, g_s):
        from . import _native
        want = tuple(ctx.needs_input_grad[:2])
        if (g_o is None and g_s is None) or not any(want):
            return None, None, None, None
        opacities, scales, filter_3D = ctx.saved_tensors
        d_o, d_s = _native.filter3d_apply_backward(opacities, scales, filter_3D, ctx.raw, None if g_o is None else g_o.contiguous(),
                                                   None if g_s is None else g_s.contiguous(), want)
        return d_o, d_s, None, None


def _on_gpu(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def compute_filter_3d(xyz, cameras, native=None):
    """-> filter_3D [P,1].  xyz [P,3]; cameras: a sequence of objects with image_width, image_height, FoVx, FoVy and
    world_view_transform ([4,4], row-vector convention).  Raises ValueError when no Gaussian is seen by any camera.
    native: None = the HIP kernels for an fp32 tensor on a GPU, torch ops elsewhere; False = torch ops."""
    if xyz.dim() != 2 or xyz.shape[1] != 3:
        raise ValueError(f"compute_filter_3d: xyz [P,3] expected, got {tuple(xyz.shape)}")
    if len(cameras) == 0:
        raise ValueError("compute_filter_3d: cameras is empty")
    on_gpu = _on_gpu(xyz)
    if native is None:
        native = on_gpu
    if not native:
        return compute_filter_3d_torch(xyz, cameras)
    if not on_gpu:
        raise RuntimeError("compute_filter_3d(native=True) needs an fp32 tensor on a GPU: the HIP kernels have no CPU path")
    from . import _native
    if xyz.shape[0] == 0:
        return torch.empty(0, 1, dtype=torch.float32, device=xyz.device)
    table, focal_max = camera_table(cameras, xyz.device)
    out, seen = _native.filter3d_compute(xyz.detach().contiguous(), table, focal_max)
    if not seen:
        raise ValueError("compute_filter_3d: no Gaussian is seen by any camera")
    return out


def apply_filter_3d(opacities, scales, filter_3D, raw=False, native=None):
    """-> (opacities', scales'), shaped like the inputs.  opacities [P] or [P,1], scales [P,3], filter_3D [P] or [P,1] (a buffer: it
    receives no gradient).  raw: logits and log-scales in, logits and log-scales out.
    native: None = the HIP kernels for fp32 tensors on a GPU, torch ops elsewhere; False = torch ops."""
    if scales.dim() != 2 or scales.shape[1] != 3:
        raise ValueError(f"apply_filter_3d: scales [P,3] expected, got {tuple(scales.shape)}")
    P = scales.shape[0]
    if opacities.numel() != P or opacities.dim() not in (1, 2):
        raise ValueError(f"apply_filter_3d: opacities [P] or [P,1] expected for P = {P}, got {tuple(opacities.shape)}")
    if filter_3D.numel() != P or filter_3D.dim() not in (1, 2):
        raise ValueError(f"apply_filter_3d: filter_3D [P] or [P,1] expected for P = {P}, got {tuple(filter_3D.shape)}")
    for name, t in (("opacities", opacities), ("filter_3D", filter_3D)):       # loud, not a quiet trip through the twin
        if t.device != scales.device or t.dtype != scales.dtype:
            raise ValueError(f"apply_filter_3d: {name} is {t.dtype} on {t.device}, scales {scales.dtype} on {scales.device}: "
                             "one device and one dtype expected")
    on_gpu = _on_gpu(opacities, scales, filter_3D)
    if native is None:
        native = on_gpu
    if not native:
        return apply_filter_3d_torch(opacities, scales, filter_3D, raw=bool(raw))
    if not on_gpu:
        raise RuntimeError("apply_filter_3d(native=True) needs fp32 tensors on a GPU: the HIP kernels have no CPU path")
    return _ApplyFilter3D.apply(opacities, scales, filter_3D.detach(), bool(raw))
