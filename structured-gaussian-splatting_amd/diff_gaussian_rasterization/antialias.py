"""compensate_opacity: anti-aliased rendering (upstream's `antialiasing` switch, the 2D filter of Mip-Splatting) as one
differentiable per-Gaussian op in front of the unchanged rasterizer (csrc/gsr_antialias.hip; the C ABI and the rule:
include/gsrast.h, gsr_opacity_compensation_*).

The rasterizer low-passes every splat by adding h = 0.3 px^2 to the diagonal of its 2D covariance, and keeps that dilated covariance
for the radius, the binning rectangle and the conic.  With a0, b, c0 the 2D covariance BEFORE the dilation (same frustum clamp of
tx/tz, ty/tz and same scale_modifier as the preprocess kernel):

    det0 = a0 c0 - b^2      det1 = (a0 + h)(c0 + h) - b^2      x = det0 / det1
    rho = sqrt(max(AA_MIN_RATIO, x))                            opacity' = opacity rho

The entries are formed from the 2 x 3 factor W = T R diag(s) of that covariance (a0 = |W0|^2, c0 = |W1|^2, b = W0 . W1, det0 = the sum
of W's squared 2 x 2 minors): the same numbers without a0 c0 - b^2's cancellation on thin splats.

A Gaussian the preprocess culls before it has a covariance (view z <= 0.2), or one with det1 == 0, passes through unchanged.  The
gradient reaches opacity, means3D, scales and rotations; a clamped tx/tz (ty/tz) passes nothing through that coordinate and a
clamped x nothing at all, as in the rasterizer's own backward.  raw=True: the tensors are logits, log-scales and unnormalised
quaternions (GaussianRasterizer.forward_raw), the result is the logit of sigmoid(opacity) rho, the gradients are those on the raw
tensors.  No gradient is computed for the camera: a viewmatrix that requires grad is refused.

`native=False`, or tensors that are not fp32 on a GPU, take the same rule as torch ops (the CPU path of the host tests, and the
baseline of the GPU tests).  On a GPU a missing kernel is an error, never a quiet fall-back.
"""
import torch

NEAR_CUT = 0.2              # include/gsr_constants.h GSR_NEAR_CUT
FOV_CLAMP = 1.3             # GSR_FOV_CLAMP
COV2D_DILATE = 0.3          # GSR_COV2D_DILATE
AA_MIN_RATIO = 0.000025     # GSR_AA_MIN_RATIO: rho >= 0.005


def refuse_camera_grad(raster_settings) -> None:
    """rho depends on the view matrix and that gradient is not computed: refuse rather than return a camera gradient without it."""
    rs = raster_settings
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
        raise ValueError("antialiasing: the opacity compensation depends on the view matrix and returns no gradient for it; a viewmatrix, "
                         "projmatrix or campos that requires grad is not supported (detach them)")


def compensate_opacity_torch(opacities, means3D, scales, rotations, raster_settings, raw=False):
    """The rule as torch ops (any device, any float dtype), differentiable through autograd."""
    rs = raster_settings
    dt, shape = opacities.dtype, opacities.shape
    o = opacities.reshape(-1)
    V = rs.viewmatrix.detach().to(device=means3D.device, dtype=dt)
    if raw:
        s, q, op = torch.exp(scales), torch.nn.functional.normalize(rotations), torch.sigmoid(o)
    else:
        s, q, op = scales, rotations, o
    # the value is scale_modifier s; its gradient goes to s WITHOUT the factor scale_modifier, as the rasterizer's own backward
    # returns it (csrc/gsr_math.h geom_backward_one): the two add up on the same tensor
    s = (s * rs.scale_modifier).detach() + (s - s.detach())
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)
    pv = means3D @ V[:3, :3] + V[3, :3]
    culled = ~(pv[:, 2] > NEAR_CUT)
    tz = torch.where(culled, torch.ones_like(pv[:, 2]), pv[:, 2])
    fx, fy = rs.image_width / (2.0 * rs.tanfovx), rs.image_height / (2.0 * rs.tanfovy)
    limx, limy = FOV_CLAMP * rs.tanfovx, FOV_CLAMP * rs.tanfovy
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    # a clamped coordinate passes no gradient (the rasterizer's convention, csrc/gsr_math.h xmul / ymul)
    tx = torch.where((txtz < -limx) | (txtz > limx), (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where((tytz < -limy) | (tytz > limy), (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -(fx * tx) / (tz * tz), zero, fy / tz, -(fy * ty) / (tz * tz)], 1).view(-1, 2, 3)
    # the 2D covariance before the dilation is W W^T, W = J R_w2c R diag(s) [P,2,3]: its entries and, by Cauchy-Binet, its determinant
    # are sums without a subtraction of nearly equal terms (a0 c0 - b^2 loses (aspect ratio)^2 of its bits on a needle)
    W = (J @ V[:3, :3].transpose(0, 1)) @ R * s[:, None, :]
    w0, w1 = W[:, 0], W[:, 1]
    minors = torch.stack([w0[:, 0] * w1[:, 1] - w0[:, 1] * w1[:, 0], w0[:, 0] * w1[:, 2] - w0[:, 2] * w1[:, 0],
                          w0[:, 1] * w1[:, 2] - w0[:, 2] * w1[:, 1]], 1)
    h = COV2D_DILATE
    det0 = (minors * minors).sum(1)
    det1 = det0 + h * (W * W).sum((1, 2)) + h * h
    through = culled | (det1 == 0)
    ratio = det0 / torch.where(through, torch.ones_like(det1), det1)
    rho = torch.sqrt(torch.where(ratio > AA_MIN_RATIO, ratio, torch.full_like(ratio, AA_MIN_RATIO)))
    pp = op * torch.where(through, torch.ones_like(rho), rho)
    if raw:
        pp = torch.where(through, o, torch.log(pp) - torch.log1p(-pp))
    elif through.any():
        pp = torch.where(through, o, pp)
    return pp.reshape(shape)


class _CompensateOpacity(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opacities, means3D, scales, rotations, viewmatrix, desc, raw):
        from . import _native
        inputs = tuple(t.contiguous() for t in (opacities, means3D, scales, rotations, viewmatrix))
        out = _native.opacity_compensation_forward(desc, inputs[4], inputs[1], inputs[0], inputs[2], inputs[3], raw)
        if any(ctx.needs_input_grad[:4]):            # (under no_grad nothing is retained: nothing will ask)
            ctx.save_for_backward(*inputs)           # the backward recomputes from the inputs: the forward keeps no more
        ctx.desc, ctx.raw = desc, raw
        ctx.set_materialize_grads(False)
        return out

    @staticmethod
    def backward(ctx, grad):
        from . import _native
        want = tuple(ctx.needs_input_grad[:4])
        if grad is None or not any(want):
            return (None,) * 7
        opacities, means3D, scales, rotations, viewmatrix = ctx.saved_tensors
        grads = _native.opacity_compensation_backward(ctx.desc, viewmatrix, means3D, opacities, scales, rotations, ctx.raw,
                                                      grad.contiguous(), want)
        return grads + (None, None, None)


def compensate_opacity(opacities, means3D, scales, rotations, raster_settings, raw=False, native=None):
    """-> the compensated opacities, shaped like `opacities` ([P] or [P,1]).  means3D [P,3], scales [P,3], rotations [P,4];
    raster_settings: a GaussianRasterizationSettings (image size, tanfovx / tanfovy, scale_modifier and viewmatrix are read).
    raw: logits, log-scales and unnormalised quaternions in, a logit out.
    native: None = the HIP kernels for fp32 tensors on a GPU, torch ops elsewhere; False = torch ops."""
    rs = raster_settings
    P = means3D.shape[0]
    if opacities.numel() != P or tuple(means3D.shape) != (P, 3) or tuple(scales.shape) != (P, 3) or tuple(rotations.shape) != (P, 4):
        raise ValueError("compensate_opacity: opacities [P] or [P,1], means3D [P,3], scales [P,3], rotations [P,4] expected "
                         "(a precomputed 3D covariance is not supported)")
    refuse_camera_grad(rs)
    tensors = (opacities, means3D, scales, rotations)
    on_gpu = all(t.is_cuda and t.dtype == torch.float32 for t in tensors)
    if native is None:
        native = on_gpu
    if not native:
        return compensate_opacity_torch(*tensors, rs, raw=bool(raw))
    if not on_gpu:
        raise RuntimeError("compensate_opacity(native=True) needs fp32 tensors on a GPU: the HIP kernels have no CPU path")
    from . import _native
    desc = _native.make_desc(P, 0, 0, int(rs.image_width), int(rs.image_height), rs.tanfovx, rs.tanfovy, rs.scale_modifier, False, rs.debug)
    V = rs.viewmatrix.detach().to(device=means3D.device, dtype=torch.float32)
    return _CompensateOpacity.apply(*tensors, V, desc, bool(raw))
