"""compose_structures: the composition of the latent structured model (scene/latent_gaussian_model.py) as one autograd node over
two HIP launches (csrc/gsr_structured.hip; the C ABI and the rules: include/gsrast.h, gsr_structured_compose_*).

B structures carry a mean, an opacity logit, a log-scale and a raw rotation; a decoder gives each K children of D = 11 + 3 M
floats.  Child p = b K + k, with c = decoded[b, k D : (k + 1) D]:

    xyz = c[0:3] + mean[b]    opacity = c[3] + opacity[b]    scaling = c[4:7] + scale[b]
    rotation = std(normalize(rotation[b]) (x) normalize(c[7:11]))       features = c[11:] as [M, 3]

((x): Hamilton product, real part first; std flips the sign where the real part is negative.)  The five results are exactly what
GaussianRasterizer.forward_raw takes with one interleaved SH table.  The structure gradients are sums over a structure's children
in ascending k, without atomics: the same inputs give the same bits.

`native=False`, or tensors that are not on a GPU, take the same rules as torch ops (the CPU path of the model's host tests, and
the baseline of tools/structured_bench.py).  On a GPU a missing kernel is an error, never a quiet fall-back.
"""
import torch


def _hamilton(a, b):
    aw, ax, ay, az = a.unbind(-1)
    bw, bx, by, bz = b.unbind(-1)
    return torch.stack((aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                        aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw), -1)


def compose_structures_torch(decoded, means, opacities, scales, rotations, K, sh_coeffs):
    """The composition as torch ops (any device, any float dtype)."""
    B, D = decoded.shape[0], 11 + 3 * sh_coeffs
    c = decoded.reshape(B, K, D)
    normalize = torch.nn.functional.normalize
    q = _hamilton(normalize(rotations, dim=-1).unsqueeze(1), normalize(c[:, :, 7:11], dim=-1))
    q = torch.where(q[..., 0:1] < 0, -q, q)
    return ((c[:, :, 0:3] + means.unsqueeze(1)).flatten(0, 1), (c[:, :, 3:4] + opacities.unsqueeze(1)).flatten(0, 1),
            (c[:, :, 4:7] + scales.unsqueeze(1)).flatten(0, 1), q.flatten(0, 1), c[:, :, 11:].reshape(B * K, sh_coeffs, 3))


class _ComposeStructures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, decoded, means, opacities, scales, rotations, K, sh_coeffs):
        from . import _native
        inputs = tuple(t.contiguous() for t in (decoded, means, opacities, scales, rotations))
        outs = _native.structured_compose_forward(*inputs, K, sh_coeffs)
        if any(ctx.needs_input_grad[:5]):            # (under no_grad nothing is retained: nothing will ask)
            ctx.save_for_backward(*inputs)           # the backward recomputes from the inputs: the forward keeps no more
        ctx.K, ctx.sh_coeffs = K, sh_coeffs
        ctx.set_materialize_grads(False)             # an unused output arrives as None and goes to the kernel as NULL
        return outs

    @staticmethod
    def backward(ctx, *grads):
        from . import _native
        want = tuple(ctx.needs_input_grad[:5])
        if all(g is None for g in grads) or not any(want):
            return (None,) * 7
        grads = tuple(None if g is None else g.contiguous() for g in grads)
        return _native.structured_compose_backward(*ctx.saved_tensors, ctx.K, ctx.sh_coeffs, grads, want) + (None, None)


def compose_structures(decoded, means, opacities, scales, rotations, K, sh_coeffs, native=None):
    """-> (xyz [P,3], opacity [P,1], scaling [P,3], rotation [P,4], features [P,sh_coeffs,3]), P = B K.
    decoded [B, K (11 + 3 sh_coeffs)], means [B,3], opacities [B,1], scales [B,3], rotations [B,4]; K >= 1 (any value),
    sh_coeffs in {1, 4, 9, 16}.  native: None = the HIP kernels for fp32 tensors on a GPU, torch ops elsewhere; False = torch ops."""
    K, sh_coeffs = int(K), int(sh_coeffs)
    B = means.shape[0]
    if K < 1 or sh_coeffs not in (1, 4, 9, 16):
        raise ValueError(f"K = {K} must be >= 1 and sh_coeffs = {sh_coeffs} one of 1, 4, 9, 16")
    if tuple(decoded.shape) != (B, K * (11 + 3 * sh_coeffs)) or tuple(opacities.shape) != (B, 1) or \
            tuple(means.shape) != (B, 3) or tuple(scales.shape) != (B, 3) or tuple(rotations.shape) != (B, 4):
        raise ValueError("compose_structures: decoded [B, K (11 + 3 sh_coeffs)], means [B,3], opacities [B,1], scales [B,3], "
                         "rotations [B,4] expected")
    tensors = (decoded, means, opacities, scales, rotations)
    on_gpu = all(t.is_cuda and t.dtype == torch.float32 for t in tensors)
    if native is None:
        native = on_gpu
    if not native:
        return compose_structures_torch(*tensors, K, sh_coeffs)
    if not on_gpu:
        raise RuntimeError("compose_structures(native=True) needs fp32 tensors on a GPU: the HIP composition has no CPU path")
    return _ComposeStructures.apply(*tensors, K, sh_coeffs)
