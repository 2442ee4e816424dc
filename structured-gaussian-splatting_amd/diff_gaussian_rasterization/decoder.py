"""decode_structures: the decoder of the latent structured model (scene/latent_gaussian_model.py: Decoder) as one autograd node over
the HIP kernels of csrc/gsr_decoder.hip (the C ABI and the rules: include/gsrast.h, gsr_decoder_*).

For each of B structures, with x = (pos_emb[b], latents[b]) (the positional dims in FRONT, as the model concatenates them):

    h1 = relu(w0 x + b0)        h2 = relu((w1 h1 + b1) + h1)        decoded[b] = w2 h2 + b2

with nn.Linear's layouts (w [out, in]).  The forward is one launch that reads the inputs and writes `decoded` and nothing else; no
concatenated input and no hidden layer reaches memory.  The backward recomputes the hidden layers (the forward saves only its
inputs), passes a gradient where the pre-activation is > 0 as torch does, and sums the weight and bias gradients over B in a fixed
order without atomics: the same inputs give the same bits.  `pos_emb` gets no gradient (the model detaches the means).

The kernels cover fp32, hidden size 32, 1 <= latent size and input size <= 128.  `native=None` takes them for such tensors on a GPU
and the same rules as torch ops for everything else; `native=False` is the torch ops; `native=True` on anything the kernels do not
cover is a RuntimeError that says why, never a quiet fall-back.
"""
import torch

HIDDEN, MAX_IN = 32, 128


def decode_structures_torch(latents, w0, b0, w1, b1, w2, b2, pos_emb=None):
    """The decoder as torch ops (any device, any float dtype): op for op what scene.latent_gaussian_model.Decoder.forward runs."""
    linear = torch.nn.functional.linear
    x = latents if pos_emb is None else torch.cat((pos_emb, latents), dim=1)
    x = torch.relu(linear(x, w0, b0))
    x = torch.relu(linear(x, w1, b1) + x)
    return linear(x, w2, b2)


class _DecodeStructures(torch.autograd.Function):
    @staticmethod
    def forward(ctx, latents, w0, b0, w1, b1, w2, b2, pos_emb):
        from . import _native
        tensors = tuple(t.contiguous() for t in (latents, w0, b0, w1, b1, w2, b2))
        pos_emb = None if pos_emb is None else pos_emb.contiguous()
        decoded = _native.decoder_forward(pos_emb, tensors[0], tensors[1:])
        ctx.has_pos = pos_emb is not None
        if any(ctx.needs_input_grad[:7]):            # (under no_grad nothing is retained: nothing will ask)
            ctx.save_for_backward(*tensors, *(() if pos_emb is None else (pos_emb,)))      # the backward recomputes from the inputs
        return decoded

    @staticmethod
    def backward(ctx, d_decoded):
        from . import _native
        want = tuple(ctx.needs_input_grad[:7])
        if not any(want):
            return (None,) * 8
        saved = ctx.saved_tensors
        pos_emb = saved[7] if ctx.has_pos else None
        return _native.decoder_backward(pos_emb, saved[0], saved[1:7], d_decoded.contiguous(), want) + (None,)


def _unsupported(latents, w0, b0, w1, b1, w2, b2, pos_emb):
    """Why the HIP kernels do not take these tensors, or None when they do."""
    if w0.shape[0] != HIDDEN:
        return f"hidden_size = {w0.shape[0]} is not supported (the kernels are built for {HIDDEN})"
    if w0.shape[1] > MAX_IN:
        return f"in_size = {w0.shape[1]} is not supported (at most {MAX_IN})"
    tensors = (latents, w0, b0, w1, b1, w2, b2) + (() if pos_emb is None else (pos_emb,))
    if not all(t.is_cuda for t in tensors):
        return "needs tensors on a GPU: the HIP decoder has no CPU path"
    if not all(t.dtype == torch.float32 for t in tensors):
        return "needs fp32 tensors"
    if len({t.device for t in tensors}) != 1:
        return "needs all tensors on one device"
    return None


def decode_structures(latents, w0, b0, w1, b1, w2, b2, pos_emb=None, native=None):
    """-> decoded [B, OUT].  latents [B, L], pos_emb [B, IN - L] or None, w0 [H, IN], b0 [H], w1 [H, H], b1 [H], w2 [OUT, H],
    b2 [OUT].  native: None = the HIP kernels where they apply (fp32 on a GPU, H = 32, IN <= 128), torch ops elsewhere; False = torch
    ops; True = the HIP kernels or a RuntimeError."""
    if latents.dim() != 2 or w0.dim() != 2 or w1.dim() != 2 or w2.dim() != 2 or (pos_emb is not None and pos_emb.dim() != 2):
        raise ValueError("decode_structures: latents [B, L], pos_emb [B, IN - L], w0 [H, IN], w1 [H, H], w2 [OUT, H] expected")
    B, L = latents.shape
    H, IN = w0.shape
    P0 = 0 if pos_emb is None else pos_emb.shape[1]
    if L < 1 or IN != P0 + L or (pos_emb is not None and pos_emb.shape[0] != B) or w2.shape[0] < 1 or tuple(w1.shape) != (H, H) or \
            w2.shape[1] != H or tuple(b0.shape) != (H,) or tuple(b1.shape) != (H,) or tuple(b2.shape) != (w2.shape[0],):
        raise ValueError(f"decode_structures: shapes do not fit: latents {tuple(latents.shape)}, pos_emb "
                         f"{None if pos_emb is None else tuple(pos_emb.shape)}, w0 {tuple(w0.shape)}, b0 {tuple(b0.shape)}, w1 "
                         f"{tuple(w1.shape)}, b1 {tuple(b1.shape)}, w2 {tuple(w2.shape)}, b2 {tuple(b2.shape)}")
    why = _unsupported(latents, w0, b0, w1, b1, w2, b2, pos_emb)
    if native is None:
        native = why is None
    if not native:
        return decode_structures_torch(latents, w0, b0, w1, b1, w2, b2, pos_emb)
    if why is not None:
        raise RuntimeError(f"decode_structures(native=True): {why}")
    return _DecodeStructures.apply(latents, w0, b0, w1, b1, w2, b2, pos_emb)
