"""Binary64 restatement of the latent structured model's decoder with an EXPLICIT backward (numpy, no autograd), the magnitude
network that bounds what an fp32 evaluation in any summation order may differ by, and the two kinds of test data.  What the fp32
paths are held to (tests/test_decoder_ref.py on the host, tests/test_gpu_decoder.py on the GPU).

    x = (pos_emb, latents)    z0 = x W0^T + b0    h1 = max(z0, 0)    z1 = h1 W1^T + b1 + h1    h2 = max(z1, 0)    out = h2 W2^T + b2

Bounds, with u = 2^-24: an fma chain of n terms errs by at most n u sum|a b| (to first order), and ReLU is 1-Lipschitz, so with
    A0 = |x| |W0|^T + |b0|      A1 = A0 |W1|^T + |b1| + A0      A2 = A1 |W2|^T + |b2|
the three layers err by at most (IN + 2) u A0, (IN + 38) u A1 and (IN + 72) u A2 elementwise.  A structure is FRAGILE if a binary64
pre-activation lies within twice its layer's bound of zero: an fp32 evaluation may then take the other side of the ReLU, and its
row of G is zeroed for both sides.  The backward's magnitudes are the same chain with absolute values and the binary64 masks.
"""
import numpy as np

U = 2.0 ** -24
NAMES = ("latents", "w0", "b0", "w1", "b1", "w2", "b2")


def forward(x, w0, b0, w1, b1, w2, b2):
    """All binary64 arrays; x [B, IN] is the concatenated input.  -> dict(z0, h1, z1, h2, out)."""
    z0 = x @ w0.T + b0
    h1 = np.maximum(z0, 0.0)
    z1 = h1 @ w1.T + b1 + h1
    h2 = np.maximum(z1, 0.0)
    return dict(z0=z0, h1=h1, z1=z1, h2=h2, out=h2 @ w2.T + b2)


def backward(x, params, G, L, fwd=None):
    """The chain rule written out.  -> the seven gradients in NAMES' order (d latents = the last L columns of d x)."""
    w0, b0, w1, b1, w2, b2 = params
    f = fwd or forward(x, *params)
    dz1 = (G @ w2) * (f["z1"] > 0)
    dz0 = (dz1 @ w1 + dz1) * (f["z0"] > 0)
    dx = dz0 @ w0
    return (dx[:, x.shape[1] - L:], dz0.T @ x, dz0.sum(0), dz1.T @ f["h1"], dz1.sum(0), G.T @ f["h2"], G.sum(0))


def magnitudes(x, params):
    w0, b0, w1, b1, w2, b2 = (np.abs(p) for p in params)
    A0 = np.abs(x) @ w0.T + b0
    A1 = A0 @ w1.T + b1 + A0
    return A0, A1, A1 @ w2.T + b2


def backward_magnitudes(x, params, G, L, fwd=None):
    """`mag` of each gradient in NAMES' order: the backward chain with absolute values and the binary64 masks of `fwd` (None: no
    masks).  The forward's error enters the weight gradients through h1, h2, which A0, A1 dominate."""
    w0, b0, w1, b1, w2, b2 = (np.abs(p) for p in params)
    A0, A1, _ = magnitudes(x, params)
    g = np.abs(G)
    m1 = (g @ w2) * (1.0 if fwd is None else fwd["z1"] > 0)
    m0 = (m1 @ w1 + m1) * (1.0 if fwd is None else fwd["z0"] > 0)
    return ((m0 @ w0)[:, x.shape[1] - L:], m0.T @ np.abs(x), m0.sum(0), m1.T @ A0, m1.sum(0), g.T @ A1, g.sum(0))


def fragile(x, params, fwd):
    """[B] bool: a pre-activation within twice its own forward bound of zero."""
    IN = x.shape[1]
    A0, A1, _ = magnitudes(x, params)
    return ((np.abs(fwd["z0"]) <= 2 * (IN + 2) * U * A0) | (np.abs(fwd["z1"]) <= 2 * (IN + 38) * U * A1)).any(1)


def forward_bound(x, params):
    return (x.shape[1] + 72) * U * magnitudes(x, params)[2]


def gradient_bounds(x, params, G, L, fwd):
    """Elementwise bounds in NAMES' order: (OUT + IN + 80) u mag for d latents, (OUT + IN + 80 + B) u mag for the sums over B."""
    B, IN, OUT = x.shape[0], x.shape[1], G.shape[1]
    mags = backward_magnitudes(x, params, G, L, fwd)
    return tuple((OUT + IN + 80 + (B if i else 0)) * U * m for i, m in enumerate(mags))


# ---- test data ---------------------------------------------------------------------------------------------------------------------
def integer_case(B, L, P0, OUT, seed):
    """Small-integer data, binary64 arrays: (pos_emb or None, latents, params, G).  W0 and W1 are banded with 4 entries of +-1 per
    row, W2 has 3 per row, inputs and G are in {-1, 0, 1}; the signs are drawn, so no pattern is symmetric.  Every sum of such
    terms is an integer far below 2^24 (the tests assert largest_magnitude < 2^24), so binary32 is exact in ANY order, and pre-activations of
    exactly 0 are common."""
    rng = np.random.default_rng(seed)
    IN, H = P0 + L, 32
    sign = lambda: float(rng.choice((-1.0, 1.0)))
    w0, w1, w2 = np.zeros((H, IN)), np.zeros((H, H)), np.zeros((OUT, H))
    for i in range(H):
        for t in range(4):
            w0[i, (4 * i + t) % IN] += sign()
            w1[i, (i + 5 * t + 1) % H] = sign()
    for o in range(OUT):
        for col in ((7 * o + 3) % H, (3 * o + 11) % H, (o // 3 + 20) % H):
            w2[o, col] = sign()
    ints = lambda *s: rng.integers(-1, 2, size=s).astype(np.float64)
    params = (w0, ints(H), w1, ints(H), w2, ints(OUT))
    return (ints(B, P0) if P0 else None), ints(B, L), params, ints(B, OUT)


def largest_magnitude(x, params, G, L):
    """What no product and no partial sum of the forward or the backward, taken in any order, can exceed: the unmasked chains of
    absolute values (a mask only removes terms)."""
    return max(float(m.max()) for m in magnitudes(x, params) + backward_magnitudes(x, params, G, L))


def float_case(B, L, P0, OUT, seed):
    """nn.Linear's default initialisation, randn latents, the model's positional embedding of randn means: fp32 torch tensors
    (pos_emb or None, latents, params, G) on the host."""
    import torch
    from scene.latent_gaussian_model import Decoder, positional_embedding
    torch.manual_seed(seed)
    assert P0 in (0, 63)
    dec = Decoder(L, 32, OUT, P0)
    latents = torch.randn(B, L)
    pos = positional_embedding(torch.randn(B, 3)) if P0 else None
    G = torch.randn(B, OUT)
    params = tuple(p.detach().clone() for p in (dec.lin0.weight, dec.lin0.bias, dec.lin1.weight, dec.lin1.bias, dec.lin2.weight,
                                                dec.lin2.bias))
    return pos, latents, params, G


def to64(pos, latents, params, G=None):
    """fp32 torch tensors -> (x, params, G) as binary64 arrays (exact)."""
    n = lambda t: t.detach().cpu().numpy().astype(np.float64)
    x = n(latents) if pos is None else np.concatenate((n(pos), n(latents)), 1)
    return x, tuple(n(p) for p in params), (None if G is None else n(G))
