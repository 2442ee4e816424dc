"""Binary64 restatement of the latent structured model (decoder + composition), with autograd: the reference the fp32 paths are
held to (tests/test_structured_ref.py on the host, tests/test_gpu_structured.py on the GPU).  Written from the rules alone and
formulated unlike the product code (diff_gaussian_rasterization/structured.py, csrc/gsr_math.h compose_child): the quaternion
product is the contraction of the algebra's structure constants built from the multiplication table of 1, i, j, k, the
normalisation is spelled out, the sign rule is a multiplication by +-1, every child looks its structure up through an index.

    child p = b K + k, c = decoded[b, k D : (k + 1) D], D = 11 + 3 M
    xyz = c[0:3] + mean[b]   opacity = c[3] + opacity[b]   scaling = c[4:7] + scale[b]
    rotation = std(n(rot[b]) (x) n(c[7:11]))   n(v) = v / max(|v|, 1e-12)   std(q) = -q iff q_w < 0   features = c[11:] as [M,3]
"""
import torch

F64 = torch.float64


def _structure_constants():
    """E[i, j, k]: coefficient of basis element i in e_j e_k, for (1, i, j, k)."""
    E = torch.zeros(4, 4, 4, dtype=F64)
    for j in range(4):
        E[j, 0, j] = 1.0                       # 1 e = e
        E[j, j, 0] = 1.0                       # e 1 = e
    for j in (1, 2, 3):
        E[0, j, j] = -1.0                      # i i = j j = k k = -1
    for a, b, c in ((1, 2, 3), (2, 3, 1), (3, 1, 2)):
        E[c, a, b] = 1.0                       # i j = k, j k = i, k i = j
        E[c, b, a] = -1.0                      # and the other way round with a minus
    return E


_E = _structure_constants()


def unit(v):
    n = (v * v).sum(-1, keepdim=True).sqrt()
    return v / torch.clamp(n, min=1e-12)


def compose(decoded, means, opacities, scales, rotations, K, M):
    """All binary64.  -> (xyz [P,3], opacity [P,1], scaling [P,3], rotation [P,4], features [P,M,3])."""
    B, D = means.shape[0], 11 + 3 * M
    rows = decoded.reshape(B * K, D)
    owner = torch.arange(B * K) // K
    xyz = rows[:, 0:3] + means[owner]
    opacity = rows[:, 3:4] + opacities[owner]
    scaling = rows[:, 4:7] + scales[owner]
    q = torch.einsum("ijk,pj,pk->pi", _E.to(rows.device), unit(rotations)[owner], unit(rows[:, 7:11]))
    sign = 1.0 - 2.0 * (q[:, 0:1] < 0).to(F64)
    return xyz, opacity, scaling, q * sign, rows[:, 11:].reshape(B * K, M, 3)


def decode(state, use_positional_embedding=False, multires=10):
    """The decoder on a state_dict (any float dtype), in binary64: [B, K D]."""
    p = {k: v.to(F64) for k, v in state.items() if v.is_floating_point()}
    x = p["structure_latents"]
    if use_positional_embedding:
        m = p["structure_means"].detach()
        # the frequencies are binary32 powers of two: exact in either precision
        emb = [m] + [f(m * 2.0 ** i) for i in range(multires) for f in (torch.sin, torch.cos)]
        x = torch.cat(emb + [x], dim=1)
    h0 = torch.clamp(x @ p["decoder.lin0.weight"].T + p["decoder.lin0.bias"], min=0)
    h1 = torch.clamp(h0 @ p["decoder.lin1.weight"].T + p["decoder.lin1.bias"] + h0, min=0)
    return h1 @ p["decoder.lin2.weight"].T + p["decoder.lin2.bias"]


def model_forward(state, K, M, use_positional_embedding=False):
    """-> (decoded [B, K D], the five composed tensors) from a state_dict whose float tensors may require grad."""
    decoded = decode(state, use_positional_embedding)
    p = {k: state[k].to(F64) for k in ("structure_means", "structure_opacities", "structure_scales", "structure_rotations")}
    return decoded, compose(decoded, p["structure_means"], p["structure_opacities"], p["structure_scales"], p["structure_rotations"], K, M)


def compose_backward(decoded, means, opacities, scales, rotations, K, M, grads):
    """dL/d(decoded, means, opacities, scales, rotations) for incoming `grads` (five tensors or None) — autograd of compose()."""
    leaves = [t.detach().to(F64).clone().requires_grad_(True) for t in (decoded, means, opacities, scales, rotations)]
    outs = compose(*leaves, K, M)
    total = sum((o * g.to(F64)).sum() for o, g in zip(outs, grads) if g is not None)
    return torch.autograd.grad(total, leaves, allow_unused=True)


# ---- what the fp32 paths are held to (tests/test_structured_ref.py, tests/test_gpu_structured.py): a rotation component is <= 1 and about
# 30 roundings of 2^-24 reach it: 2e-6 absolute; the quaternion gradients carry the factor |g| / |q| of the normalisation's
# derivative: 4e-6 |g_rot|_2 / |c_q|_2 per element of d c_q, 4e-6 sum_k |g_rot_k|_1 / |s_rot|_2 of d s_rot; a sum of K terms taken
# in any fixed order: K 2^-23 sum_k |g_k|.
ROT_ABS = 2e-6
ROT_GRAD_REL = 4e-6


def make_case(B, K, M, seed, device="cpu"):
    """fp32 inputs: decoder output, the four structure tensors, five incoming gradients; quaternion norms drawn in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    D, P = 11 + 3 * M, B * K
    r = lambda *s: torch.randn(*s, generator=g)
    with_norm = lambda q: q / q.norm(dim=-1, keepdim=True) * (0.5 + 1.5 * torch.rand(*q.shape[:-1], 1, generator=g))
    decoded = r(B, K, D)
    decoded[:, :, 7:11] = with_norm(decoded[:, :, 7:11])
    inputs = [decoded.reshape(B, K * D).contiguous(), r(B, 3), r(B, 1), r(B, 3), with_norm(r(B, 4))]
    grads = [r(P, 3), r(P, 1), r(P, 3), r(P, 4), r(P, M, 3)]
    return [t.to(device) for t in inputs], [t.to(device) for t in grads]


def check_against_ref(B, K, M, inputs, grads, outs, d_in, what=""):
    """outs: the five composed tensors; d_in: gradients w.r.t. (decoded, means, opacities, scales, rotations) (or None to skip the
    backward).  Everything is compared on the host against structured_ref in binary64, under the bounds above;
    returns the share of rows judged with the other sign (|q_w| < 1e-6 in binary64: the fp32 sign may legitimately differ)."""
    D, P = 11 + 3 * M, B * K
    cpu = lambda ts: [None if t is None else t.detach().cpu() for t in ts]
    inputs, grads, outs = cpu(inputs), cpu(grads), cpu(outs)
    want = compose(*[t.to(F64) for t in inputs], K, M)
    for name, got, ref in zip(("xyz", "opacity", "scaling"), outs[:3], want[:3]):
        assert torch.equal(got, ref.to(torch.float32)), f"{what} {name}: a single fp32 add must be bit-equal"
    assert torch.equal(outs[4], inputs[0].reshape(P, D)[:, 11:].reshape(P, M, 3)), f"{what} features: a copy"
    q64, got_q = want[3], outs[3].to(F64)
    flipped = (q64[:, 0].abs() < 1e-6) & ((got_q + q64).abs().sum(1) < (got_q - q64).abs().sum(1))
    sgn = torch.where(flipped, -1.0, 1.0).to(F64)[:, None]
    err = (got_q * sgn - q64).abs().max().item()
    share = float(flipped.sum()) / P
    print(f"{what} rotation: max abs error {err:.3e} (bound {ROT_ABS:.0e}); rows judged with the other sign: {int(flipped.sum())} of {P}")
    assert err <= ROT_ABS, f"{what} rotation error {err:.3e}"
    assert share <= 1e-4, f"{what}: {share:.2e} of the rows needed the other sign"
    if d_in is None:
        return share
    d_in = cpu(d_in)
    g_for_ref = list(grads)
    if g_for_ref[3] is not None:
        g_for_ref[3] = g_for_ref[3].to(F64) * sgn            # the other sign of q: the rotation gradients negated accordingly
    ref = compose_backward(*inputs, K, M, g_for_ref)
    zeros = lambda i: torch.zeros_like(outs[i])
    g = [zeros(i) if x is None else x for i, x in enumerate(grads)]
    if d_in[0] is not None:
        dd = d_in[0].reshape(P, D)
        assert torch.equal(dd[:, 0:3], g[0]) and torch.equal(dd[:, 3:4], g[1]) and torch.equal(dd[:, 4:7], g[2]), f"{what} d decoded adds"
        assert torch.equal(dd[:, 11:], g[4].reshape(P, 3 * M)), f"{what} d decoded SH columns"
        cq = inputs[0].reshape(P, D)[:, 7:11].to(F64)
        bound = ROT_GRAD_REL * g[3].to(F64).norm(dim=1) / cq.norm(dim=1)
        e = (dd[:, 7:11].to(F64) - ref[0].reshape(P, D)[:, 7:11]).abs().max(1).values
        ok = bound > 0
        print(f"{what} d c_q: worst error / bound {(e[ok] / bound[ok]).max().item() if ok.any() else 0.0:.3f}")
        assert (e <= bound).all(), f"{what} d decoded[7:11]: worst ratio {(e[ok] / bound[ok]).max().item():.2f}"
    if d_in[4] is not None:
        bound = ROT_GRAD_REL * g[3].to(F64).abs().sum(1).reshape(B, K).sum(1) / inputs[4].to(F64).norm(dim=1)
        e = (d_in[4].to(F64) - ref[4]).abs().max(1).values
        ok = bound > 0
        print(f"{what} d s_rot: worst error / bound {(e[ok] / bound[ok]).max().item() if ok.any() else 0.0:.3f}")
        assert (e <= bound).all(), f"{what} d s_rot: worst ratio {(e[ok] / bound[ok]).max().item():.2f}"
    for i, gi, name in ((1, 0, "means"), (2, 1, "opacities"), (3, 2, "scales")):
        if d_in[i] is None:
            continue
        bound = K * 2.0 ** -23 * g[gi].to(F64).abs().reshape(B, K, -1).sum(1)
        e = (d_in[i].to(F64) - ref[i]).abs()
        assert (e <= bound).all(), f"{what} d {name}: {e.max().item():.3e}"
    return share
