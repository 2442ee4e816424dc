"""The fused HIP decoder on the GPU (csrc/gsr_decoder.hip through diff_gaussian_rasterization.decoder.decode_structures) against the
binary64 restatement with its explicit backward (tests/decoder_ref.py, which also holds the bounds and their derivation):
small-integer data that binary32 sums exactly in any order, so every output must come out bit for bit (a dropped tile, a wrong k
permutation, a swapped row and column or a bad tail cannot hide, and exact zeros among the pre-activations pin the > 0 mask rule);
random data under the derived bounds; the same bits from the same inputs; wanted and unwanted gradients; and
scene.LatentGaussianModel with native_decode=True through render() and the fused loss."""
import numpy as np
import pytest
import torch

import decoder_ref as DR
import scene_synth as S
from diff_gaussian_rasterization import _native as N
from diff_gaussian_rasterization.decoder import decode_structures
from scene.latent_gaussian_model import LatentGaussianModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, L, pos, K, M): under one column tile; a row tail and half a column tile; odd L (the k padding) and OUT no multiple of 32;
# IN = 95 with 15 column tiles; many blocks, each with several tile groups, and the reduce kernel, without and with the embedding
SHAPES = [(1, 32, False, 1, 1), (33, 32, False, 8, 1), (257, 7, False, 3, 4), (257, 32, True, 8, 16),
          (70_000, 32, False, 8, 1), (70_000, 32, True, 2, 1)]
SMALL = SHAPES[:4]
# (B, L, positional dims, OUT) beyond those, for the exact test alone: IN = 103, so dW0 has a fourth row tile (a wave's second small
# accumulator), and OUT = 590 = 19 column tiles, more than one backward launch holds accumulators for (dW2 takes a second launch)
EXTRA_DIMS = [(70, 40, 63, 590)]
_RUNS = {}


def _dims(shape):
    B, L, pos, K, M = shape
    return B, L, (63 if pos else 0), K * (11 + 3 * M)


def _hip(pos, latents, params, G):
    """One forward and one backward with every gradient wanted -> (decoded, the seven gradients in DR.NAMES' order), on the device."""
    leaves = [latents.clone().requires_grad_(True)] + [p.clone().requires_grad_(True) for p in params]
    out = decode_structures(*leaves, pos_emb=pos, native=True)
    return out.detach(), torch.autograd.grad(out, leaves, G)


def _float_run(shape, seed):
    """The float data of one shape and seed, its binary64 reference with the fragile structures' rows of G zeroed, and the HIP
    results: computed once, shared by the tests below and left unchanged by them."""
    key = (shape, seed)
    if key not in _RUNS:
        B, L, P0, OUT = _dims(shape)
        pos, latents, params, G = DR.float_case(B, L, P0, OUT, seed)
        x, p64, g64 = DR.to64(pos, latents, params, G)
        fwd = DR.forward(x, *p64)
        frag = DR.fragile(x, p64, fwd)
        g64[frag] = 0.0
        dev = lambda t: None if t is None else t.to(DEV)
        inputs = (dev(pos), dev(latents), tuple(dev(p) for p in params), torch.from_numpy(g64).float().to(DEV))
        out, grads = _hip(*inputs)
        _RUNS[key] = dict(x=x, p64=p64, g64=g64, fwd=fwd, frag=frag, inputs=inputs, out=out, grads=grads)
    return _RUNS[key]


@pytest.mark.parametrize("dims", [_dims(s) for s in SHAPES] + EXTRA_DIMS)
def test_integer_data_bit_for_bit(dims):
    B, L, P0, OUT = dims
    pos, lat, params, G = DR.integer_case(B, L, P0, OUT, 7 + B + OUT)
    x = lat if pos is None else np.concatenate((pos, lat), 1)
    worst = DR.largest_magnitude(x, params, G, L)
    assert worst < 2 ** 24, worst                          # every product and partial sum, in any order, is exact in binary32
    fwd = DR.forward(x, *params)
    if B > 1:
        assert (fwd["z0"] == 0).any() and (fwd["z1"] == 0).any() and (fwd["z0"] > 0).any() and (fwd["z1"] > 0).any()
    t = lambda a: None if a is None else torch.from_numpy(a).float().to(DEV)
    out, grads = _hip(t(pos), t(lat), tuple(t(p) for p in params), t(G))
    torch.cuda.synchronize()
    assert tuple(out.shape) == (B, OUT)
    want = fwd["out"]
    got = out.cpu().numpy().astype(np.float64)
    assert np.array_equal(got, want), f"decoded: {int((got != want).sum())} of {want.size} differ, first at {np.argwhere(got != want)[:4].tolist()}"
    for name, g, w in zip(DR.NAMES, grads, DR.backward(x, params, G, L, fwd)):
        g = g.cpu().numpy().astype(np.float64)
        assert g.shape == w.shape, name
        assert np.array_equal(g, w), f"d {name}: {int((g != w).sum())} of {w.size} differ, first at {np.argwhere(g != w)[:4].tolist()}"


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("shape", SMALL)
def test_float_data_within_the_derived_bounds(shape, seed):
    B, L, P0, OUT = _dims(shape)
    r = _float_run(shape, seed)
    nfrag = int(r["frag"].sum())
    assert nfrag <= max(2, 0.05 * B), f"{nfrag} fragile structures of {B}"
    err = np.abs(r["out"].cpu().numpy().astype(np.float64) - r["fwd"]["out"])
    bound = DR.forward_bound(r["x"], r["p64"])
    ratios = {"decoded": float((err / bound).max())}
    ok = bool((err <= bound).all())
    want = DR.backward(r["x"], r["p64"], r["g64"], L, r["fwd"])
    bounds = DR.gradient_bounds(r["x"], r["p64"], r["g64"], L, r["fwd"])
    for name, g, w, b in zip(DR.NAMES, r["grads"], want, bounds):
        e = np.abs(g.cpu().numpy().astype(np.float64) - w)
        ok &= bool((e <= b).all())
        live = b > 0
        ratios["d " + name] = float((e[live] / b[live]).max()) if live.any() else 0.0
    print(f"decoder {shape} seed {seed}: {nfrag} fragile; worst error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert ok, ratios


def test_same_inputs_same_bits():
    r = _float_run(SHAPES[4], 0)                           # the largest shape: 183 blocks of three tile groups and the reduction
    out, grads = _hip(*r["inputs"])
    assert torch.equal(out, r["out"])
    for name, a, b in zip(DR.NAMES, grads, r["grads"]):
        assert torch.equal(a, b), name
    # and inside the bounds there too, where a block adds many tiles
    B, L, P0, OUT = _dims(SHAPES[4])
    assert int(r["frag"].sum()) <= 0.05 * B
    assert (np.abs(out.cpu().numpy().astype(np.float64) - r["fwd"]["out"]) <= DR.forward_bound(r["x"], r["p64"])).all()
    want = DR.backward(r["x"], r["p64"], r["g64"], L, r["fwd"])
    for name, g, w, b in zip(DR.NAMES, grads, want, DR.gradient_bounds(r["x"], r["p64"], r["g64"], L, r["fwd"])):
        assert (np.abs(g.cpu().numpy().astype(np.float64) - w) <= b).all(), name


def test_wanted_and_unwanted_gradients():
    r = _float_run(SHAPES[3], 0)
    pos, latents, params, G = r["inputs"]
    for subset in ((0,), (1, 2), (3, 4), (5, 6), (0, 5), (2,), tuple(range(7))):
        leaves = [t.clone().requires_grad_(i in subset) for i, t in enumerate((latents,) + params)]
        out = decode_structures(*leaves, pos_emb=pos, native=True)
        assert torch.equal(out, r["out"])
        got = torch.autograd.grad(out, [leaves[i] for i in subset], G)
        for i, g in zip(subset, got):
            assert torch.equal(g, r["grads"][i]), (subset, DR.NAMES[i])
    # nothing wanted: nothing is retained, under no_grad or because no input asks
    with torch.no_grad():
        out = decode_structures(latents.clone().requires_grad_(True), *params, pos_emb=pos, native=True)
    assert out.grad_fn is None and not out.requires_grad and torch.equal(out, r["out"])
    out = decode_structures(latents, *params, pos_emb=pos, native=True)
    assert out.grad_fn is None and torch.equal(out, r["out"])
    # native=None takes the same kernels for these tensors; B = 0 launches nothing
    assert torch.equal(decode_structures(latents, *params, pos_emb=pos), r["out"])
    assert tuple(decode_structures(latents[:0], *params, pos_emb=pos[:0], native=True).shape) == (0, r["out"].shape[1])
    # what the kernels do not cover is refused with the reason, never run some other way
    with pytest.raises(RuntimeError, match="fp32"):
        decode_structures(latents.double(), *(p.double() for p in params), pos_emb=pos.double(), native=True)


# ---- the model through render() and the fused loss ------------------------------------------------------------------------------------
W, H, B_E2E, K_E2E = 160, 112, 300, 8


def _model(native_decode, seed=5):
    torch.manual_seed(seed)
    means = S.make_scene(B_E2E, W, H, 0, seed, zmin=1.0).means3D
    m = LatentGaussianModel(0, means.to(DEV), gaussians_per_structure=K_E2E)
    with torch.no_grad():
        m.structure_scales.fill_(-3.0)           # exp(-3 + decoded): splats of a few pixels
    m.native_decode = native_decode
    return m


def _step(m, cam, bg, target):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    m()
    m._decoded.retain_grad()
    loss = training_loss(render(cam, m, Pipe(), bg)["render"], target, 0.2)
    loss.backward()
    return loss.detach()


def test_model_end_to_end():
    """The rule of tests/test_gpu_structured.py's model check, applied to the decoder: the op is isolated inside the full chain.  The
    gradient that ARRIVED on the decoder's output goes through the restatement's backward, and the decoder's parameter gradients
    are held to the bounds of test_float_data_within_the_derived_bounds (no 1e-5 max|g| rule is used there or here); the torch
    model on the same weights is held to the same bounds, so the two agree within their sum."""
    cam, bg = S.make_camera(W, H).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = (S.make_grad_image(W, H, 3) * 0.5 + 0.5).to(DEV)
    on, off = _model(True), _model(False)
    assert list(on.state_dict().keys()) == list(off.state_dict().keys())
    assert all(torch.equal(a, b) for a, b in zip(on.state_dict().values(), off.state_dict().values()))
    N.profile_enable(True)
    _step(off, cam, bg, target)
    torch.cuda.synchronize()
    prof_off = N.profile_read(64)
    N.profile_enable(True)
    loss0 = _step(on, cam, bg, target)
    torch.cuda.synchronize()
    prof_on = N.profile_read(64)
    N.profile_enable(False)
    assert not [k for k in prof_off if k.startswith("decoder_")], prof_off
    assert prof_on["decoder_fwd"][1] == 1 and prof_on["decoder_bwd"][1] == 1 and prof_on["decoder_reduce"][1] == 1, prof_on
    for name, p in on.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    d = on.decoder
    params = (d.lin0.weight, d.lin0.bias, d.lin1.weight, d.lin1.bias, d.lin2.weight, d.lin2.bias)
    x, p64, g64 = DR.to64(None, on.structure_latents, params, on._decoded.grad)
    fwd = DR.forward(x, *p64)
    assert (np.abs(on._decoded.detach().cpu().numpy() - fwd["out"]) <= DR.forward_bound(x, p64)).all()
    assert (np.abs(off._decoded.detach().cpu().numpy() - fwd["out"]) <= DR.forward_bound(x, p64)).all()
    # a structure on the edge of a ReLU may take the other side in fp32: it is judged by neither side (its row of G counts as 0)
    frag = DR.fragile(x, p64, fwd)
    assert int(frag.sum()) <= max(2, 0.05 * B_E2E)
    g64[frag] = 0.0
    keep = torch.from_numpy(~frag).to(DEV)[:, None]
    leaves = [on.structure_latents.detach().clone().requires_grad_(True)] + [p.detach().clone().requires_grad_(True) for p in params]
    G = on._decoded.grad * keep
    got = torch.autograd.grad(decode_structures(*leaves, native=True), leaves, G)
    ref = torch.autograd.grad(decode_structures(*leaves, native=False), leaves, G)
    want = DR.backward(x, p64, g64, 32, fwd)
    bounds = DR.gradient_bounds(x, p64, g64, 32, fwd)
    for name, g, t, w, b in zip(DR.NAMES, got, ref, want, bounds):
        g, t = g.cpu().numpy().astype(np.float64), t.cpu().numpy().astype(np.float64)
        assert (np.abs(g - w) <= b).all() and (np.abs(t - w) <= b).all() and (np.abs(g - t) <= 2 * b).all(), name
    if not frag.any():                                        # then those ARE the model's gradients, bit for bit (the same kernels)
        assert torch.equal(got[0], on.structure_latents.grad)
        assert all(torch.equal(g, p.grad) for g, p in zip(got[1:], params))
    # 30 Adam steps lower the loss
    on.training_setup(type("Opt", (), {"percent_dense": 0.01})())
    for _ in range(30):
        on.optimizer.zero_grad(set_to_none=True)
        _step(on, cam, bg, target)
        on.optimizer.step()
    on.optimizer.zero_grad(set_to_none=True)
    loss1 = _step(on, cam, bg, target)
    assert float(loss1) < float(loss0), (float(loss0), float(loss1))
