"""The fused decoder without a device: the C ABI's layouts, exports and refusals (include/gsrast.h gsr_decoder_*), the Python
surface's refusals and routing (diff_gaussian_rasterization/decoder.py), its torch path bit for bit against the model's Decoder,
the binary64 restatement's explicit backward (tests/decoder_ref.py) against float64 autograd, and LatentGaussianModel with
native_decode off (unchanged) and None (the torch path on host tensors: the same bits), down to the recorded reference."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import decoder_ref as DR
from diff_gaussian_rasterization.decoder import decode_structures, decode_structures_torch
from scene.latent_gaussian_model import Decoder, LatentGaussianModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_decoder_workspace_size", "gsr_decoder_forward", "gsr_decoder_backward")
F64 = torch.float64


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_decoder_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared and name in native.EXPORTS and hasattr(lib, name), name
    assert [f for f, _ in native.DecoderDesc._fields_] == ["B", "in_size", "latent_size", "hidden_size", "out_size"]
    assert [f for f, _ in native.DecoderGrads._fields_] == list(DR.NAMES)
    assert lib.gsr_version() == 12


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    one = C.c_void_p(256)
    params = native.DecoderParams(*([one] * 6))
    grads = native.DecoderGrads(*([one] * 7))

    def fwd(desc, pos=None, latents=one, p=params, decoded=one):
        rc = lib.gsr_decoder_forward(C.byref(desc), pos, latents, C.byref(p) if p else None, decoded, None)
        return rc, lib.gsr_last_error()

    def bwd(desc, pos=None, latents=one, p=params, g=grads, G=one, ws=one, ws_bytes=1 << 40):
        rc = lib.gsr_decoder_backward(C.byref(desc), pos, latents, C.byref(p) if p else None, G, C.byref(g) if g else None, ws,
                                      C.c_size_t(ws_bytes), None)
        return rc, lib.gsr_last_error()

    def refused(word, desc, **kw):                       # by both calls, for the same reason (never a complete argument list)
        for rc, msg in (fwd(desc, **kw), bwd(desc, **kw)):
            assert rc == -1 and word in msg, (word, rc, msg)

    D = native.DecoderDesc
    for desc, word in ((D(10, 32, 32, 16, 14), b"hidden_size"), (D(10, 32, 32, 64, 14), b"hidden_size"),
                       (D(10, 129, 32, 32, 14), b"in_size"), (D(10, 32, 0, 32, 14), b"latent_size"),
                       (D(10, 16, 32, 32, 14), b"latent_size"), (D(10, 32, 32, 32, 0), b"out_size"), (D(-1, 32, 32, 32, 14), b"B = -1")):
        refused(word, desc)
        size = C.c_size_t(0)
        assert lib.gsr_decoder_workspace_size(C.byref(desc), C.byref(size)) == -1 and word in lib.gsr_last_error()
    ok = D(10, 32, 32, 32, 14)
    refused(b"latents", ok, latents=None)
    refused(b"pos_emb", ok, pos=one)                      # a positional embedding without room for it in in_size
    refused(b"pos_emb", D(10, 95, 32, 32, 14))           # and room without one
    refused(b"six decoder parameters", ok, p=native.DecoderParams(one, one, one, one, None, one))
    refused(b"16-byte aligned", ok, p=native.DecoderParams(one, one, one, one, C.c_void_p(260), one))
    rc, msg = fwd(ok, decoded=None)
    assert rc == -1 and b"decoded" in msg
    rc, msg = bwd(ok, G=None)
    assert rc == -1 and b"d_decoded" in msg
    rc, msg = bwd(ok, g=None)
    assert rc == -1 and b"grads" in msg
    # the workspace: a function of the desc alone, one partial of OUT 33 + 32 33 + IN 32 + 32 floats per block
    need = native.decoder_workspace_size(ok)
    per_block = 14 * 33 + 32 * 33 + 32 * 32 + 32
    assert per_block * 4 <= need < (per_block + 4) * 4 + 256
    big = native.decoder_workspace_size(D(125_000, 95, 32, 32, 472))
    assert big == native.decoder_workspace_size(D(125_000, 95, 32, 32, 472)) and big <= 256 * (472 * 33 + 32 * 33 + 32 * 95 + 36) * 4 + 256
    for kw in (dict(ws_bytes=need - 1), dict(ws=None), dict(ws_bytes=0)):
        rc, msg = bwd(ok, **kw)
        assert rc == -4 and b"workspace" in msg, kw
    # nothing to do: no structure, or no gradient wanted (not even a workspace is needed then)
    empty = D(0, 32, 32, 32, 14)
    assert fwd(empty, latents=None, p=None, decoded=None)[0] == 0 and bwd(empty, latents=None, p=None, g=None, G=None, ws=None)[0] == 0
    assert bwd(ok, g=native.DecoderGrads(), ws=None, ws_bytes=0)[0] == 0


def _case(B, L, P0, OUT, seed, dtype=torch.float32):
    pos, latents, params, G = DR.float_case(B, L, P0, OUT, seed)
    cast = lambda t: None if t is None else t.to(dtype)
    return cast(pos), cast(latents), tuple(cast(p) for p in params), cast(G)


def test_python_surface_refuses_and_routes():
    pos, latents, params, _ = _case(5, 32, 63, 14, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        decode_structures(latents, *params, pos_emb=pos, native=True)
    with pytest.raises(ValueError, match="shapes do not fit"):
        decode_structures(latents, *params)                                        # w0 expects the positional dims
    with pytest.raises(ValueError, match="shapes do not fit"):
        decode_structures(latents, *params, pos_emb=pos[:4])
    with pytest.raises(ValueError, match="shapes do not fit"):
        decode_structures(latents, *params[:5], params[5][:3], pos_emb=pos)
    with pytest.raises(ValueError, match="expected"):
        decode_structures(latents[0], *params, pos_emb=pos)
    # what the kernels do not cover goes to torch under native=None and is refused with the reason under native=True
    wide = Decoder(32, 64, 14)
    p64 = tuple(p.detach() for p in (wide.lin0.weight, wide.lin0.bias, wide.lin1.weight, wide.lin1.bias, wide.lin2.weight, wide.lin2.bias))
    assert torch.equal(decode_structures(latents, *p64), wide(latents))
    with pytest.raises(RuntimeError, match="hidden_size = 64"):
        decode_structures(latents, *p64, native=True)
    long = Decoder(100, 32, 14, 63)
    pl = tuple(p.detach() for p in (long.lin0.weight, long.lin0.bias, long.lin1.weight, long.lin1.bias, long.lin2.weight, long.lin2.bias))
    x = torch.randn(5, 100)
    assert torch.equal(decode_structures(x, *pl, pos_emb=pos), long(x, pos))
    with pytest.raises(RuntimeError, match="in_size = 163"):
        decode_structures(x, *pl, pos_emb=pos, native=True)
    assert torch.equal(decode_structures(latents.double(), *(p.double() for p in params), pos_emb=pos.double()),
                       decode_structures_torch(latents.double(), *(p.double() for p in params), pos_emb=pos.double()))


@pytest.mark.parametrize("L,P0,OUT", [(32, 0, 112), (7, 0, 69), (32, 63, 472)])
def test_torch_path_is_bit_equal_to_the_model_decoder(L, P0, OUT):
    B = 37
    pos, latents, params, G = _case(B, L, P0, OUT, 3)
    dec = Decoder(L, 32, OUT, P0)
    with torch.no_grad():
        for dst, src in zip((dec.lin0.weight, dec.lin0.bias, dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias), params):
            dst.copy_(src)
    lat_a, lat_b = latents.clone().requires_grad_(True), latents.clone().requires_grad_(True)
    leaves = [p.clone().requires_grad_(True) for p in params]
    want = dec(lat_a, pos)
    for native in (False, None):
        got = decode_structures(lat_b, *leaves, pos_emb=pos, native=native)
        assert torch.equal(got, want)
        d_got = torch.autograd.grad(got, [lat_b] + leaves, G)
        d_want = torch.autograd.grad(want, [lat_a] + list(dec.parameters()), G, retain_graph=True)
        for name, a, b in zip(DR.NAMES, d_got, d_want):
            assert torch.equal(a, b), name


@pytest.mark.parametrize("L,P0,OUT", [(32, 0, 14), (7, 0, 69), (32, 63, 28)])
def test_restatement_backward_against_float64_autograd(L, P0, OUT):
    B = 41
    pos, latents, params, G = _case(B, L, P0, OUT, 5, F64)
    lat = latents.clone().requires_grad_(True)
    leaves = [p.clone().requires_grad_(True) for p in params]
    out = decode_structures_torch(lat, *leaves, pos_emb=pos)
    d_want = torch.autograd.grad(out, [lat] + leaves, G)
    x, p64, g64 = DR.to64(pos, latents, params, G)
    fwd = DR.forward(x, *p64)
    assert np.abs(fwd["out"] - out.detach().numpy()).max() <= 1e-13 * np.abs(fwd["out"]).max()
    for name, got, want in zip(DR.NAMES, DR.backward(x, p64, g64, L, fwd), d_want):
        want = want.numpy()
        assert got.shape == want.shape and np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0), name
    # and the bounds are bounds: the fp32 torch path, summed in whatever order its GEMMs take, lies inside them
    pos32, lat32, par32, G32 = _case(B, L, P0, OUT, 5)
    x, p64, g64 = DR.to64(pos32, lat32, par32, G32)
    fwd = DR.forward(x, *p64)
    frag = DR.fragile(x, p64, fwd)
    g64[frag] = 0.0
    lat = lat32.clone().requires_grad_(True)
    leaves = [p.clone().requires_grad_(True) for p in par32]
    out = decode_structures_torch(lat, *leaves, pos_emb=pos32)
    assert (np.abs(out.detach().numpy() - fwd["out"]) <= DR.forward_bound(x, p64)).all()
    got = torch.autograd.grad(out, [lat] + leaves, torch.from_numpy(g64).float())
    for name, a, want, bound in zip(DR.NAMES, got, DR.backward(x, p64, g64, L, fwd), DR.gradient_bounds(x, p64, g64, L, fwd)):
        assert (np.abs(a.numpy() - want) <= bound).all(), name


def test_integer_data_is_exact_in_any_order():
    """The GPU test's coverage data on the host: below 2^24 everywhere, zeros among the pre-activations, and the fp32 torch path
    already reproduces the restatement bit for bit."""
    for B, L, P0, OUT in ((33, 32, 0, 112), (257, 7, 0, 69), (257, 32, 63, 472)):
        pos, lat, params, G = DR.integer_case(B, L, P0, OUT, B)
        x = lat if pos is None else np.concatenate((pos, lat), 1)
        assert DR.largest_magnitude(x, params, G, L) < 2 ** 24
        fwd = DR.forward(x, *params)
        assert (fwd["z0"] == 0).any() and (fwd["z1"] == 0).any() and (fwd["z0"] > 0).any() and (fwd["z1"] > 0).any()
        t = lambda a: None if a is None else torch.from_numpy(a).float()
        leaves = [t(lat).requires_grad_(True)] + [t(p).requires_grad_(True) for p in params]
        out = decode_structures(*leaves, pos_emb=t(pos))
        assert np.array_equal(out.detach().numpy().astype(np.float64), fwd["out"])
        got = torch.autograd.grad(out, leaves, t(G))
        for name, a, want in zip(DR.NAMES, got, DR.backward(x, params, G, L, fwd)):
            assert np.array_equal(a.numpy().astype(np.float64), want), name


@pytest.mark.parametrize("pos", [False, True])
def test_model_flag_off_is_unchanged_and_none_is_the_same_bits_on_the_host(pos):
    torch.manual_seed(11)
    m = LatentGaussianModel(1, torch.randn(9, 3), gaussians_per_structure=3, use_positional_embedding=pos)
    assert m.native_decode is False
    names = list(m.state_dict().keys())
    noise = torch.randn(9, 32) * 0.1

    def run():
        m.zero_grad(set_to_none=True)
        returned = m(noise)
        loss = sum((getattr(m, k) * (i + 1.5)).sum() for i, k in enumerate(("_xyz", "_opacity", "_scaling", "_rotation", "_features")))
        loss.backward()
        return returned.detach().clone(), m._decoded.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters()}

    off = run()
    # off: the module call itself
    from scene.latent_gaussian_model import positional_embedding
    emb = positional_embedding(m.structure_means.detach(), 10) if pos else None
    assert torch.equal(off[1], m.decoder(m.structure_latents + noise, emb))
    m.native_decode = None
    auto = run()
    assert list(m.state_dict().keys()) == names
    assert torch.equal(off[0], auto[0]) and torch.equal(off[1], auto[1])
    assert off[2].keys() == auto[2].keys() and all(torch.equal(off[2][k], auto[2][k]) for k in off[2])
    m.native_decode = True
    with pytest.raises(RuntimeError, match="no CPU path"):
        m()


@pytest.mark.parametrize("case", ["b5_k8_deg0", "b4_k3_deg1_pos"])
def test_recorded_reference_through_the_new_entry_point(case):
    z = np.load(os.path.join(ROOT, "tests", "golden", "structured_compose.npz"))
    rec = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(case + "/")}
    B, K, deg, pos, latent, hidden = (int(v) for v in rec["meta"])
    state = {k[len("state/"):]: torch.from_numpy(v.copy()) for k, v in rec.items() if k.startswith("state/")}
    model = LatentGaussianModel(deg, torch.zeros(B, 3), latent_size=latent, hidden_size=hidden, gaussians_per_structure=K,
                                use_positional_embedding=bool(pos))
    model.load_state_dict(state)
    model.native_decode = None
    returned = model()

    def close(got, want, what):
        want = torch.as_tensor(want).to(F64)
        err = float((got.detach().to(F64).reshape(want.shape) - want).abs().max()) if want.numel() else 0.0
        assert err <= 2e-5 * max(float(want.abs().max()) if want.numel() else 0.0, 1.0), f"{what}: {err:.3e}"

    close(returned, rec["out/returned"], f"{case} returned")
    composed = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")
    loss = 0.0
    for k in composed:
        close(getattr(model, k), rec["out/" + k], f"{case} {k}")
        loss = loss + (getattr(model, k) * torch.from_numpy(rec["w/" + k])).sum()
    loss.backward()
    for k, p in model.named_parameters():
        close(p.grad, rec["grad/" + k], f"{case} d {k}")
