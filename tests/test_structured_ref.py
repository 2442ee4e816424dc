"""CPU checks of the latent structured model: the C ABI is additive (two new symbols declared and exported, the five structs
mirrored, the version unchanged) and validates its arguments without touching a GPU; the kernels' own per-child functions
(csrc/gsr_math.h compose_child / compose_child_backward, compiled with g++: tests/structured_host.cpp) agree with the binary64
restatement (tests/structured_ref.py); that restatement, and this package's LatentGaussianModel on host tensors, reproduce what the
reference's own model computed (tests/golden/structured_compose.npz, recorded by tests/golden/make_structured_golden.py); the
exactly representable edge rows come out bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import structured_ref as SR
from diff_gaussian_rasterization.structured import compose_structures
from scene.latent_gaussian_model import LatentGaussianModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_structured_compose_forward", "gsr_structured_compose_backward")
F64 = torch.float64
@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_structured_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert lib.gsr_version() == 12 and "#define GSR_VERSION 12" in hdr


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    one = C.c_void_p(16)
    st = native.Structures(16, 16, 16, 16)
    ch = native.Children(16, 16, 16, 16, 16)
    gout = native.StructuredGrads(16, 16, 16, 16, 16)

    def both(desc, decoded=one, structures=st):
        f = lib.gsr_structured_compose_forward(C.byref(desc), decoded, C.byref(structures), C.byref(ch), None)
        msg_f = lib.gsr_last_error()
        b = lib.gsr_structured_compose_backward(C.byref(desc), decoded, C.byref(structures), C.byref(ch), C.byref(gout), None)
        return f, b, msg_f, lib.gsr_last_error()

    for desc, word in ((native.StructuredDesc(4, 0, 1), b"K = 0"), (native.StructuredDesc(4, 8, 2), b"sh_coeffs = 2"),
                       (native.StructuredDesc(-1, 8, 1), b"B = -1"), (native.StructuredDesc(1 << 25, 8, 1), b"2^28"),
                       (native.StructuredDesc(1 << 14, 1 << 14, 16), b"2^28")):
        f, b, msg_f, msg_b = both(desc)
        assert f == -1 and b == -1 and word in msg_f and word in msg_b, (desc.B, desc.K, desc.sh_coeffs, msg_f, msg_b)
    f, b, msg_f, msg_b = both(native.StructuredDesc(4, 8, 1), decoded=None)
    assert f == -1 and b == -1 and b"decoded" in msg_f and b"decoded" in msg_b
    f, b, msg_f, msg_b = both(native.StructuredDesc(4, 8, 1), structures=native.Structures(16, None, 16, 16))
    assert f == -1 and b == -1 and b"structure" in msg_f and b"structure" in msg_b
    assert both(native.StructuredDesc((1 << 25) - 1, 8, 1), decoded=None)[:2] == (-1, -1)       # in range: the next check speaks
    assert both(native.StructuredDesc(0, 8, 1), decoded=None)[:2] == (0, 0)                     # B = 0: nothing to do, nothing read
    unaligned = native.Children(16, 16, 16, 20, 16)
    assert lib.gsr_structured_compose_forward(C.byref(native.StructuredDesc(4, 8, 1)), one, C.byref(st), C.byref(unaligned), None) == -1
    assert b"16-byte aligned" in lib.gsr_last_error()


def test_python_surface_refuses_bad_shapes():
    z = torch.zeros
    with pytest.raises(ValueError, match="K = 0"):
        compose_structures(z(2, 0), z(2, 3), z(2, 1), z(2, 3), z(2, 4), 0, 1)
    with pytest.raises(ValueError, match="sh_coeffs = 2"):
        compose_structures(z(2, 17), z(2, 3), z(2, 1), z(2, 3), z(2, 4), 1, 2)
    with pytest.raises(ValueError, match="expected"):
        compose_structures(z(2, 15), z(2, 3), z(2, 1), z(2, 3), z(2, 4), 1, 1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compose_structures(z(2, 14), z(2, 3), z(2, 1), z(2, 3), z(2, 4), 1, 1, native=True)


# ---- the torch composition (the CPU path, and the GPU tests' bit-equality baseline) ------------------------------------------------
@pytest.mark.parametrize("B,K,M", [(1, 1, 1), (3, 8, 1), (5, 3, 4), (40, 8, 16), (2, 300, 1)])
def test_torch_composition_against_the_restatement(B, K, M):
    inputs, grads = SR.make_case(B, K, M, 100 + B)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    outs = compose_structures(*leaves, K, M)
    assert [tuple(o.shape) for o in outs] == [(B * K, 3), (B * K, 1), (B * K, 3), (B * K, 4), (B * K, M, 3)]
    d_in = torch.autograd.grad(outs, leaves, grads)
    SR.check_against_ref(B, K, M, inputs, grads, outs, d_in, what=f"torch ({B},{K},{M})")


# ---- the kernels' per-child functions on the host ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def structured_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sh") / "structured_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "structured_host.cpp")])

    def run(c, s, g):
        """c, s, g: [n, 11] fp32 -> (composed, d_c, d_s) [n, 11] fp32 from compose_child / compose_child_backward."""
        d = os.path.dirname(exe)
        rows = torch.cat((c, s, g), 1).to(torch.float32).numpy()
        np.savetxt(os.path.join(d, "in.txt"), rows, fmt="%.9g")
        subprocess.check_call([exe, os.path.join(d, "in.txt"), os.path.join(d, "out.txt")])
        out = torch.from_numpy(np.loadtxt(os.path.join(d, "out.txt"), dtype=np.float32, ndmin=2))
        assert out.shape == (c.shape[0], 33)
        return out[:, :11], out[:, 11:22], out[:, 22:]
    return run


def _as_children(inputs, grads, K):
    """The 11 geometry columns of every child, its structure's 11 and its incoming gradient's 11, as rows."""
    decoded, means, opac, scales, rots = inputs
    B = means.shape[0]
    c = decoded.reshape(B * K, -1)[:, :11]
    s = torch.cat((means, opac, scales, rots), 1).repeat_interleave(K, 0)
    g = torch.cat((grads[0], grads[1], grads[2], grads[3]), 1)
    return c, s, g


def test_compose_child_on_the_host_against_the_restatement(structured_host):
    """K = 1 turns every child into its own structure: the per-child d_s IS the structure gradient, and the whole comparison of
    the GPU tests applies to the g++ build of the very functions the kernels call."""
    B, K, M = 2000, 1, 1
    inputs, grads = SR.make_case(B, K, M, 5)
    c, s, g = _as_children(inputs, grads, K)
    out, d_c, d_s = structured_host(c, s, g)
    outs = (out[:, 0:3], out[:, 3:4], out[:, 4:7], out[:, 7:11], inputs[0][:, 11:].reshape(B, M, 3))
    d_decoded = torch.cat((d_c, grads[4].reshape(B, 3 * M)), 1)
    SR.check_against_ref(B, K, M, inputs, grads, outs, (d_decoded, d_s[:, 0:3], d_s[:, 3:4], d_s[:, 4:7], d_s[:, 7:11]), what="host")


def _edge_rows():
    """(structure rotation, child quaternion, expected composed rotation): exact in fp32."""
    return (((1, 0, 0, 0), (0, 1, 0, 0), (0, 1, 0, 0)),           # w == 0: not flipped
            ((1, 0, 0, 0), (-1, 0, 0, 0), (1, 0, 0, 0)),          # w < 0: flipped
            ((0, 0, 2, 0), (0, 0, 0, 0.5), (0, 1, 0, 0)),         # j k = i, norms 2 and 0.5 divided out exactly
            ((1, 0, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0)))           # a zero child quaternion: a zero row


def test_edge_rows_bit_for_bit(structured_host):
    rows = _edge_rows()
    n = len(rows)
    t = lambda i: torch.tensor([r[i] for r in rows], dtype=torch.float32)
    gen = torch.Generator().manual_seed(3)
    c = torch.randn(n, 11, generator=gen)
    s = torch.randn(n, 11, generator=gen)
    g = torch.randn(n, 11, generator=gen)
    c[:, 7:11], s[:, 7:11] = t(1), t(0)
    want_adds = c[:, :7] + s[:, :7]
    # the host build of the kernels' functions
    out, d_c, d_s = structured_host(c, s, g)
    assert torch.equal(out[:, :7], want_adds) and torch.equal(out[:, 7:11], t(2))
    assert torch.isfinite(d_c).all() and torch.isfinite(d_s).all()
    assert torch.equal(d_c[:, :7], g[:, :7]) and torch.equal(d_s[:, :7], g[:, :7])
    # a zero child quaternion: normalize divided by eps, the clamp passes nothing: d c_q = (dL/d n(c_q)) / 1e-12, d s_rot = 0
    assert not d_s[3, 7:11].any() and d_c[3, 7:11].abs().max() > 1e9
    # the torch composition on the same rows, K = 1 (every child its own structure), no SH beyond three zeros
    leaves = [x.clone().requires_grad_(True) for x in (torch.cat((c, torch.zeros(n, 3)), 1), s[:, 0:3], s[:, 3:4], s[:, 4:7], s[:, 7:11])]
    outs = compose_structures(*leaves, 1, 1)
    assert torch.equal(outs[3], t(2)) and torch.equal(torch.cat(outs[:3], 1), want_adds)
    grads = torch.autograd.grad(outs, leaves, [g[:, 0:3], g[:, 3:4], g[:, 4:7], g[:, 7:11], torch.zeros(n, 1, 3)])
    assert all(torch.isfinite(x).all() for x in grads)
    assert not grads[4][3].any() and grads[0][3, 7:11].abs().max() > 1e9


def test_k_equals_one_is_a_plain_composition():
    inputs, grads = SR.make_case(7, 1, 4, 21)
    outs = compose_structures(*inputs, 1, 4)
    assert torch.equal(outs[0], inputs[0][:, 0:3] + inputs[1]) and torch.equal(outs[1], inputs[0][:, 3:4] + inputs[2])
    assert torch.equal(outs[4], inputs[0][:, 11:].reshape(7, 4, 3))


# ---- the reference's own model, recorded ------------------------------------------------------------------------------------------
COMPOSED = ("_xyz", "_opacity", "_scaling", "_rotation", "_features_dc", "_features_rest")
# The recording is fp32: three layers of fan-in <= 79 (each dot product within n 2^-24 = 5e-6 of sum |a_i b_i|, a few times the
# result here) feed single adds and a normalised product.  2e-5 of a tensor's largest entry (plus as much of 1 for the O(1)
# composed values) is a few times that, and a wrong term or a transposed weight moves entries by the whole of it.
GOLDEN_REL = 2e-5


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(ROOT, "tests", "golden", "structured_compose.npz"))
    cases = {}
    for key in z.files:
        case, rest = key.split("/", 1)
        cases.setdefault(case, {})[rest] = z[key]
    assert set(cases) == {"b5_k8_deg0", "b4_k3_deg1_pos"}
    return cases


def _close(got, want, what):
    want = torch.as_tensor(want).to(F64)
    got = got.detach().to(F64).reshape(want.shape)
    if want.numel() == 0:
        return
    tol = GOLDEN_REL * max(float(want.abs().max()), 1.0)
    err = float((got - want).abs().max())
    assert err <= tol, f"{what}: {err:.3e} > {tol:.3e}"


def _split(outs):
    xyz, opacity, scaling, rotation, features = outs
    return dict(_xyz=xyz, _opacity=opacity, _scaling=scaling, _rotation=rotation, _features_dc=features[:, :1], _features_rest=features[:, 1:])


@pytest.mark.parametrize("case", ["b5_k8_deg0", "b4_k3_deg1_pos"])
def test_restatement_reproduces_the_recorded_reference(golden, case):
    rec = golden[case]
    B, K, deg, pos, latent, hidden = (int(v) for v in rec["meta"])
    M = (deg + 1) ** 2
    state = {k[len("state/"):]: torch.from_numpy(v) for k, v in rec.items() if k.startswith("state/")}
    names = [k for k, v in state.items() if v.is_floating_point() and v.numel() and k != "max_radii2D"]
    leaves = {k: state[k].to(F64).requires_grad_(True) for k in names}
    decoded, outs = SR.model_forward({**state, **leaves}, K, M, bool(pos))
    _close(decoded.reshape(B * K, -1), rec["out/returned"], f"{case} returned")
    parts = _split(outs)
    for k in COMPOSED:
        _close(parts[k], rec["out/" + k], f"{case} {k}")
    loss = sum((parts[k] * torch.from_numpy(rec["w/" + k]).to(F64)).sum() for k in COMPOSED)
    grads = torch.autograd.grad(loss, [leaves[k] for k in names])
    recorded = {k[len("grad/"):] for k in rec if k.startswith("grad/")}
    assert recorded == set(names)
    for k, g in zip(names, grads):
        _close(g, rec["grad/" + k], f"{case} d {k}")


@pytest.mark.parametrize("case", ["b5_k8_deg0", "b4_k3_deg1_pos"])
def test_model_on_the_host_reproduces_the_recorded_reference(golden, case):
    rec = golden[case]
    B, K, deg, pos, latent, hidden = (int(v) for v in rec["meta"])
    state = {k[len("state/"):]: torch.from_numpy(v.copy()) for k, v in rec.items() if k.startswith("state/")}
    model = LatentGaussianModel(deg, torch.zeros(B, 3), latent_size=latent, hidden_size=hidden, gaussians_per_structure=K,
                                use_positional_embedding=bool(pos))
    assert list(model.state_dict().keys()) == list(state.keys())          # the reference's names, in its order
    assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    model.load_state_dict(state)
    returned = model()
    _close(returned, rec["out/returned"], f"{case} returned")
    assert model.packed_features and model._features_dc.shape[1] == 1
    loss = 0.0
    for k in COMPOSED:
        _close(getattr(model, k), rec["out/" + k], f"{case} {k}")
        loss = loss + (getattr(model, k) * torch.from_numpy(rec["w/" + k])).sum()
    loss.backward()
    for k, p in model.named_parameters():
        _close(p.grad, rec["grad/" + k], f"{case} d {k}")


# ---- the model's host logic -------------------------------------------------------------------------------------------------------
def test_model_initial_values_and_freezing():
    torch.manual_seed(0)
    m = LatentGaussianModel(1, torch.randn(6, 3), gaussians_per_structure=3)
    assert torch.allclose(torch.sigmoid(m.structure_opacities), torch.full((6, 1), 0.1)) and (m.structure_scales == 1).all()
    assert m.structure_rotations.shape == (6, 4) and m.structure_latents.shape == (6, 32) and m.decoder.lin2.out_features == 3 * 23
    assert int(m.max_sh_degree) == 1 and int(m.active_sh_degree) == 0
    m.oneupSHdegree(); m.oneupSHdegree()
    assert int(m.active_sh_degree) == 1 and int(m.state_dict()["active_sh_degree"]) == 1
    out = m()
    assert out.shape == (18, 23) and m.get_xyz.shape == (18, 3) and m.get_features.shape == (18, 4, 3)
    assert torch.allclose(m.get_scaling, torch.exp(m._scaling)) and torch.allclose(m.get_opacity, torch.sigmoid(m._opacity))
    assert m.get_covariance().shape == (18, 6)

    def grads_after(flag):
        m.zero_grad()
        m.set_freeze_structures_params(False)
        if flag:
            setattr(m, flag, True)
        m()
        (m._xyz.sum() + m._opacity.sum() + m._scaling.sum() + m._rotation.sum()).backward()
        return {k: p.grad is not None for k, p in m.named_parameters() if k.startswith("structure_") and k != "structure_latents"}
    every = dict(structure_means=True, structure_opacities=True, structure_scales=True, structure_rotations=True)
    assert grads_after(None) == every
    assert grads_after("freeze_structure_means") == {**every, "structure_means": False}
    assert grads_after("freeze_structure_rotations") == {**every, "structure_rotations": False}
    # as the reference: the opacities flag also holds the scales, and the scales flag holds nothing
    assert grads_after("freeze_structure_opacities") == {**every, "structure_opacities": False, "structure_scales": False}
    assert grads_after("freeze_structure_scales") == every
    m.set_freeze_structures_params(True)
    m.zero_grad()
    m()
    m._xyz.sum().backward()
    assert m.structure_means.grad is None and m.structure_latents.grad is not None
    m.training_setup(type("Opt", (), {"percent_dense": 0.01})())
    assert isinstance(m.optimizer, torch.optim.Adam) and m.optimizer.defaults["lr"] == 5e-4 and m.optimizer.defaults["eps"] == 1e-15
    assert len(m.optimizer.param_groups[0]["params"]) == 11
