"""The latent structured model on the GPU: the HIP composition (csrc/gsr_structured.hip through
diff_gaussian_rasterization.structured.compose_structures) against the binary64 restatement (tests/structured_ref.py, whose
check_against_ref holds the bounds and their derivation), bit-equal adds and copies against the fp32 torch composition on the same
device, the same bits from the same inputs, NULL handling both ways, and scene.LatentGaussianModel through render(): gradients on
every parameter, the composition isolated inside the full chain, a falling loss, the fused raw path, persistence."""
import os

import pytest
import torch

import scene_synth as S
import structured_ref as SR
from diff_gaussian_rasterization import _native as N
from diff_gaussian_rasterization.structured import compose_structures
from scene.latent_gaussian_model import LatentGaussianModel

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# the smallest shapes that reach every path: one child; one tile; K no power of two; across a 256-thread block with a tail;
# P = 1.12 M, beyond the capped grids, so every grid-stride loop runs; K > 256: a structure's sum carried over two chunks
SHAPES = [(1, 1, 1), (3, 8, 1), (5, 3, 4), (257, 8, 16), (70_000, 16, 1), (2, 300, 1)]
_RUNS = {}


def _run(shape):
    """One forward and one backward of the HIP composition per shape, shared by the tests below (left unchanged by them)."""
    if shape not in _RUNS:
        B, K, M = shape
        inputs, grads = SR.make_case(B, K, M, 1000 + B, device=DEV)
        leaves = [t.clone().requires_grad_(True) for t in inputs]
        outs = compose_structures(*leaves, K, M)
        d_in = torch.autograd.grad(outs, leaves, grads, retain_graph=True)
        _RUNS[shape] = dict(inputs=inputs, grads=grads, leaves=leaves, outs=outs, d_in=d_in)
    return _RUNS[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_composition_against_the_restatement(shape):
    B, K, M = shape
    r = _run(shape)
    assert [tuple(o.shape) for o in r["outs"]] == [(B * K, 3), (B * K, 1), (B * K, 3), (B * K, 4), (B * K, M, 3)]
    SR.check_against_ref(B, K, M, r["inputs"], r["grads"], r["outs"], r["d_in"], what=f"hip {shape}")


@pytest.mark.parametrize("shape", SHAPES)
def test_adds_and_copies_are_bit_equal_to_the_torch_composition(shape):
    B, K, M = shape
    r = _run(shape)
    leaves = [t.clone().requires_grad_(True) for t in r["inputs"]]
    t_outs = compose_structures(*leaves, K, M, native=False)
    for i, name in ((0, "xyz"), (1, "opacity"), (2, "scaling"), (4, "features")):
        assert torch.equal(r["outs"][i], t_outs[i]), name
    assert (r["outs"][3] - t_outs[3]).abs().max() <= 2 * SR.ROT_ABS
    t_d = torch.autograd.grad(t_outs, leaves, r["grads"])
    D = 11 + 3 * M
    hip, ref = r["d_in"][0].reshape(B * K, D), t_d[0].reshape(B * K, D)
    assert torch.equal(hip[:, :7], ref[:, :7]) and torch.equal(hip[:, 11:], ref[:, 11:])


@pytest.mark.parametrize("shape", [(5, 3, 4), (257, 8, 16), (70_000, 16, 1), (2, 300, 1)])
def test_same_inputs_same_bits(shape):
    r = _run(shape)
    again = torch.autograd.grad(r["outs"], r["leaves"], r["grads"], retain_graph=True)
    for a, b in zip(r["d_in"], again):
        assert torch.equal(a, b)
    outs2 = compose_structures(*r["inputs"], shape[1], shape[2])
    for a, b in zip(r["outs"], outs2):
        assert torch.equal(a, b)


def test_frozen_inputs_and_unused_outputs():
    B, K, M = 257, 8, 16
    r = _run((B, K, M))
    D = 11 + 3 * M
    # a structure tensor that wants no gradient gets None; the others are what they were, bit for bit
    for frozen in range(1, 5):
        leaves = [t.clone().requires_grad_(i != frozen) for i, t in enumerate(r["inputs"])]
        outs = compose_structures(*leaves, K, M)
        d = torch.autograd.grad(outs, [t for t in leaves if t.requires_grad], r["grads"])
        want = [x for i, x in enumerate(r["d_in"]) if i != frozen]
        assert len(d) == 4 and all(torch.equal(a, b) for a, b in zip(d, want)), frozen
    # every structure frozen: d decoded alone (no reduction runs); decoded frozen: the structure sums alone
    leaves = [r["inputs"][0].clone().requires_grad_(True)] + r["inputs"][1:]
    d, = torch.autograd.grad(compose_structures(*leaves, K, M), leaves[:1], r["grads"])
    assert torch.equal(d, r["d_in"][0])
    leaves = [r["inputs"][0]] + [t.clone().requires_grad_(True) for t in r["inputs"][1:]]
    d = torch.autograd.grad(compose_structures(*leaves, K, M), leaves[1:], r["grads"])
    assert all(torch.equal(a, b) for a, b in zip(d, r["d_in"][1:]))
    # only xyz enters the loss: the other incoming gradients are None -> NULL -> zeros in their columns of d decoded
    leaves = [t.clone().requires_grad_(True) for t in r["inputs"]]
    outs = compose_structures(*leaves, K, M)
    d = torch.autograd.grad((outs[0] * r["grads"][0]).sum(), leaves, allow_unused=True)
    dd = d[0].reshape(B * K, D)
    assert torch.equal(dd[:, 0:3], r["grads"][0]) and not dd[:, 3:].any()
    assert torch.equal(d[1], r["d_in"][1]) and not d[2].any() and not d[3].any() and not d[4].any()
    # only the SH table: the geometry columns are zeros
    d = torch.autograd.grad((compose_structures(*leaves, K, M)[4] * r["grads"][4]).sum(), leaves[:1])[0].reshape(B * K, D)
    assert torch.equal(d[:, 11:], r["grads"][4].reshape(B * K, 3 * M)) and not d[:, :11].any()


def test_nothing_is_retained_without_grad():
    B, K, M = 5, 3, 4
    r = _run((B, K, M))
    with torch.no_grad():
        outs = compose_structures(*r["leaves"], K, M)
    assert all(o.grad_fn is None and not o.requires_grad for o in outs)
    assert all(torch.equal(a, b) for a, b in zip(outs, r["outs"]))
    outs = compose_structures(*r["inputs"], K, M)                   # no input wants a gradient
    assert all(o.grad_fn is None for o in outs)
    empty = compose_structures(*[t[:0] for t in r["inputs"]], K, M)  # B = 0: nothing is launched
    assert [tuple(o.shape) for o in empty] == [(0, 3), (0, 1), (0, 3), (0, 4), (0, M, 3)]


# ---- the model through render() ---------------------------------------------------------------------------------------------------
W, H, B_E2E, K_E2E = 64, 48, 400, 8


def _model(deg, seed=5):
    torch.manual_seed(seed)
    means = S.make_scene(B_E2E, W, H, 0, seed, zmin=1.0).means3D
    m = LatentGaussianModel(deg, means.to(DEV), gaussians_per_structure=K_E2E)
    with torch.no_grad():
        m.structure_scales.fill_(-3.0)           # exp(-3 + decoded): splats of a few pixels (the constructor's unit log-scale fills the view)
    for _ in range(deg):
        m.oneupSHdegree()
    return m


@pytest.mark.parametrize("deg", [0, 1])
def test_model_end_to_end(deg):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    M = (deg + 1) ** 2
    m = _model(deg)
    assert m.structure_means.is_cuda and m.decoder.lin0.weight.is_cuda and not m.active_sh_degree.is_cuda
    cam, bg = S.make_camera(W, H).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = (S.make_grad_image(W, H, 3) * 0.5 + 0.5).to(DEV)
    N.profile_enable(True)
    returned = m()
    assert returned.shape == (B_E2E * K_E2E, 11 + 3 * M)
    composed = [m._xyz, m._opacity, m._scaling, m._rotation, m._features]
    for t in [m._decoded] + composed:
        t.retain_grad()
    out = render(cam, m, Pipe(), bg)
    loss0 = (out["render"] - target).abs().mean()
    loss0.backward()
    torch.cuda.synchronize()
    prof = N.profile_read(64)
    N.profile_enable(False)
    # the fused raw path: the composition's two kernels and no activation kernel (exp / normalize / sigmoid ran inside the rasterizer)
    assert prof["structured_fwd"][1] == 1 and prof["structured_bwd"][1] == 1, prof
    assert not [k for k in prof if k.startswith("activations_")], prof
    assert (out["radii"] > 0).sum() > 100
    vs = out["viewspace_points"].grad
    assert vs is not None and torch.isfinite(vs).all() and vs.abs().max() > 0
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
    # the composition inside the full chain: what arrived on the composed tensors, through the restatement's backward
    structures = [m.structure_means, m.structure_opacities, m.structure_scales, m.structure_rotations]
    SR.check_against_ref(B_E2E, K_E2E, M, [m._decoded.detach()] + [p.detach() for p in structures], [t.grad for t in composed],
                         [t.detach() for t in composed], [m._decoded.grad] + [p.grad for p in structures], what=f"model deg {deg}")
    # 30 Adam steps lower the loss
    m.training_setup(type("Opt", (), {"percent_dense": 0.01})())
    for _ in range(30):
        m.optimizer.zero_grad(set_to_none=True)
        m()
        (render(cam, m, Pipe(), bg)["render"] - target).abs().mean().backward()
        m.optimizer.step()
    with torch.no_grad():
        m()
        loss1 = (render(cam, m, Pipe(), bg)["render"] - target).abs().mean()
    assert float(loss1) < float(loss0.detach()), (float(loss0.detach()), float(loss1))


def test_state_dict_and_ply_round_trip(tmp_path):
    from scene import GaussianModel
    m = _model(1)
    with torch.no_grad():
        m()
    path = str(tmp_path / "lgm.pth")
    torch.save(m.state_dict(), path)
    torch.manual_seed(99)
    m2 = LatentGaussianModel(1, torch.zeros(B_E2E, 3, device=DEV), gaussians_per_structure=K_E2E)
    m2.load_state_dict(torch.load(path))
    assert int(m2.active_sh_degree) == 1 and not m2.active_sh_degree.is_cuda
    with torch.no_grad():
        m2()
    for name in ("_xyz", "_opacity", "_scaling", "_rotation", "_features"):
        assert torch.equal(getattr(m, name), getattr(m2, name)), name
    ply = str(tmp_path / "out" / "point_cloud.ply")
    m.save_ply(ply)
    g = GaussianModel(1)
    g.load_ply(ply, device=DEV)
    assert g._xyz.shape == (B_E2E * K_E2E, 3) and g._features.shape == (B_E2E * K_E2E, 4, 3)
    for name in ("_xyz", "_opacity", "_scaling", "_rotation", "_features"):
        assert torch.equal(getattr(g, name).detach(), getattr(m, name)), name
