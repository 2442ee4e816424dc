"""GPU checks of Mip-Splatting's 3D smoothing filter: the HIP kernels (csrc/gsr_filter3d.hip) against the binary64 restatement and
the error rules of tests/filter3d_ref.py (the ones the host build of the same functions meets in tests/test_filter3d_ref.py), at sizes
that cross wave and block edges and camera counts on both sides of the staged chunk; the same inputs give the same bits, and so does
any order of the cameras; render() of a model with a filter is render() of the model with the op's outputs for leaves, bit for bit,
and its gradients are the op's backward of the rasterizer's; the training loop keeps the filter current."""
from dataclasses import replace

import numpy as np
import pytest
import torch
from torch import nn

import filter3d_ref as FR
import scene_synth as S
from diff_gaussian_rasterization.filter3d import apply_filter_3d, compute_filter_3d

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 63, 257, 2049)
F32 = torch.float32


@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", FR.FIXTURES)
def test_compute_in_the_bracket_same_bits_any_camera_order(name, P):
    xyz, cams = FR.fixture(name, P)
    br = FR.compute_bracket(xyz, cams)
    dev_cams = [c.to(DEV) for c in cams]
    got = compute_filter_3d(xyz.to(DEV), dev_cams)
    assert got.shape == (P, 1) and got.dtype == F32 and got.is_cuda
    FR.check_compute(got, br, f"native {name} P={P}")
    assert torch.equal(compute_filter_3d(xyz.to(DEV), cams), got)                       # cameras on the host: the same table
    assert torch.equal(compute_filter_3d(xyz.to(DEV), dev_cams, native=True), got)      # two runs, the same bits
    if len(cams) > 1:
        perm = [dev_cams[i] for i in torch.randperm(len(cams), generator=torch.Generator().manual_seed(3)).tolist()]
        assert torch.equal(compute_filter_3d(xyz.to(DEV), perm), got)
    FR.check_compute(compute_filter_3d(xyz.to(DEV), dev_cams, native=False), br, f"twin on the device {name} P={P}")


def test_compute_past_one_sweep_of_the_finishing_grid():
    """k_filter3d_finish runs at most 1024 blocks of 256: beyond 262 144 Gaussians its loop takes a second turn, and the depth pass
    hands it more partial maxima than one round of its reduction reads."""
    P = 1024 * 256 + 300
    xyz, cams = FR.fixture("posed3", P)
    br = FR.compute_bracket(xyz, cams)
    got = compute_filter_3d(xyz.to(DEV), cams)
    FR.check_compute(got, br, f"native posed3 P={P}")
    assert bool((~br["seen_maybe"][1024 * 256:]).any()) and bool(br["seen_sure"][1024 * 256:].any())      # both rules in the second turn
    assert torch.equal(compute_filter_3d(xyz.to(DEV), cams[::-1]), got)


def test_compute_edge_rows_and_nothing_seen():
    xyz, cams, rows, inside = FR.edge_fixture()
    br = FR.compute_bracket(xyz, cams)
    got = compute_filter_3d(xyz.to(DEV), cams).cpu()
    FR.check_compute(got, br, "native edge")
    k = np.float32(np.sqrt(np.float32(0.2))) / np.float32(64.0)
    fill = xyz[:247][br["seen_sure"][:247], 2].max().numpy()
    want = torch.tensor([np.float32(z) * k if ins else fill * k for z, ins in zip(xyz[rows, 2].numpy(), inside.tolist())])
    assert torch.equal(got[rows, 0], want)
    cam = FR.posed_trio()[0]
    with pytest.raises(ValueError, match="no Gaussian is seen"):
        compute_filter_3d(FR._behind(cam, 300, torch.Generator().manual_seed(1)).to(DEV), [cam])
    assert compute_filter_3d(torch.zeros(0, 3, device=DEV), [cam]).shape == (0, 1)


def _native(inputs, g_o, g_s, raw):
    o, s, f = (t.to(DEV) for t in inputs)
    leaves = [o.clone().requires_grad_(True), s.clone().requires_grad_(True)]
    o_out, s_out = apply_filter_3d(*leaves, f, raw=raw, native=True)
    d_o, d_s = torch.autograd.grad((o_out, s_out), leaves, (g_o.to(DEV), g_s.to(DEV)))
    return o_out.detach(), s_out.detach(), d_o, d_s


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", SIZES)
def test_apply_against_the_restatement(P, raw):
    inputs, g_o, g_s = FR.apply_case(P, 40 + P, raw)
    got = _native(inputs, g_o, g_s, raw)
    FR.check_apply(inputs, g_o, g_s, got, raw, f"native P={P}")
    again = _native(inputs, g_o, g_s, raw)
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    zero = (inputs[2] == 0).reshape(-1)
    if zero.any():
        assert torch.equal(got[0].cpu()[zero], inputs[0][zero]) and torch.equal(got[1].cpu()[zero], inputs[1][zero])
        assert torch.equal(got[2].cpu()[zero], g_o[zero]) and torch.equal(got[3].cpu()[zero], g_s[zero])
    # either gradient alone; [P] opacities and filters
    o, s, f = (t.to(DEV) for t in inputs)
    leaf = s.clone().requires_grad_(True)
    only_s = torch.autograd.grad(apply_filter_3d(o.reshape(-1), leaf, f.reshape(-1), raw=raw)[1], leaf, g_s.to(DEV))[0]
    FR.check_apply(inputs, torch.zeros_like(g_o), g_s, (None, None, None, only_s), raw, f"native scales only P={P}")
    leaf = o.clone().requires_grad_(True)
    only_o = torch.autograd.grad(apply_filter_3d(leaf, s, f, raw=raw)[0], leaf, g_o.to(DEV))[0]
    assert torch.equal(only_o, got[2])


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_apply_extremes_stay_finite(raw):
    inputs = FR.extreme_case(raw)
    n = inputs[1].shape[0]
    got = _native(inputs, torch.ones(n, 1), torch.ones(n, 3), raw)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    FR.check_apply(inputs, torch.ones(n, 1), torch.ones(n, 3), got, raw, "native extremes")      # forward and both gradients
    o, s, f = inputs
    zero = (f == 0).reshape(-1)
    assert torch.equal(got[0].cpu()[zero], o[zero]) and torch.equal(got[1].cpu()[zero], s[zero])
    small = ((f == 1e-6).reshape(-1)) & (s[:, 0] >= (50.0 if raw else 1.0))
    cols = slice(0, 1) if raw else slice(0, 3)
    assert int(small.sum()) >= 3 and torch.equal(got[1].cpu()[small, cols], s[small, cols])


# ---- render() ---------------------------------------------------------------------------------------------------------------------
def _models():
    from scene import GaussianModel
    scene = S.make_scene(2000, 64, 64, 2, 17, scale_lo=0.01, scale_hi=0.08, zmin=0.5)
    cams = [S.make_camera(64, 64).to(DEV)] + [c.to(DEV) for c in S.arc_cameras(64, 64, 2)]
    gm = GaussianModel(2); gm.adopt_scene(scene, device=DEV)
    gm.compute_3D_filter(cams)
    with torch.no_grad():
        logits, log_scales = apply_filter_3d(gm._opacity, gm._scaling, gm.filter_3D, raw=True)
    plain = GaussianModel(2); plain.adopt_scene(scene, device=DEV)
    plain._t["opacity"] = nn.Parameter(logits.detach().clone())
    plain._t["scaling"] = nn.Parameter(log_scales.detach().clone())
    plain._acts.invalidate()
    assert plain.filter_3D is None
    return gm, plain, cams


@pytest.mark.parametrize("antialiasing", [False, True], ids=["plain", "antialiased"])
@pytest.mark.parametrize("fused", [None, False], ids=["raw_path", "getter_path"])
def test_render_with_a_filter_is_render_of_the_filtered_leaves(fused, antialiasing):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    gm, plain, cams = _models()
    pipe = Pipe()
    pipe.fused_activations, pipe.antialiasing = fused, antialiasing
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    weight = S.make_grad_image(64, 64, 3).to(DEV)
    out = {}
    for name, model in (("filter", gm), ("plain", plain)):
        pkg = render(cams[1], model, pipe, bg)
        (pkg["render"] * weight).sum().backward()
        out[name] = pkg
    assert torch.equal(out["filter"]["render"], out["plain"]["render"]) and torch.equal(out["filter"]["radii"], out["plain"]["radii"])
    assert int((out["filter"]["radii"] > 0).sum()) > 500
    assert torch.equal(out["filter"]["viewspace_points"].grad, out["plain"]["viewspace_points"].grad)
    for k in ("xyz", "features", "rotation"):
        assert torch.equal(gm._t[k].grad, plain._t[k].grad), k
    # the leaves' gradients: the op's backward of what the rasterizer returned on the filtered tensors
    g_o, g_s = plain._opacity.grad.cpu(), plain._scaling.grad.cpu()
    assert float(g_o.abs().max()) > 0 and float(g_s.abs().max()) > 0
    inputs = (gm._opacity.detach().cpu(), gm._scaling.detach().cpu(), gm.filter_3D.cpu())
    FR.check_apply(inputs, g_o, g_s, (None, None, gm._opacity.grad, gm._scaling.grad), True, "render leaves")
    # and the filter does something: the unfiltered model renders another image
    with torch.no_grad():
        gm.filter_3D = None
        assert not torch.equal(render(cams[1], gm, pipe, bg)["render"], out["plain"]["render"])


# ---- the training loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strategy, optimizer_type", [("default", "default"), ("mcmc", "sparse_adam")])
def test_training_loop_keeps_the_filter_current(strategy, optimizer_type):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    torch.manual_seed(0)
    W = H = 64
    cams = [c.to(DEV) for c in S.arc_cameras(W, H, 3)]
    scene = S.make_scene(2000, W, H, 2, 30, scale_lo=0.01, scale_hi=0.08, zmin=0.5)
    truth = GaussianModel(2); truth.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    base = replace(OptimizationDefaults(), densify_strategy=strategy, optimizer_type=optimizer_type, mcmc_cap_max=2400, densify_from_iter=5,
                   densification_interval=10, densify_until_iter=35, densify_grad_threshold=1e-6)
    for on in (True, False):
        gm = GaussianModel(2); gm.adopt_scene(scene, device=DEV)
        with torch.no_grad():
            gm._xyz.add_(0.01 * torch.randn_like(gm._xyz))
            gm._opacity[::50] = -7.0
        opt = replace(base, filter_3d=on)
        gm.training_setup(opt)
        counts, seen = [], []

        def on_iteration(it, loss, g):
            assert bool(torch.isfinite(loss.detach())), it
            counts.append(g._xyz.shape[0])
            seen.append(None if g.filter_3D is None else g.filter_3D.shape[0])
        train(gm, cams, targets, opt, Pipe(), bg, iterations=40, scene_extent=3.0, on_iteration=on_iteration)
        assert len(set(counts)) > 1, "the run never changed the number of Gaussians"
        assert seen == (counts if on else [None] * 40)
        if on:
            assert bool(torch.isfinite(gm.filter_3D).all()) and bool((gm.filter_3D > 0).all())
