"""GPU checks of the normal-map ops (diff_gaussian_rasterization/normals.py, csrc/gsr_normals.hip): the kernels
against the binary64 restatement (tests/normals_ref.py) under its error rule, element by element, forward and every gradient; what
must be zero is +0.0 in all bits; the inputs are unwritten; two runs give the same bits and a gradient asked for alone has the bits
it has beside the others; render_normals is the hand-made composition bit for bit and its normal map is the oracle's blend of the same
(signed) precomputed colours; train() with lambda_normal, and without it the launches and bits of a run that never reaches the term.
Every check prints the worst ratio error / bound it saw."""
from dataclasses import replace

import numpy as np
import pytest
import torch

import normals_ref as NR
import scene_synth as S
import streams as ST
from test_normals_ref import CASES, GAUSS_CASES, GRAD_LOSS, TX, TY, _gaussian_reference, ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64


def dev(a, grad=False):
    return torch.as_tensor(np.asarray(a)).to(DEV).contiguous().requires_grad_(grad)


def host(t):
    return t.detach().cpu()


# ---- depth_to_normal and the loss -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W, form", CASES)
def test_depth_to_normal_and_the_loss_against_the_reference(H, W, form):
    from diff_gaussian_rasterization.normals import depth_to_normal, normal_consistency_loss
    depth, alpha = NR.make_maps(H, W, form)
    gn, Nm = NR.make_upstream(H, W)
    tag = f"gpu {H}x{W} {form}"
    # the reference, once
    dr, ar = (torch.tensor(v, dtype=F64).requires_grad_(True) for v in (depth, alpha))
    nr = NR.depth_to_normal_ref(dr, ar, TX, TY)
    nr.backward(torch.as_tensor(gn, dtype=F64))
    t = NR.depth_normal_tracked(depth, alpha, TX, TY, grad_n=gn)

    def run(want_d=True, want_a=True):
        d, a = dev(depth[None], want_d), dev(alpha[None], want_a)
        n = depth_to_normal(d, a, TX, TY)
        n.backward(dev(gn))
        return n, d, a
    n, d, a = run()
    assert n.shape == (3, H, W) and d.grad.shape == (1, H, W) and a.grad.shape == (1, H, W)
    assert ST.same_bits(host(d), torch.as_tensor(depth[None])) and ST.same_bits(host(a), torch.as_tensor(alpha[None]))      # unwritten
    assert ratio(host(n), NR.Tracked(nr.detach(), t["n"].e), tag + " n") <= 1
    assert ratio(host(d.grad), NR.Tracked(dr.grad, t["ddepth"].e), tag + " ddepth") <= 1
    assert ratio(host(a.grad), NR.Tracked(ar.grad, t["dalpha"].e), tag + " dalpha") <= 1
    if H < 3 or W < 3:                                                  # every pixel is border: all bits zero
        for z in (n, d.grad, a.grad):
            assert int(host(z).view(torch.int32).abs().max()) == 0
    n2, d2, a2 = run()
    assert ST.same_bits(host(n2), host(n)) and ST.same_bits(host(d2.grad), host(d.grad)) and ST.same_bits(host(a2.grad), host(a.grad))
    _, d3, a3 = run(want_a=False)
    _, d4, a4 = run(want_d=False)
    assert a3.grad is None and d4.grad is None
    assert ST.same_bits(host(d3.grad), host(d.grad)) and ST.same_bits(host(a4.grad), host(a.grad))
    # the loss against the composed binary64 form
    Nt = torch.tensor(Nm, dtype=F64, requires_grad=True)
    dl, al = (torch.tensor(v, dtype=F64).requires_grad_(True) for v in (depth, alpha))
    Lr = NR.normal_consistency_ref(Nt, dl, al, TX, TY)
    Lr.backward(torch.tensor(GRAD_LOSS, dtype=F64))
    tl = NR.depth_normal_tracked(depth, alpha, TX, TY, normal_map=Nm, grad_loss=GRAD_LOSS)

    def run_loss(wN=True, wd=True, wa=True):
        N, d, a = dev(Nm, wN), dev(depth[None], wd), dev(alpha[None], wa)
        L = normal_consistency_loss(N, d, a, TX, TY)
        L.backward(torch.tensor(GRAD_LOSS, device=DEV))
        return L, N, d, a
    L, N, d, a = run_loss()
    r = abs(float(L.detach()) - float(Lr.detach())) / float(tl["loss"].e)
    print(f"{tag} loss: worst error / bound = {r:.3f}")
    assert L.shape == () and r <= 1
    assert ratio(host(N.grad), NR.Tracked(Nt.grad, tl["dN"].e), tag + " dN") <= 1
    assert ratio(host(d.grad), NR.Tracked(dl.grad, tl["ddepth"].e), tag + " ddepth (loss)") <= 1
    assert ratio(host(a.grad), NR.Tracked(al.grad, tl["dalpha"].e), tag + " dalpha (loss)") <= 1
    L2, N2, d2, a2 = run_loss()
    assert ST.same_bits(host(L2), host(L)) and ST.same_bits(host(N2.grad), host(N.grad)) and ST.same_bits(host(d2.grad), host(d.grad))
    assert ST.same_bits(host(a2.grad), host(a.grad))
    _, N3, d3, a3 = run_loss(wd=False, wa=False)
    _, N4, d4, a4 = run_loss(wN=False, wa=False)
    _, N5, d5, a5 = run_loss(wN=False, wd=False)
    assert d3.grad is None and a3.grad is None and N4.grad is None and a4.grad is None and N5.grad is None and d5.grad is None
    assert ST.same_bits(host(N3.grad), host(N.grad)) and ST.same_bits(host(d4.grad), host(d.grad)) and ST.same_bits(host(a5.grad), host(a.grad))


def test_loss_where_a_block_walks_more_than_one_tile():
    """More than 1 024 tiles of 64 x 16 pixels (the loss forward's block cap): the blocks walk two tiles each, the last block adds 1 024 sums."""
    from diff_gaussian_rasterization.normals import normal_consistency_loss
    H, W = 520, 2050                                                    # 33 x 33 tiles
    assert NR.loss_adds(H, W) == 4 * 2 + 10 and NR.loss_adds(64, 256) == 14
    depth, alpha = NR.make_maps(H, W, "holes")
    _, Nm = NR.make_upstream(H, W)
    tl = NR.depth_normal_tracked(depth, alpha, TX, TY, normal_map=Nm, grad_loss=GRAD_LOSS)
    Nt = torch.tensor(Nm, dtype=F64, requires_grad=True)
    dl, al = (torch.tensor(v, dtype=F64).requires_grad_(True) for v in (depth, alpha))
    Lr = NR.normal_consistency_ref(Nt, dl, al, TX, TY)
    Lr.backward(torch.tensor(GRAD_LOSS, dtype=F64))
    N, d, a = dev(Nm, True), dev(depth[None], True), dev(alpha[None], True)
    L = normal_consistency_loss(N, d, a, TX, TY)
    L.backward(torch.tensor(GRAD_LOSS, device=DEV))
    r = abs(float(L.detach()) - float(Lr.detach())) / float(tl["loss"].e)
    print(f"gpu {H}x{W} loss: worst error / bound = {r:.3f}")
    assert r <= 1
    assert ratio(host(N.grad), NR.Tracked(Nt.grad, tl["dN"].e), f"gpu {H}x{W} dN") <= 1
    assert ratio(host(d.grad), NR.Tracked(dl.grad, tl["ddepth"].e), f"gpu {H}x{W} ddepth (loss)") <= 1
    assert ratio(host(a.grad), NR.Tracked(al.grad, tl["dalpha"].e), f"gpu {H}x{W} dalpha (loss)") <= 1
    L2 = normal_consistency_loss(dev(Nm), dev(depth[None]), dev(alpha[None]), TX, TY)
    assert ST.same_bits(host(L2), host(L))


def test_validity_edges_zero_area_and_refusals():
    from diff_gaussian_rasterization.normals import depth_to_normal, normal_consistency_loss
    depth, alpha = NR.make_maps(9, 11, "smooth")
    alpha[4, 5] = np.float32(NR.ALPHA_MIN)                              # exactly the cut-off: valid
    depth[4, 5] = np.float32(3.0) * alpha[4, 5]
    depth[6, 3] = 0.0                                                   # depth 0: invalid
    alpha[2, 8] = np.nextafter(np.float32(NR.ALPHA_MIN), np.float32(0))
    n = host(depth_to_normal(dev(depth), dev(alpha), TX, TY)).numpy()
    assert np.array_equal(np.abs(n).max(0) > 0, NR.normal_mask(NR.valid_mask(depth, alpha)))
    has = np.abs(n).max(0) > 0
    assert has[4, 4] and has[4, 6] and not has[6, 2] and not has[6, 4] and not has[2, 7]
    # a zero-area image: empty tensors, no launch that reads
    for shape in ((0, 5), (4, 0)):
        d = torch.zeros(1, *shape, device=DEV, requires_grad=True)
        out = depth_to_normal(d, torch.zeros(1, *shape, device=DEV), TX, TY)
        assert out.shape == (3, *shape)
        out.sum().backward()
        assert d.grad.shape == (1, *shape)
        with pytest.raises(ValueError, match="no mean"):
            normal_consistency_loss(torch.zeros(3, *shape, device=DEV), d, torch.zeros(1, *shape, device=DEV), TX, TY)
    d, a, N = torch.ones(1, 6, 7, device=DEV), torch.ones(1, 6, 7, device=DEV), torch.zeros(3, 6, 7, device=DEV)
    for bad in (dict(depth=torch.ones(2, 6, 7, device=DEV)), dict(alpha=torch.ones(1, 6, 8, device=DEV)), dict(alpha=a.double()), dict(alpha=a.cpu()),
                dict(depth=torch.ones(1, 6, 7, device=DEV, dtype=torch.int32)), dict(depth=torch.ones(1, 7, 6, device=DEV).transpose(1, 2)),
                dict(alpha=torch.ones(1, 6, 14, device=DEV)[:, :, ::2]), dict(tanfovy=0.0)):
        kw = dict(depth=d, alpha=a, tanfovx=TX, tanfovy=TY)
        kw.update(bad)
        with pytest.raises(ValueError):
            depth_to_normal(**kw)
        with pytest.raises(ValueError):
            normal_consistency_loss(N, **kw)
    for badN in (torch.zeros(3, 6, 8, device=DEV), N.cpu(), N.half(), torch.zeros(6, 7, 3, device=DEV).permute(2, 0, 1)):
        with pytest.raises(ValueError):
            normal_consistency_loss(badN, d, a, TX, TY)
    with pytest.raises(RuntimeError, match="no CPU path"):
        depth_to_normal(d.cpu(), a.cpu(), TX, TY, native=True)
    # native=False on device tensors is the twin, under the same bound
    depth, alpha = NR.make_maps(17, 33, "holes")
    t = NR.depth_normal_tracked(depth, alpha, TX, TY)
    twin = depth_to_normal(dev(depth), dev(alpha), TX, TY, native=False)
    assert ratio(host(twin), NR.Tracked(NR.depth_to_normal_ref(torch.as_tensor(depth, dtype=F64), torch.as_tensor(alpha, dtype=F64), TX, TY), t["n"].e),
                 "device twin n") <= 1


# ---- gaussian_normals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P, logs, unit", GAUSS_CASES)
def test_gaussian_normals_against_the_reference(P, logs, unit):
    from diff_gaussian_rasterization.normals import gaussian_normals
    (s, q, m, V, c, g), out, dq, k, flipped, t = _gaussian_reference(P, logs, unit)
    assert int(t["fragile"].sum()) == 0
    ts, tq, tm = dev(s, True), dev(q, True), dev(m, True)
    o = gaussian_normals(ts, tq, tm, dev(V), dev(c))
    assert o.shape == (P, 3)
    o.backward(dev(g))
    assert ts.grad is None and tm.grad is None and tq.grad.shape == (P, 4)
    if P:
        tag = f"gpu P={P} logs={logs} unit={unit}"
        assert ratio(host(o), NR.Tracked(out, t["out"].e), tag + " normals") <= 1
        assert ratio(host(tq.grad), NR.Tracked(dq, t["dq"].e), tag + " dq") <= 1
    assert ST.same_bits(host(tq), torch.as_tensor(q)) and ST.same_bits(host(ts), torch.as_tensor(s))
    tq2 = dev(q, True)
    o2 = gaussian_normals(dev(s), tq2, dev(m), dev(V), dev(c))
    o2.backward(dev(g))
    assert ST.same_bits(host(o2), host(o)) and ST.same_bits(host(tq2.grad), host(tq.grad))


def test_gaussian_normals_exact_cases_and_refusals():
    from diff_gaussian_rasterization.normals import gaussian_normals
    s, q, m, V, c, want = NR.exact_gaussians()
    got = host(gaussian_normals(dev(s), dev(q), dev(m), dev(V), dev(c))).numpy()
    assert np.array_equal(got, want), got                               # the dot of exactly 0 does not flip; either sign; the ties
    with pytest.raises(ValueError, match="requires grad"):
        gaussian_normals(dev(s), dev(q), dev(m), dev(V, True), dev(c))
    with pytest.raises(ValueError, match="requires grad"):
        gaussian_normals(dev(s), dev(q), dev(m), dev(V), dev(c, True))
    for bad in (dict(scales=dev(s).double()), dict(rotations=dev(q).cpu()), dict(means3D=dev(m)[:4]), dict(rotations=dev(np.ones((5, 8), np.float32))[:, ::2])):
        kw = dict(scales=dev(s), rotations=dev(q), means3D=dev(m), viewmatrix=dev(V), campos=dev(c))
        kw.update(bad)
        with pytest.raises(ValueError):
            gaussian_normals(**kw)


# ---- render_normals -------------------------------------------------------------------------------------------------------------
def _scene_model(P=4000, W=160, H=96, D=1, seed=41):
    from scene import GaussianModel
    scene = S.make_scene(P, W, H, D, seed, scale_lo=0.01, scale_hi=0.08)
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    return scene, gm, S.make_camera(W, H)


def test_render_normals_is_the_composition_and_the_oracles_blend():
    import math

    import oracle
    from diff_gaussian_rasterization.normals import depth_to_normal, gaussian_normals
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_normals
    from util import raster_kwargs
    scene, gm, cam = _scene_model()
    camd, pipe, bg = cam.to(DEV), Pipe(), torch.tensor([0.2, 0.3, 0.1], device=DEV)
    with torch.no_grad():
        before = render(camd, gm, pipe, bg)["render"].clone()
    out = render_normals(camd, gm, pipe)
    assert set(out) == {"normal", "depth", "alpha", "depth_normal", "viewspace_points", "radii", "visibility_filter"}
    # the hand-made composition, bit for bit
    normals = gaussian_normals(gm.get_scaling, gm.get_rotation, gm.get_xyz, camd.world_view_transform, camd.camera_center)
    pkg = render(camd, gm, pipe, torch.zeros(3, device=DEV), override_color=normals, depth_alpha=True)
    tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    want = dict(normal=pkg["render"], depth=pkg["depth"], alpha=pkg["alpha"], depth_normal=depth_to_normal(pkg["depth"], pkg["alpha"], tx, ty),
                radii=pkg["radii"], visibility_filter=pkg["visibility_filter"])
    for key, w in want.items():
        assert ST.same_bits(host(out[key]), host(w)), key
    normal, depth_normal = out["normal"].detach(), out["depth_normal"].detach()
    assert float(normal.min()) < -0.1 and float(normal.max()) > 0.1 and float(depth_normal.abs().max()) > 0.5
    # the normal map is the oracle's blend of the same precomputed colours, negative components and all
    kw = raster_kwargs(scene, cam, colors_precomp=host(normals).numpy().astype(np.float64))
    for name, getter in (("means3D", gm.get_xyz), ("opacities", gm.get_opacity), ("scales", gm.get_scaling), ("rotations", gm.get_rotation)):
        kw[name] = host(getter).numpy()
    fr = oracle.rasterize(dtype=np.float64, **kw)
    assert np.array_equal(host(out["radii"]).numpy(), fr.radii)
    strict = fr.fragile_px == 0
    err = np.abs(host(out["normal"]).numpy() - fr.color).max(0)
    print(f"render_normals vs oracle: max error on {int(strict.sum())} strict pixels {err[strict].max():.2e}")
    assert strict.mean() > 0.5 and err[strict].max() <= 1e-5
    # gradients reach the rotations through both maps, and a plain render() afterwards is what it was
    loss = (out["normal"] * out["depth_normal"]).sum()
    loss.backward()
    assert float(gm._rotation.grad.abs().sum()) > 0 and bool(torch.isfinite(gm._rotation.grad).all()) and bool(torch.isfinite(gm._xyz.grad).all())
    with torch.no_grad():
        after = render(camd, gm, pipe, bg)["render"]
    assert ST.same_bits(host(after), host(before))
    pipe.absgrad = True
    with pytest.raises(ValueError, match="depth_alpha"):
        render_normals(camd, gm, pipe)


def test_sharded_renderer_refuses_normals():
    import types

    from diff_gaussian_rasterization.sharded import ShardedRenderer
    fake_dist = types.SimpleNamespace(get_backend=lambda group=None: "nccl")
    with pytest.raises(ValueError, match="lambda_normal"):
        ShardedRenderer(fake_dist, 1, 0, lambda_normal=0.05)
    with pytest.raises(ValueError, match="render_normals"):
        ShardedRenderer(fake_dist, 1, 0).render_normals(None, None, None)


# ---- train() --------------------------------------------------------------------------------------------------------------------
NORMAL_SCOPES = {"gaussian_normals_fwd", "gaussian_normals_bwd", "normal_consistency_fwd", "normal_consistency_bwd", "depth_normal_fwd",
                 "depth_normal_bwd"}


def _train(iterations=6, **opt_kw):
    import random

    from diff_gaussian_rasterization import _native
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    torch.manual_seed(0)
    random.seed(0)
    W, H = 96, 64
    cams = [c.to(DEV) for c in S.arc_cameras(W, H, 2)]
    scene = S.make_scene(1500, W, H, 1, 30, scale_lo=0.01, scale_hi=0.08)
    truth = GaussianModel(1)
    truth.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    gm = GaussianModel(1)
    gm.adopt_scene(scene, device=DEV)
    with torch.no_grad():
        gm._xyz.add_(0.01 * torch.randn_like(gm._xyz))
    opt = replace(OptimizationDefaults(), **opt_kw)
    gm.training_setup(opt)
    losses = []
    _native.profile_enable(True)
    try:
        train(gm, cams, targets, opt, Pipe(), bg, iterations=iterations, scene_extent=3.0, on_iteration=lambda it, loss, g: losses.append(float(loss.detach())))
        scopes = _native.profile_read(128)
    finally:
        _native.profile_enable(False)
    return gm, losses, scopes


def test_training_loop_with_and_without_the_normal_term():
    off, losses_off, scopes_off = _train()
    assert not NORMAL_SCOPES & set(scopes_off), "the default loop launched a normals kernel"
    # a weight whose first iteration lies behind the window: the same launches, the same bits
    late, losses_late, scopes_late = _train(lambda_normal=0.05)
    assert {k: v[1] for k, v in scopes_late.items()} == {k: v[1] for k, v in scopes_off.items()}
    for name in ("_xyz", "_rotation", "_scaling", "_opacity", "_features"):
        if hasattr(off, name):
            assert ST.same_bits(host(getattr(late, name)), host(getattr(off, name))), name
    assert losses_late == losses_off
    on, losses_on, scopes_on = _train(lambda_normal=0.05, normal_from_iter=3)
    for name in ("gaussian_normals_fwd", "gaussian_normals_bwd", "normal_consistency_fwd", "normal_consistency_bwd"):
        assert scopes_on[name][1] == 4, (name, scopes_on.get(name))              # iterations 3 .. 6: one launch each way
    assert "depth_normal_bwd" not in scopes_on                                   # the fused loss: n is never stored
    assert losses_on[:3] == losses_off[:3] and all(np.isfinite(losses_on))       # the reported loss is the image loss: the same until the term acts
    assert not torch.equal(on._rotation, off._rotation) and bool(torch.isfinite(on._rotation).all())
    with pytest.raises(ValueError, match="lambda_normal"):
        _train(lambda_normal=-1.0)
