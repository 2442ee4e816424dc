"""The extra-colour channels (GaussianRasterizer(..., depth_alpha=True)(..., extra_colors=t)) on the GPU.

Bits: the frame's other outputs are those of the call without extra colours, the extra map is the colour of the same geometry rendered
with colors_precomp = t over a zero background, and both forward kernels render it alike.  Gradients: by linearity the float64
reference of L = <g_c, C> + <g_z, depth> + <g_a, alpha> + <g_e, extra> is the sum of three oracle backwards (tests/test_extra_abi.py pins
the construction against torch autograd): test_gpu_depth_alpha._want plus the backward of oracle.rasterize(colors_precomp = t, bg = 0)
for g_e, whose colors_precomp gradient is dL/dt; every Gaussian under test_gpu_parity._check_grads' bound, dL/dt under the rule it
applies to the SH coefficients.  Extra colours are signed, uniform in [-1, 1].  The oracle frames of a scene are computed once and shared."""
import os
import random
import subprocess
import sys
from dataclasses import replace

import numpy as np
import pytest
import torch

import oracle
import scene_synth as S
import streams as ST
from test_gpu_depth_alpha import G1_CASES, _assert_multi_chunk, _aux_oracle, _uncovered_half_kwargs, _upstream, _want
from test_gpu_parity import DEV, _check_grads, _fixture_kwargs, _inputs, _settings, _strict_pixels

pytestmark = pytest.mark.gpu

CASES = G1_CASES + ["uncovered half"]
_id = lambda c: c if isinstance(c, str) else f"P{c['P']}_{c['W']}x{c['H']}_s{c['seed']}" + (f"_pose{c['pose']}" if "pose" in c else "")
MID = dict(P=2048, W=128, H=128, D=3, seed=105)          # (make_scene's scales for P > 64 are test_g1_raw_path_through_render's)
_KW, _REF = {}, {}


def _kwargs(c):
    key = _id(c)
    if key not in _KW:
        kw = _uncovered_half_kwargs() if isinstance(c, str) else _fixture_kwargs(c)
        P = np.asarray(kw["means3D"]).shape[0]
        extra = torch.rand(P, 3, generator=torch.Generator().manual_seed(7 + P), dtype=torch.float64).numpy() * 2 - 1
        _KW[key] = (kw, extra.astype(np.float32))
    return _KW[key]


def _reference(c):
    """(SH frame, (z, 1, 0) frame, z, extra frame) of the float64 oracle, once per scene; never modified."""
    key = _id(c)
    if key not in _REF:
        kw, extra = _kwargs(c)
        par = isinstance(c, str)
        fr_aux, z = _aux_oracle(kw, parallel=par)
        ekw = {k: v for k, v in kw.items() if k != "shs"}
        ekw.update(colors_precomp=extra.astype(np.float64), bg=np.zeros(3))
        _REF[key] = (oracle.rasterize(dtype=np.float64, parallel=par, **kw), fr_aux, z, oracle.rasterize(dtype=np.float64, parallel=par, **ekw))
    return _REF[key]


def _render(kw, extra, grad=True, debug=False):
    """-> ((color, radii, depth, alpha[, extra map]), geometry leaves, means2D, the extra leaf or None)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, grad)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=grad)
    t = None if extra is None else torch.as_tensor(extra, dtype=torch.float32).to(DEV).requires_grad_(grad)
    more = {} if t is None else {"extra_colors": t}
    return GaussianRasterizer(_settings(kw, debug), depth_alpha=True)(means2D=means2D, **inp, **more), inp, means2D, t


def _bits(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy())


def _debug_views(kw):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    inp = _inputs(kw, False)
    _, _, fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, _settings(kw), aux=True)
    torch.cuda.synchronize()
    return N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan), N.bwd_segment_entries()


# ---- 1. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_bits_of_every_output(c):
    import diff_gaussian_rasterization as dgr
    kw, extra = _kwargs(c)
    if isinstance(c, str):
        _assert_multi_chunk(kw)                      # the maps are carried between chunks, the chunk-start planes are written
    with torch.no_grad():
        (c0, r0, d0, a0), _, _, _ = _render(kw, None, grad=False)
        (c1, r1, d1, a1, e1), inp, _, t = _render(kw, extra, grad=False)
        assert _bits(c0, c1) and _bits(r0, r1) and _bits(d0, d1) and _bits(a0, a1)
        assert e1.shape == (3,) + tuple(c1.shape[1:]) and float(e1.min()) < -0.01 and float(e1.max()) > 0.01
        # the colour of the same geometry with colors_precomp = extra over a zero background
        rs0 = _settings(kw)._replace(bg=torch.zeros(3, device=DEV))
        c2, r2, _ = dgr.rasterize_forward(inp["means3D"], None, t, inp["opacities"], inp["scales"], inp["rotations"], None, rs0)
        assert _bits(r2, r1) and _bits(c2, e1)
        # (z, 1, 0): channel 0 is the depth map's bits, channel 1 the alpha map to the bound of _check_maps, channel 2 nothing
        views, seg = _debug_views(kw)
        z = views["splat_records"][:, 9].clone()
        zc = torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1).contiguous()
        (_, _, d3, a3, e3), _, _, _ = _render(kw, zc.cpu().numpy(), grad=False)
        assert _bits(e3[0], d3[0]) and _bits(d3, d1)
        err = float((e3[1] - a3[0]).abs().max())
        print(f"{_id(c)}: |extra[1] - alpha| max {err:.2e}")
        assert err <= 1e-5 and float(e3[2].abs().max()) == 0.0
        if isinstance(c, str):
            assert int(views["tile_walk"].max()) > seg


def _child_maps(out, which):
    kw, extra = _kwargs(dict(P=5000, W=256, H=192, D=3, seed=109) if which == "big" else MID)
    with torch.no_grad():
        (_, _, _, alpha, emap), _, _, _ = _render(kw, extra, grad=False)
    np.save(out, np.concatenate([emap.cpu().numpy(), alpha.cpu().numpy()]))


@pytest.mark.parametrize("which", ["big"])
def test_both_forward_kernels_render_the_same_extra_map(tmp_path, which):
    outs = []
    for forced in ("0", "1"):                        # (GSR_FWD_GROUPS is read when the library loads: a child process each)
        out = str(tmp_path / f"maps{forced}.npy")
        env = dict(os.environ, GSR_FWD_GROUPS=forced, PYTHONPATH=os.pathsep.join(sys.path))
        subprocess.run([sys.executable, os.path.abspath(__file__), out, which], check=True, env=env, timeout=300)
        outs.append(np.load(out))
    assert outs[0][3].max() > 0.5 and np.abs(outs[0][:3]).max() > 0.1
    assert np.array_equal(outs[0], outs[1])


# ---- 2., 3. gradients against float64 ----------------------------------------------------------------------------------------------
NAMES = ["means3D", "means2D", "opacities", "shs", "scales", "rotations", "extra_colors"]


def _gradients(c, which=("color", "depth", "alpha", "extra"), check_walk=False):
    """The frame's gradients for the upstream gradients named in `which` (the others absent: None reaches the backward) against the
    reference, every Gaussian strict.  -> (live Gaussians, got)"""
    kw, extra = _kwargs(c)
    multi = isinstance(c, str)
    fr_sh, fr_aux, z, fr_ext = _reference(c)
    H, W = kw["image_height"], kw["image_width"]
    (color, radii, depth, alpha, emap), inp, means2D, t = _render(kw, extra)
    strict = _strict_pixels(fr_sh, radii.cpu().numpy()) & (fr_aux.fragile_px == 0) & (fr_ext.fragile_px == 0)
    err = np.abs(emap.detach().cpu().numpy() - fr_ext.color).max(0)
    print(f"{_id(c)} {'+'.join(which)}: extra map max error on {int(strict.sum())} strict pixels {err[strict].max():.2e}")
    assert err[strict].max() <= 1e-5                                         # (|extra| <= 1: the colour image's bound)
    seed = 17 if multi else c["seed"]
    gc, gz, ga = _upstream(H, W, seed, float(np.abs(z).max()))
    ge = S.make_grad_image(W, H, seed + 1).numpy().astype(np.float64)
    gc, gz, ga, ge = (gc * strict[None] if "color" in which else np.zeros_like(gc), gz * strict if "depth" in which else np.zeros_like(gz),
                      ga * strict if "alpha" in which else np.zeros_like(ga), ge * strict[None] if "extra" in which else np.zeros_like(ge))
    dev = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    pairs = [(color, dev(gc), "color"), (depth, dev(gz)[None], "depth"), (alpha, dev(ga)[None], "alpha"), (emap, dev(ge), "extra")]
    torch.autograd.backward([o for o, _, n in pairs if n in which], [g for _, g, n in pairs if n in which])
    got = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    got["means2D"], got["extra_colors"] = means2D.grad.detach().cpu().numpy(), t.grad.detach().cpu().numpy()
    want = _want(fr_sh, fr_aux, kw, gc, gz, ga, parallel=multi)
    wext = fr_ext.backward(ge, parallel=multi)
    for n in ("means3D", "means2D", "opacities", "scales", "rotations"):
        want[n] = want[n] + wext[n]
    want["extra_colors"] = wext["colors_precomp"]
    live, strict_live = _check_grads(fr_sh, want, got, NAMES, masked=True)
    assert strict_live == live
    if "extra" not in which:
        assert not got["extra_colors"].any()
    if "color" not in which:
        assert not got["shs"].any()
    if check_walk:                                   # some tile walked more than kSeg entries: a segment checkpoint of the new planes was read
        views, seg = _debug_views(kw)
        assert int(views["tile_walk"].max()) > seg, (int(views["tile_walk"].max()), seg)
    return live, got


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gradients_against_the_oracle(c):
    multi = isinstance(c, str)
    live, got = _gradients(c, check_walk=multi)
    assert live > (1000 if multi else 0) and np.abs(got["extra_colors"]).max() > 0
    P = got["extra_colors"].shape[0]
    kw, _ = _kwargs(c)
    # a Gaussian without a row gets exactly 0 (and nothing but the visible ones owns rows)
    fr_sh = _reference(c)[0]
    assert not got["extra_colors"][fr_sh.radii == 0].any() and got["extra_colors"].shape == (P, 3)


@pytest.mark.parametrize("which", ["color", "depth", "alpha", "extra"])
def test_partial_upstream_gradients(which):
    live, got = _gradients(MID, which=(which,))
    assert live > 0
    if which == "extra":
        assert np.abs(got["extra_colors"]).max() > 0 and np.abs(got["means3D"]).max() > 0


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------
def test_the_same_frame_gives_the_same_gradient_bits():
    kw, extra = _kwargs(dict(P=5000, W=256, H=192, D=3, seed=109))
    runs = []
    for _ in range(2):
        (color, radii, depth, alpha, emap), inp, means2D, t = _render(kw, extra)
        g = torch.Generator().manual_seed(3)
        ups = [torch.rand(o.shape, generator=g).to(DEV) - 0.5 for o in (color, depth, alpha, emap)]
        torch.autograd.backward([color, depth, alpha, emap], ups, retain_graph=True)
        first = {k: v.grad.clone() for k, v in {**inp, "means2D": means2D, "extra": t}.items()}
        for v in list(inp.values()) + [means2D, t]:
            v.grad = None
        torch.autograd.backward([color, depth, alpha, emap], ups)          # a second backward of the same frame
        for k, v in {**inp, "means2D": means2D, "extra": t}.items():
            assert ST.same_bits(first[k], v.grad), k
        runs.append({**{k: v.cpu() for k, v in first.items()}, "map": emap.detach().cpu()})
    for k in runs[0]:
        assert ST.same_bits(runs[0][k], runs[1][k]), k
    assert float(runs[0]["extra"].abs().max()) > 0


# ---- 5., 6. render(), render_with_normals() -------------------------------------------------------------------------------------------
def _model(D=3, seed=105, P=2048, W=128, H=128):
    from scene import GaussianModel
    scene, cam = S.make_scene(P, W, H, D, seed, scale_lo=0.005, scale_hi=0.06), S.make_camera(W, H)
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    return gm, cam.to(DEV)


def test_raw_path_through_render_matches_the_getter_path():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    fr_sh, fr_aux, z, fr_ext = _reference(MID)
    _, extra = _kwargs(MID)
    gm, cam = _model()
    t = torch.as_tensor(extra).to(DEV).requires_grad_(True)
    bg = torch.zeros(3, device=DEV)
    raw = render(cam, gm, Pipe(), bg, depth_alpha=True, extra_colors=t)
    assert set(raw) >= {"render", "radii", "depth", "alpha", "extra", "viewspace_points", "visibility_filter"}
    pipe = Pipe()
    pipe.fused_activations = False
    with torch.no_grad():
        get = render(cam, gm, pipe, bg, depth_alpha=True, extra_colors=t)
        plain = render(cam, gm, Pipe(), bg, depth_alpha=True)
    assert "extra" not in plain and ST.same_bits(plain["render"], raw["render"].detach()) and ST.same_bits(plain["depth"], raw["depth"].detach())
    strict = (fr_sh.fragile_px == 0) & (fr_aux.fragile_px == 0) & (fr_ext.fragile_px == 0)
    zmax = float(np.abs(z).max())
    host = lambda v: v.detach().cpu().numpy()
    # the bounds of test_g1_raw_path_through_render (_check_maps): 1e-5 zmax on the depth, 1e-5 on alpha - and on the extra map, |t| <= 1
    assert np.abs(host(raw["depth"]) - host(get["depth"]))[0][strict].max() <= 1e-5 * zmax
    assert np.abs(host(raw["alpha"]) - host(get["alpha"]))[0][strict].max() <= 1e-5
    err = np.abs(host(raw["extra"]) - host(get["extra"])).max(0)[strict].max()
    print(f"raw path vs getter path: extra map max difference {err:.2e}")
    assert err <= 1e-5 and np.abs(host(raw["extra"]) - fr_ext.color).max(0)[strict].max() <= 1e-5
    raw["extra"].sum().backward()
    assert float(t.grad.abs().max()) > 0 and float(gm._xyz.grad.abs().max()) > 0 and bool(torch.isfinite(gm._rotation.grad).all())


@pytest.mark.parametrize("fused", [False, None], ids=["getter path", "raw path"])
def test_render_with_normals_is_render_plus_render_normals_in_one_frame(fused):
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_normals, render_with_normals
    gm, cam = _model()
    pipe = Pipe()
    pipe.fused_activations = fused
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        one = render_with_normals(cam, gm, pipe, bg)
        color = render(cam, gm, pipe, bg)
        two = render_normals(cam, gm, pipe)
    assert set(one) >= {"render", "radii", "viewspace_points", "visibility_filter", "normal", "depth", "alpha", "depth_normal"}
    assert ST.same_bits(one["render"], color["render"]) and ST.same_bits(one["radii"], color["radii"])
    assert float(one["normal"].min()) < -0.1 and float(one["normal"].max()) > 0.1 and float(one["depth_normal"].abs().max()) > 0.5
    if fused is False:                               # both use the same activations: the two-frame maps, bit for bit
        for k in ("normal", "depth", "alpha", "depth_normal"):
            assert ST.same_bits(one[k], two[k]), k
    else:
        assert float((one["normal"] - two["normal"]).abs().max()) <= 1e-3
    one = render_with_normals(cam, gm, pipe, bg)
    (one["normal"] * one["depth_normal"]).sum().backward()
    assert float(gm._rotation.grad.abs().sum()) > 0 and bool(torch.isfinite(gm._rotation.grad).all()) and bool(torch.isfinite(gm._xyz.grad).all())
    pipe.absgrad = True
    with pytest.raises(ValueError, match="depth_alpha"):
        render_with_normals(cam, gm, pipe, bg)


def test_antialiasing_fused_getters_and_the_3d_filter():
    """The switches the call composes with: the other outputs keep the bits of the same call without extra colours, and the extra map
    is the colour of the same switch's frame fed the triple over a zero background."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_params import Pipe
    from gaussian_renderer import render
    kw, extra = _kwargs(MID)
    t = torch.as_tensor(extra).to(DEV)
    rs = _settings(kw)
    rs0 = rs._replace(bg=torch.zeros(3, device=DEV))
    with torch.no_grad():
        inp = _inputs(kw, False)
        m2 = torch.zeros(t.shape[0], 3, device=DEV)
        # antialiasing=True
        aa = GaussianRasterizer(rs, depth_alpha=True, antialiasing=True)
        c0, r0, d0, a0 = aa(means2D=m2, **inp)
        c1, r1, d1, a1, e1 = aa(means2D=m2, extra_colors=t, **inp)
        geom = {k: v for k, v in inp.items() if k != "shs"}
        c2, _ = GaussianRasterizer(rs0, antialiasing=True)(means2D=m2, colors_precomp=t, **geom)
        assert _bits(c0, c1) and _bits(d0, d1) and _bits(a0, a1) and _bits(r0, r1) and _bits(c2, e1)
        plain = GaussianRasterizer(rs, depth_alpha=True)(means2D=m2, extra_colors=t, **inp)[4]
        assert not _bits(plain, e1)                                  # (the compensated opacity is what gets blended)
    # FUSE_GETTERS: the getters' outputs over leaves are rendered from the leaves, with the extra colours
    g = torch.Generator().manual_seed(5)
    P, M = inp["shs"].shape[0], inp["shs"].shape[1]
    leaf = lambda v: v.detach().clone().to(DEV).requires_grad_(True)
    xyz, dc, rest = leaf(inp["means3D"]), leaf(inp["shs"][:, :1]), leaf(inp["shs"][:, 1:])
    op, sc, rot = leaf(torch.logit(inp["opacities"].clamp(1e-4, 1 - 1e-4))), leaf(inp["scales"].log()), leaf(inp["rotations"] * 1.5)
    te = leaf(t)
    rast = GaussianRasterizer(rs, depth_alpha=True)

    def getters(**more):
        return rast(means3D=xyz, means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), opacities=torch.sigmoid(op),
                    shs=torch.cat((dc, rest), 1), scales=torch.exp(sc), rotations=torch.nn.functional.normalize(rot), **more)
    was = dgr.FUSE_GETTERS
    dgr.FUSE_GETTERS = True
    try:
        f0 = getters()
        f1 = getters(extra_colors=te)
        assert type(f1[0].grad_fn).__name__.startswith("_RasterizeGaussiansRaw")
    finally:
        dgr.FUSE_GETTERS = was
    with torch.no_grad():
        raw = rast.forward_raw(xyz, torch.zeros(P, 3, device=DEV), dc, rest, op, sc, rot, extra_colors=te)
    assert len(f1) == 5 and all(_bits(x, y) for x, y in zip(f0, f1[:4])) and _bits(f1[4], raw[4])
    f1[4].sum().backward()
    assert float(te.grad.abs().max()) > 0 and float(op.grad.abs().max()) > 0 and float(rot.grad.abs().max()) > 0
    # a model with a 3D filter, through render() on the getter path
    gm, cam = _model()
    gm.compute_3D_filter([cam])
    assert gm.filter_3D is not None
    pipe = Pipe()
    pipe.fused_activations = False
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        a = render(cam, gm, pipe, bg, depth_alpha=True)
        b = render(cam, gm, pipe, bg, depth_alpha=True, extra_colors=t)
        c = render(cam, gm, pipe, torch.zeros(3, device=DEV), override_color=t)
        d = render(cam, gm, Pipe(), bg, depth_alpha=True, extra_colors=t)            # the raw path: it runs, the same shape
    assert all(ST.same_bits(a[k], b[k]) for k in ("render", "depth", "alpha", "radii")) and ST.same_bits(b["extra"], c["render"])
    assert d["extra"].shape == b["extra"].shape and bool(torch.isfinite(d["extra"]).all())


# ---- 7. train() ----------------------------------------------------------------------------------------------------------------------
def _train(iterations=20, seed=0, **opt_kw):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    torch.manual_seed(seed)
    random.seed(seed)
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
    losses, forwards = [], [0]
    inner = dgr.rasterize_forward

    def counted(*a, **k):
        forwards[0] += 1
        return inner(*a, **k)
    dgr.rasterize_forward = counted
    _native.profile_enable(True)
    try:
        train(gm, cams, targets, opt, Pipe(), bg, iterations=iterations, scene_extent=3.0, on_iteration=lambda it, loss, g: losses.append(float(loss.detach())))
        scopes = _native.profile_read(128)
    finally:
        _native.profile_enable(False)
        dgr.rasterize_forward = inner
    return gm, losses, {k: v[1] for k, v in scopes.items()}, forwards[0]


def test_training_with_the_normals_in_the_colour_frame():
    kw = dict(lambda_normal=0.05, normal_from_iter=5)
    two_a, loss_a, scopes_a, fwd_a = _train(seed=0, **kw)
    two_b, loss_b, scopes_b, fwd_b = _train(seed=1, **kw)
    one, loss_1, scopes_1, fwd_1 = _train(seed=0, normal_in_frame=True, **kw)
    # iterations 1 .. 4: one frame each; 5 .. 20: two frames each on the two-frame path, one on the one-frame path
    assert fwd_a == fwd_b == 4 + 2 * 16 and fwd_1 == 20
    assert scopes_1.get("render_fwd_ext", 0) >= 16 and scopes_1.get("render_bwd_ext", 0) == 16 and "render_fwd_ext" not in scopes_a
    assert loss_1[:4] == loss_a[:4] and all(np.isfinite(loss_1)) and bool(torch.isfinite(one._rotation).all())
    assert not torch.equal(one._rotation, two_a._rotation)
    # the final image loss: within the two-frame run's by what two two-frame runs of different seeds differ by
    # (the mean of the last four reported image losses: a single one depends on which camera the iteration drew)
    tail = lambda l: float(np.mean(l[-4:]))
    margin = abs(tail(loss_a) - tail(loss_b))
    print(f"final loss (mean of 4): two frames {tail(loss_a):.6f} (other seed {tail(loss_b):.6f}), one frame {tail(loss_1):.6f}; margin {margin:.2e}")
    assert margin > 0 and abs(tail(loss_1) - tail(loss_a)) <= margin
    # the flag off: the two-frame loop's launches and bits
    off, loss_off, scopes_off, fwd_off = _train(seed=0, normal_in_frame=False, **kw)
    assert scopes_off == scopes_a and fwd_off == fwd_a and loss_off == loss_a
    for name in ("_xyz", "_rotation", "_scaling", "_opacity", "_features"):
        assert ST.same_bits(getattr(off, name).detach().cpu(), getattr(two_a, name).detach().cpu()), name


# ---- 8. refusals that need a device tensor ----------------------------------------------------------------------------------------------
def test_refusals_on_the_device():
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization.contrib import ContributionStats
    kw, extra = _kwargs(G1_CASES[0])
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    m2 = torch.zeros(P, 3, device=DEV)
    ok = torch.as_tensor(extra).to(DEV)
    call = lambda rast, t: rast(means2D=m2, extra_colors=t, **inp)
    with pytest.raises(ValueError, match="the frame's inputs live on"):
        call(GaussianRasterizer(_settings(kw), depth_alpha=True), ok.cpu())
    with pytest.raises(ValueError, match="shape"):
        call(GaussianRasterizer(_settings(kw), depth_alpha=True), ok[:-1])
    with pytest.raises(ValueError, match="dtype"):
        call(GaussianRasterizer(_settings(kw), depth_alpha=True), ok.double())
    with pytest.raises(ValueError, match="depth_alpha=True"):
        call(GaussianRasterizer(_settings(kw)), ok)
    with pytest.raises(ValueError, match="absgrad"):
        call(GaussianRasterizer(_settings(kw), absgrad=True), ok)
    with pytest.raises(ValueError, match="contributions"):
        call(GaussianRasterizer(_settings(kw), contributions=ContributionStats(P, device=DEV)), ok)
    rs = _settings(kw)
    with pytest.raises(ValueError, match="camera gradients"):
        call(GaussianRasterizer(rs._replace(viewmatrix=rs.viewmatrix.clone().requires_grad_(True)), depth_alpha=True), ok)
    # an empty scene, and debug=True: the same maps
    empty = {k: (v[:0] if k in ("means3D", "opacities", "shs", "scales", "rotations") else v) for k, v in kw.items()}
    (_, _, _, _, e0), _, _, _ = _render(empty, np.zeros((0, 3), np.float32), grad=False)
    assert float(e0.abs().max()) == 0.0
    (_, _, _, _, e1), _, _, _ = _render(kw, extra, grad=False)
    (_, _, d2, a2, e2), _, _, t = _render(kw, extra, debug=True)
    assert _bits(e1, e2)
    (e2.sum() + d2.sum()).backward()
    assert float(t.grad.abs().max()) > 0


if __name__ == "__main__":          # child process of test_both_forward_kernels_render_the_same_extra_map
    _child_maps(sys.argv[1], sys.argv[2])
