"""The median depth map (GaussianRasterizer(..., depth_alpha=True, median_depth=True)) on the GPU.

Reference: tests/median_ref.py on the float64 oracle (tests/test_median_ref.py anchors it): per pixel the median splat's index, its
depth and gap = min |T_i - 0.5| over the composited splats.  The map is held to |median - reference| <= 1e-5 max|z| - the depth map's
bound - on the pixels that are strict (test_gpu_parity._strict_pixels) and have gap >= 1e-4, ten times the bound the project holds
alpha to: nearer than that binary32 may legitimately choose the neighbouring splat.  The pixels left out for gap are at most 1 % of
every frame (0.05 .. 0.58 %; the CPU test asserts it on the same frames).  Gradients: the selection is piecewise constant, so the
reference is test_gpu_depth_alpha._want plus sum over pixels of g_m [index == g] V[:3, 2] on means3D, every Gaussian under
test_gpu_parity._check_grads' 1e-4 rule.  The oracle frames of a scene are computed once and shared.  Every test prints what it judged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import median_ref as MR
import oracle
import scene_synth as S
import streams as ST
from test_gpu_depth_alpha import G1_CASES, _aux_oracle, _uncovered_half_kwargs, _upstream, _want
from test_gpu_parity import DEV, _check_grads, _fixture_kwargs, _inputs, _settings, _strict_pixels

pytestmark = pytest.mark.gpu

GAP = 1e-4
CASES = G1_CASES + ["uncovered half"]
_id = lambda c: c if isinstance(c, str) else f"P{c['P']}_{c['W']}x{c['H']}_s{c['seed']}" + (f"_pose{c['pose']}" if "pose" in c else "")
MID = dict(P=2048, W=128, H=128, D=3, seed=105)
POSED = dict(P=2048, W=128, H=128, D=3, seed=105, pose="a")
BIG = dict(P=5000, W=256, H=192, D=3, seed=109)
_KW, _REF = {}, {}


def _kwargs(c):
    key = _id(c)
    if key not in _KW:
        _KW[key] = _uncovered_half_kwargs() if isinstance(c, str) else _fixture_kwargs(c)
    return _KW[key]


def _reference(c):
    """(SH frame, (z, 1, 0) frame, z, median_ref.median_depth of the SH frame) of the float64 oracle, once per scene; never modified."""
    key = _id(c)
    if key not in _REF:
        kw, par = _kwargs(c), isinstance(c, str)
        fr_sh = oracle.rasterize(dtype=np.float64, parallel=par, **kw)
        fr_aux, z = _aux_oracle(kw, parallel=par)
        _REF[key] = (fr_sh, fr_aux, z, MR.median_depth(fr_sh))
    return _REF[key]


def _render(kw, median=True, grad=True, debug=False, **more):
    """-> ((color, radii, depth, alpha[, median]), geometry leaves, means2D)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, grad)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=grad)
    return GaussianRasterizer(_settings(kw, debug), depth_alpha=True, median_depth=median, **more)(means2D=means2D, **inp), inp, means2D


def _host(t):
    return t.detach().cpu().numpy()


def _judged(c, radii):
    """The pixels of test 1: strict and at least GAP away from a flip of the selection; the share left out for gap is asserted."""
    fr_sh, fr_aux, z, ref = _reference(c)
    strict = _strict_pixels(fr_sh, radii) & (fr_aux.fragile_px == 0)
    near = ref["gap"] < GAP
    print(f"{_id(c)}: {int(near.sum())} of {near.size} pixels ({100.0 * near.mean():.2f} %) left out for gap < {GAP}; "
          f"{int((strict & ~near).sum())} judged")
    assert near.mean() <= 0.01
    return strict & ~near


def _check_map(c, median, mask):
    fr_sh, fr_aux, z, ref = _reference(c)
    got = _host(median)[0]
    err = np.abs(got - ref["median"])
    zmax = float(np.abs(z).max())
    print(f"{_id(c)}: median max error {err[mask].max():.3e} on {int(mask.sum())} pixels, bound {1e-5 * zmax:.3e}")
    assert err[mask].max() <= 1e-5 * zmax
    none = (ref["index"] < 0) & mask                    # pixels nothing composited: exactly +0.0
    assert (got[none].view(np.int32) == 0).all()
    return int(none.sum())


# ---- 1. maps -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_maps_against_the_reference_and_bits_of_the_other_outputs(c):
    import diff_gaussian_rasterization as dgr
    kw = _kwargs(c)
    with torch.no_grad():
        (c0, r0, d0, a0), _, _ = _render(kw, median=False, grad=False)
        (c1, r1, d1, a1, m1), inp, _ = _render(kw, grad=False)
    for name, x, y in (("color", c0, c1), ("radii", r0, r1), ("depth", d0, d1), ("alpha", a0, a1)):
        assert ST.same_bits(x.cpu(), y.cpu()), name
    assert m1.shape == d1.shape and m1.dtype == torch.float32
    mask = _judged(c, _host(r1))
    _check_map(c, m1, mask)
    if isinstance(c, str):      # the carry between chunks and the filtered chunks: the median frame itself ran them
        _, _, fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None,
                                         _settings(kw), aux=True, median=True)
        torch.cuda.synchronize()
        assert fr.plan.chunks_run > 1 and fr.plan.chunks_filtered != 0, (fr.plan.chunks_run, fr.plan.chunks_filtered)
        assert ST.same_bits(fr.median.cpu(), m1.cpu()) and ST.same_bits(fr.depth.cpu(), d1.cpu())
        enc = fr.median_enc.cpu().numpy()
        chunk = (enc >> 26) - 1
        print(f"{c}: medians by chunk {np.bincount(chunk[chunk >= 0].ravel()).tolist()}")
        assert (chunk[_reference(c)[3]["index"] >= 0] >= 0).all() and len(np.unique(chunk[chunk >= 0])) > 1


# ---- 2. gradients --------------------------------------------------------------------------------------------------------------------
def _median_term(c, gm):
    """G [P] = sum over the pixels whose median splat is g of g_m, and its chain to means3D."""
    kw = _kwargs(c)
    ref = _reference(c)[3]
    P = np.asarray(kw["means3D"]).shape[0]
    G = np.zeros(P)
    has = ref["index"] >= 0
    np.add.at(G, ref["index"][has], gm[has])
    return G, G[:, None] * np.asarray(kw["viewmatrix"], np.float64)[:3, 2][None]


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_gradients_against_the_oracle(c):
    kw, multi = _kwargs(c), isinstance(c, str)
    fr_sh, fr_aux, z, ref = _reference(c)
    H, W = kw["image_height"], kw["image_width"]
    (color, radii, depth, alpha, median), inp, means2D = _render(kw)
    mask = _judged(c, _host(radii))
    _check_map(c, median, mask)
    seed = 17 if multi else c["seed"]
    zmax = float(np.abs(z).max())
    gc, gz, ga = _upstream(H, W, seed, zmax)
    gm = (torch.rand(H, W, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64).numpy() - 0.5) / zmax
    gc, gz, ga, gm = gc * mask[None], gz * mask, ga * mask, gm * mask
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    torch.autograd.backward([color, depth, alpha, median], [t(gc), t(gz)[None], t(ga)[None], t(gm)[None]])
    got = {k: _host(v.grad) for k, v in inp.items()}
    got["means2D"] = _host(means2D.grad)
    want = _want(fr_sh, fr_aux, kw, gc, gz, ga, parallel=multi)
    G, chain = _median_term(c, gm)
    want["means3D"] = want["means3D"] + chain
    print(f"{_id(c)}: the median term reaches {int((G != 0).sum())} Gaussians, max |chain| {np.abs(chain).max():.3e} "
          f"of max |dL/dmeans3D| {np.abs(want['means3D']).max():.3e}")
    assert (G != 0).sum() > (100 if multi else 10)
    live, strict_live = _check_grads(fr_sh, want, got, ["means3D", "means2D", "opacities", "shs", "scales", "rotations"], masked=True)
    assert live > (1000 if multi else 0) and strict_live == live


def test_a_median_only_upstream_gradient_reaches_means3d_and_nothing_else():
    kw = _kwargs(MID)
    fr_sh, fr_aux, z, ref = _reference(MID)
    (color, radii, depth, alpha, median), inp, means2D = _render(kw)
    mask = _judged(MID, _host(radii))
    gm = (torch.rand(128, 128, generator=torch.Generator().manual_seed(4), dtype=torch.float64).numpy() - 0.5) * mask
    median.backward(torch.as_tensor(gm, dtype=torch.float32, device=DEV)[None])
    for n in ("opacities", "scales", "rotations", "shs"):
        assert inp[n].grad is not None and not bool(inp[n].grad.any()), n          # exactly zero
    assert not bool(means2D.grad.any())
    G, chain = _median_term(MID, gm)
    got = {"means3D": _host(inp["means3D"].grad)}
    err = np.abs(got["means3D"] - chain).max()
    print(f"median-only: max error {err:.3e} of max |want| {np.abs(chain).max():.3e}, {int((G != 0).sum())} Gaussians")
    live, strict_live = _check_grads(fr_sh, {"means3D": chain}, got, ["means3D"], masked=True)
    assert live > 100 and strict_live == live


def test_a_median_only_upstream_gradient_reaches_the_view_matrix():
    """dL/dviewmatrix[:, 2] = sum_g G_g (x_g, 1), under both bounds of tests/test_gpu_camera_grad.py (camera_ref.check_camera_grads):
    e <= 1e-4 A with A = sum |terms|, and e <= F max(yard32, 1e-7 A) with yard32 the same sum formed in binary32 (both orders)."""
    import camera_ref as CR
    from diff_gaussian_rasterization import GaussianRasterizer
    kw = _kwargs(POSED)
    fr_sh, fr_aux, z, ref = _reference(POSED)
    rs = _settings(kw)
    V = rs.viewmatrix.detach().clone().requires_grad_(True)
    inp = _inputs(kw, True)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    out = GaussianRasterizer(rs._replace(viewmatrix=V), depth_alpha=True, median_depth=True)(means2D=means2D, **inp)
    with torch.no_grad():
        plain = _render(kw, grad=False)[0]
    assert all(ST.same_bits(a.detach().cpu(), b.cpu()) for a, b in zip(out, plain))
    mask = _judged(POSED, _host(out[1]))
    gm = (torch.rand(128, 128, generator=torch.Generator().manual_seed(6), dtype=torch.float64).numpy() - 0.5) * mask
    out[4].backward(torch.as_tensor(gm, dtype=torch.float32, device=DEV)[None])
    G, chain = _median_term(POSED, gm)
    x = np.concatenate([np.asarray(kw["means3D"], np.float64), np.ones((G.shape[0], 1))], 1)           # (x_g, 1)
    terms = G[:, None] * x
    want, A = np.zeros((4, 4)), np.zeros((4, 4))
    want[:, 2], A[:, 2] = terms.sum(0), np.abs(terms).sum(0)
    # the binary32 yardstick: G accumulated and the sum formed in binary32, in ascending and in descending order
    has = ref["index"] >= 0
    G32 = np.zeros(G.shape[0], np.float32)
    np.add.at(G32, ref["index"][has], gm[has].astype(np.float32))
    t32 = G32[:, None] * x.astype(np.float32)
    yard = np.zeros((4, 4))
    yard[:, 2] = np.maximum(np.abs(np.cumsum(t32, 0, dtype=np.float32)[-1] - want[:, 2]),
                            np.abs(np.cumsum(t32[::-1], 0, dtype=np.float32)[-1] - want[:, 2]))
    got = {"viewmatrix": _host(V.grad)}
    CR.check_camera_grads(got, {"viewmatrix": want}, {"viewmatrix": A}, {"viewmatrix": yard}, label="median-only", needs=(True, False, False))
    assert np.abs(got["viewmatrix"][:, 2]).max() > 0
    err = np.abs(_host(inp["means3D"].grad) - chain).max()
    assert err <= 1e-4 * np.abs(chain).max()


# ---- 3. the closed-form two-splat scene ------------------------------------------------------------------------------------------------
def _two_splat_model(front):
    from scene import GaussianModel
    scene, cam = MR.two_splat_scene(front)
    gm = GaussianModel(0)
    gm.adopt_scene(scene, device=DEV)
    return gm, cam.to(DEV)


@pytest.mark.parametrize("front,want", [(0.4, 3.0), (0.6, 1.0)])
def test_two_splats_through_the_rasterizer_render_normals_and_the_fusion(front, want):
    import tsdf_ref as TR
    from diff_gaussian_rasterization.normals import depth_to_normal, surface_depth
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_normals
    from scene import mesh
    kw = MR.two_splat_kwargs(front)
    ref = MR.median_depth(oracle.rasterize(dtype=np.float64, **kw))
    with torch.no_grad():
        (color, radii, depth, alpha, median), _, _ = _render(kw, grad=False)
    m, c = _host(median)[0], 16
    mean = float(depth[0, c, c] / alpha[0, c, c])
    print(f"front opacity {front}: centre pixel median {m[c, c]}, mean {mean:.6f}")
    assert m[c, c] == want and 1.0 < mean < 3.0
    assert abs(mean - (front + (1 - front) * 0.9 * 3) / (front + (1 - front) * 0.9)) <= 1e-5 * 3
    none = ref["index"] < 0
    assert none.any() and (m[none].view(np.int32) == 0).all()                    # nothing composited: exactly +0.0
    ok = ref["gap"] >= GAP
    assert np.abs(m - ref["median"])[ok].max() <= 1e-5 * 3 and ok.mean() >= 0.99
    # render_normals(depth_ratio=1): the depth normals of the median surface
    gm, cam = _two_splat_model(front)
    pipe = Pipe()
    with torch.no_grad():
        one = render_normals(cam, gm, pipe, depth_ratio=1.0)
        zero = render_normals(cam, gm, pipe)
        pkg = render(cam, gm, pipe, torch.zeros(3, device=DEV), depth_alpha=True, median_depth=True)
    assert "median_depth" not in zero and "surf_depth" not in zero and set(one) == set(zero) | {"median_depth", "surf_depth"}
    for k in ("normal", "depth", "alpha"):
        assert ST.same_bits(one[k].cpu(), zero[k].cpu()), k
    assert ST.same_bits(one["surf_depth"].cpu(), (one["alpha"] * one["median_depth"]).cpu())
    assert ST.same_bits(one["depth_normal"].cpu(), depth_to_normal(one["surf_depth"], one["alpha"], 1.0, 1.0).cpu())
    assert float(one["median_depth"][0, c, c]) == want and float((one["surf_depth"] / one["alpha"].clamp_min(1e-6))[0, c, c] - want) <= 1e-5 * 3
    # fuse_depth_maps(depth_ratio=1) into a 16^3 volume: the kernel and the torch twin against the binary64 restatement of the same frame
    # (a grid in general position: with round numbers the voxel centres project onto pixel edges and every update is fragile)
    grid = TR.Grid((16, 16, 16), (-1.431, -1.373, 0.637), 0.1913, 0.5771)
    vol = TSDFVolume(grid.origin, float(grid.voxel), grid.dims, float(grid.trunc), device=DEV)
    mesh.fuse_depth_maps(gm, [cam], pipe, torch.zeros(3, device=DEV), vol, depth_ratio=1.0)
    surf = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], 1.0)
    frame = TR.Frame(_host(cam.world_view_transform), _host(surf)[0], _host(pkg["alpha"])[0], _host(pkg["render"]), 1.0, 1.0)
    tracked = TR.fuse_tracked(grid, [frame])
    TR.assert_cap(tracked, f"two splats, front {front}")
    arrays = lambda v: (_host(v.tsdf).reshape(-1), _host(v.weight).reshape(-1), _host(v.color).reshape(3, -1))
    assert TR.check_volume(*arrays(vol), tracked, f"kernel, front {front}") <= 1
    twin = TSDFVolume(grid.origin, float(grid.voxel), grid.dims, float(grid.trunc), device=DEV)
    twin.integrate(surf.contiguous(), pkg["alpha"].contiguous(), pkg["render"].contiguous(), cam.world_view_transform.contiguous(), 1.0, 1.0,
                   native=False)
    assert TR.check_volume(*arrays(twin), tracked, f"twin, front {front}") <= 1
    robust = ~tracked["fragile"].numpy()
    assert np.array_equal(arrays(vol)[1][robust], arrays(twin)[1][robust]) and arrays(vol)[1].sum() > 0         # the same integers
    with pytest.raises(ValueError, match="depth_ratio"):
        mesh.fuse_depth_maps(gm, [cam], pipe, torch.zeros(3, device=DEV), vol, depth_ratio=1.5)


# ---- 4. kernels and determinism ----------------------------------------------------------------------------------------------------------
def _child_maps(out):
    with torch.no_grad():
        (_, _, depth, alpha, median), _, _ = _render(_kwargs(BIG), grad=False)
    np.save(out, np.stack([_host(median)[0], _host(depth)[0], _host(alpha)[0]]))


def test_both_forward_kernels_render_the_same_median(tmp_path):
    outs = []
    for forced in ("0", "1"):                        # (GSR_FWD_GROUPS is read when the library loads: a child process each)
        out = str(tmp_path / f"maps{forced}.npy")
        env = dict(os.environ, GSR_FWD_GROUPS=forced, PYTHONPATH=os.pathsep.join(sys.path))
        subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
        outs.append(np.load(out))
    assert outs[0][2].max() > 0.5 and outs[0][0].max() > 0.2
    assert np.array_equal(outs[0].view(np.int32), outs[1].view(np.int32))


def test_the_same_frame_gives_the_same_bits():
    kw = _kwargs(BIG)
    runs = []
    for _ in range(2):
        (color, radii, depth, alpha, median), inp, means2D = _render(kw)
        g = torch.Generator().manual_seed(3)
        ups = [torch.rand(o.shape, generator=g).to(DEV) - 0.5 for o in (color, depth, alpha, median)]
        torch.autograd.backward([color, depth, alpha, median], ups, retain_graph=True)
        leaves = {**inp, "means2D": means2D}
        first = {k: v.grad.clone() for k, v in leaves.items()}
        for v in leaves.values():
            v.grad = None
        torch.autograd.backward([color, depth, alpha, median], ups)          # a second backward of the same frame
        for k, v in leaves.items():
            assert ST.same_bits(first[k], v.grad), k
        runs.append({**{k: v.cpu() for k, v in first.items()},
                     **{n: o.detach().cpu() for n, o in zip(("color", "radii", "depth", "alpha", "median"), (color, radii, depth, alpha, median))}})
    for k in runs[0]:
        assert ST.same_bits(runs[0][k], runs[1][k]), k
    # without an upstream gradient on the median the backward is the aux frame's, bit for bit
    (c1, r1, d1, a1, m1), inp1, m2d1 = _render(kw)
    (c0, r0, d0, a0), inp0, m2d0 = _render(kw, median=False)
    torch.autograd.backward([c1, d1, a1], ups[:3])
    torch.autograd.backward([c0, d0, a0], ups[:3])
    for k in inp0:
        assert ST.same_bits(inp0[k].grad, inp1[k].grad), k
    assert ST.same_bits(m2d0.grad, m2d1.grad)


def test_forward_forward_raw_fused_getters_and_the_switches_agree():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    kw = _kwargs(MID)
    fr_sh, fr_aux, z, ref = _reference(MID)
    zmax = float(np.abs(z).max())
    rs = _settings(kw)
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    m2 = torch.zeros(P, 3, device=DEV)
    bits = lambda a, b: ST.same_bits(a.detach().cpu(), b.detach().cpu())
    with torch.no_grad():
        # antialiasing and debug: the other outputs keep their bits; the median is a splat's depth under the compensated opacity
        for more in (dict(antialiasing=True), {}):
            for debug in (False, True):
                rsd = _settings(kw, debug)
                o0 = GaussianRasterizer(rsd, depth_alpha=True, **more)(means2D=m2, **inp)
                o1 = GaussianRasterizer(rsd, depth_alpha=True, median_depth=True, **more)(means2D=m2, **inp)
                assert len(o1) == 5 and all(bits(a, b) for a, b in zip(o0, o1[:4])), (more, debug)
                assert bool(((o1[4] > 0) == (o1[3] > 0)).all())
        plain = GaussianRasterizer(rs, depth_alpha=True, median_depth=True)(means2D=m2, **inp)
    # FUSE_GETTERS and forward_raw: the getters' outputs over leaves are rendered from the leaves
    leaf = lambda v: v.detach().clone().to(DEV).requires_grad_(True)
    xyz, dc, rest = leaf(inp["means3D"]), leaf(inp["shs"][:, :1]), leaf(inp["shs"][:, 1:])
    op, sc, rot = leaf(torch.logit(inp["opacities"].clamp(1e-4, 1 - 1e-4))), leaf(inp["scales"].log()), leaf(inp["rotations"] * 1.5)

    def getters(rast):
        return rast(means3D=xyz, means2D=torch.zeros(P, 3, device=DEV, requires_grad=True), opacities=torch.sigmoid(op),
                    shs=torch.cat((dc, rest), 1), scales=torch.exp(sc), rotations=torch.nn.functional.normalize(rot))
    was = dgr.FUSE_GETTERS
    dgr.FUSE_GETTERS = True
    try:
        f0 = getters(GaussianRasterizer(rs, depth_alpha=True))
        f1 = getters(GaussianRasterizer(rs, depth_alpha=True, median_depth=True))
        assert type(f1[0].grad_fn).__name__.startswith("_RasterizeGaussiansRaw")
    finally:
        dgr.FUSE_GETTERS = was
    with torch.no_grad():
        raw = GaussianRasterizer(rs, depth_alpha=True, median_depth=True).forward_raw(xyz, m2, dc, rest, op, sc, rot)
    assert len(f1) == 5 and len(raw) == 5 and all(bits(a, b) for a, b in zip(f0, f1[:4])) and all(bits(a, b) for a, b in zip(f1, raw))
    mask = _judged(MID, _host(plain[1]))
    for name, out in (("forward", plain), ("forward_raw", raw)):
        err = np.abs(_host(out[4])[0] - ref["median"])[mask].max()
        print(f"{name}: median max error {err:.3e}, bound {1e-5 * zmax:.3e}")
        assert err <= 1e-5 * zmax
    f1[4].sum().backward()
    assert float(xyz.grad.abs().max()) > 0 and not bool(op.grad.any()) and not bool(rot.grad.any()) and not bool(sc.grad.any())
    # render(): the dict, on the raw path and on the getter path; a model with a 3D filter
    scene, cam = S.make_scene(MID["P"], 128, 128, 3, MID["seed"], scale_lo=0.005, scale_hi=0.06), S.make_camera(128, 128).to(DEV)
    gm = GaussianModel(3)
    gm.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    for filtered in (False, True):
        if filtered:
            gm.compute_3D_filter([cam])
            assert gm.filter_3D is not None
        for fused in (None, False):
            pipe = Pipe()
            pipe.fused_activations = fused
            with torch.no_grad():
                a = render(cam, gm, pipe, bg, depth_alpha=True)
                b = render(cam, gm, pipe, bg, depth_alpha=True, median_depth=True)
            assert "median_depth" not in a and set(b) == set(a) | {"median_depth"}
            for k in ("render", "radii", "depth", "alpha"):
                assert bits(a[k], b[k]), (filtered, fused, k)
            md = b["median_depth"]
            assert md.shape == b["depth"].shape and bool(((md > 0) == (b["alpha"] > 0)).all())
    out = render(cam, gm, Pipe(), bg, depth_alpha=True, median_depth=True)
    out["median_depth"].sum().backward()
    assert float(gm._xyz.grad.abs().max()) > 0 and not bool(gm._opacity.grad.any())


# ---- 6. train() ----------------------------------------------------------------------------------------------------------------------
def _train(iterations=8, **opt_kw):
    import random
    from dataclasses import replace

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
    return gm, losses, {k: v[1] for k, v in scopes.items()}


def test_training_reads_depth_ratio_for_the_normal_term():
    kw = dict(lambda_normal=0.05, normal_from_iter=3)
    mean, loss_0, scopes_0 = _train(**kw)
    again, loss_00, scopes_00 = _train(depth_ratio=0.0, **kw)
    med, loss_1, scopes_1 = _train(depth_ratio=1.0, **kw)
    # the default is the loop as it was: no median launch, the same launches and bits
    assert "render_fwd_median" not in scopes_0 and scopes_00 == scopes_0 and loss_00 == loss_0 and torch.equal(again._xyz, mean._xyz)
    # iterations 3 .. 8: the normals frame is a median frame, and its backward carries the median's gradient
    assert scopes_1.get("render_fwd_median", 0) >= 6 and scopes_1.get("render_bwd_median", 0) == 6
    assert loss_1[:2] == loss_0[:2] and all(np.isfinite(loss_1)) and bool(torch.isfinite(med._xyz).all())
    assert not torch.equal(med._xyz, mean._xyz)
    print(f"final image loss: depth_ratio 0 {loss_0[-1]:.6f}, depth_ratio 1 {loss_1[-1]:.6f}")


if __name__ == "__main__":          # child process of test_both_forward_kernels_render_the_same_median
    _child_maps(sys.argv[1])
