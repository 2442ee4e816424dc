"""The depth and alpha maps (GaussianRasterizer(..., depth_alpha=True)) on the GPU.

Reference (tests/test_depth_alpha_abi.py pins it against torch autograd): the fp64 oracle on the same geometry with
colors_precomp = (z, 1, 0) and bg = 0 - channel 0 is depth, channel 1 is sum w = 1 - T_final - and the gradient of
L = <g_c, C> + <g_z, depth> + <g_a, alpha> is the SH frame's gradient for g_c, plus the aux frame's for (g_z, g_a, 0), plus that
frame's colors_precomp[:, 0] gradient (= dL/dz) chained to means3D."""
import os
import sys

import numpy as np
import pytest
import torch

import oracle
import scene_synth as S
from test_gpu_parity import DEV, _check_grads, _fixture_kwargs, _inputs, _settings, _strict_pixels

pytestmark = pytest.mark.gpu


def _aux_oracle(kw, parallel=False):
    V = np.asarray(kw["viewmatrix"], np.float64)
    z = np.asarray(kw["means3D"], np.float64) @ V[:3, 2] + V[3, 2]
    akw = {k: v for k, v in kw.items() if k != "shs"}
    akw.update(colors_precomp=np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), bg=np.zeros(3))
    return oracle.rasterize(dtype=np.float64, parallel=parallel, **akw), z


def _render(kw, depth_alpha=True, debug=False, grad=True):
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, grad)
    P = inp["means3D"].shape[0]
    means2D = torch.zeros(P, 3, device=DEV, requires_grad=grad)
    out = GaussianRasterizer(_settings(kw, debug), depth_alpha=depth_alpha)(means2D=means2D, **inp)
    return out, inp, means2D


def _upstream(H, W, seed, zmax):
    g = torch.Generator().manual_seed(seed)
    gc = S.make_grad_image(W, H, seed).numpy().astype(np.float64)
    gz = (torch.rand(H, W, generator=g, dtype=torch.float64).numpy() - 0.5) / zmax
    ga = torch.rand(H, W, generator=g, dtype=torch.float64).numpy() - 0.5
    return gc, gz, ga


def _want(fr_sh, fr_aux, kw, gc, gz, ga, parallel=False):
    want = fr_sh.backward(gc, parallel=parallel)
    waux = fr_aux.backward(np.stack([gz, ga, np.zeros_like(gz)]), parallel=parallel)
    out = {}
    for n in ("means3D", "means2D", "opacities", "scales", "rotations"):
        out[n] = want[n] + waux[n]
    out["means3D"] = out["means3D"] + waux["colors_precomp"][:, :1] * np.asarray(kw["viewmatrix"], np.float64)[:3, 2][None]
    out["shs"] = want["shs"]
    return out


def _check_maps(fr_aux, z, strict, depth, alpha):
    zmax = float(np.abs(z).max())
    d, a = depth.detach().cpu().numpy()[0], alpha.detach().cpu().numpy()[0]
    assert np.abs(d - fr_aux.color[0])[strict].max() <= 1e-5 * zmax
    assert np.abs(a - fr_aux.color[1])[strict].max() <= 1e-5


G1_CASES = [dict(P=64, W=48, H=80, D=2, seed=103), dict(P=2048, W=128, H=128, D=3, seed=105),
            dict(P=2048, W=128, H=128, D=3, seed=111), dict(P=5000, W=256, H=192, D=3, seed=109),
            dict(P=2048, W=128, H=128, D=3, seed=105, pose="a")]        # a posed camera (tests/posed.py): the z chain's view[6]


def _uncovered_half_kwargs():
    """test_gpu_parity's frame with an uncovered region: no splat covers the lower half, those tiles never close, every planned
    chunk runs and the late ones go through the live filter."""
    from util import raster_kwargs
    scene = S.make_scene(260_000, 480, 320, 1, 91, scale_lo=0.01, scale_hi=0.07)
    scene.means3D[:, 1] = -scene.means3D[:, 1].abs() - 0.02 * scene.means3D[:, 2]
    return raster_kwargs(scene, S.make_camera(480, 320))


def _uncovered_half_posed_kwargs():
    """The same frame in front of a posed camera (tests/posed.py to_world): the chunked colour kernel, the sparse geometry backward and
    k_geom_bwd_depth<true> with every view-matrix entry non-zero."""
    from test_gpu_parity import _uncovered_half_posed
    from util import raster_kwargs
    return raster_kwargs(*_uncovered_half_posed())


def _planned_chunks(fr):
    """The chunk count gsr_forward_preprocess planned for the frame (before gsr_forward_render merged any), on fresh workspaces."""
    from diff_gaussian_rasterization import _native as N
    geom_bytes, _ = N.workspace_sizes(fr.desc)
    geom = torch.empty(geom_bytes, dtype=torch.uint8, device=DEV)
    radii = torch.empty(fr.desc.P, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        plan = N.forward_preprocess(fr.desc, fr.cam, fr.gauss, geom, radii, torch.device(DEV))
    torch.cuda.synchronize()
    return int(plan.num_chunks)


def _assert_multi_chunk(kw, merged=False):
    """The aux frame of kw runs more than one depth chunk and live-filters one (merged: it also merged planned chunks)."""
    import diff_gaussian_rasterization as dgr
    inp = _inputs(kw, False)
    _, _, fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None,
                                     _settings(kw), aux=True)
    torch.cuda.synchronize()
    plan = fr.plan
    assert plan.chunks_run > 1 and plan.chunks_filtered != 0, (plan.chunks_run, plan.chunks_filtered)
    if merged:
        assert _planned_chunks(fr) > plan.num_chunks, (plan.num_chunks, plan.chunks_run)
    return fr


@pytest.mark.parametrize("c", G1_CASES + ["uncovered half", "uncovered half posed"],
                         ids=lambda c: c if isinstance(c, str) else f"P{c['P']}_{c['W']}x{c['H']}_s{c['seed']}" + (f"_pose{c['pose']}" if "pose" in c else ""))
def test_g1_maps_and_gradients_against_the_oracle(c):
    multi = isinstance(c, str)
    kw = (_uncovered_half_posed_kwargs() if c == "uncovered half posed" else _uncovered_half_kwargs()) if multi else _fixture_kwargs(c)
    if multi:                     # the chunk-start aux checkpoints, the depth map carried between chunks, the filtered chunks
        _assert_multi_chunk(kw)
    H, W = kw["image_height"], kw["image_width"]
    fr_sh = oracle.rasterize(dtype=np.float64, parallel=multi, **kw)
    fr_aux, z = _aux_oracle(kw, parallel=multi)
    (color, radii, depth, alpha), inp, means2D = _render(kw)
    # the posed 260 k frame holds one Gaussian with 3 sqrt(lambda) = 104.00001 (1e-7 relative above the integer): binary32 may round
    # its radius to 104; _strict_pixels leaves out the tiles only one of the two rectangles covers
    strict = _strict_pixels(fr_sh, radii.cpu().numpy(), exact_radii=c != "uncovered half posed") & (fr_aux.fragile_px == 0)
    _check_maps(fr_aux, z, strict, depth, alpha)
    gc, gz, ga = _upstream(H, W, 17 if multi else c["seed"], float(np.abs(z).max()))
    gc, gz, ga = gc * strict[None], gz * strict, ga * strict
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    torch.autograd.backward([color, depth, alpha], [t(gc), t(gz)[None], t(ga)[None]])
    got = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    got["means2D"] = means2D.grad.detach().cpu().numpy()
    want = _want(fr_sh, fr_aux, kw, gc, gz, ga, parallel=multi)
    live, strict_live = _check_grads(fr_sh, want, got, ["means3D", "means2D", "opacities", "shs", "scales", "rotations"], masked=True)
    assert live > (1000 if multi else 0) and strict_live == live


@pytest.mark.parametrize("which", ["alpha", "depth", "depth+alpha"])
def test_g1_losses_without_a_colour_gradient(which):
    """Only the maps carry a loss (the colour's upstream gradient is None): alpha alone runs the aux kernel with neither a colour nor
    a depth gradient, depth alone with neither a colour nor an alpha gradient.  Every input against the oracle."""
    c = dict(P=2048, W=128, H=128, D=3, seed=105)
    kw = _fixture_kwargs(c)
    fr_sh = oracle.rasterize(dtype=np.float64, **kw)
    fr_aux, z = _aux_oracle(kw)
    (color, radii, depth, alpha), inp, means2D = _render(kw)
    strict = _strict_pixels(fr_sh, radii.cpu().numpy()) & (fr_aux.fragile_px == 0)
    _, gz, ga = _upstream(c["H"], c["W"], c["seed"], float(np.abs(z).max()))
    gz = gz * strict if "depth" in which else np.zeros_like(gz)
    ga = ga * strict if "alpha" in which else np.zeros_like(ga)
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    outs = ([depth] if "depth" in which else []) + ([alpha] if "alpha" in which else [])
    grads = ([t(gz)[None]] if "depth" in which else []) + ([t(ga)[None]] if "alpha" in which else [])
    torch.autograd.backward(outs, grads)
    got = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    got["means2D"] = means2D.grad.detach().cpu().numpy()
    want = _want(fr_sh, fr_aux, kw, np.zeros((3, c["H"], c["W"])), gz, ga)
    assert not want["shs"].any() and not got["shs"].any()         # no colour gradient: none reaches the SH coefficients
    live, strict_live = _check_grads(fr_sh, want, got, ["means3D", "means2D", "opacities", "scales", "rotations"], masked=True)
    assert live > 0 and strict_live == live


def test_g1_raw_path_through_render():
    """render(..., depth_alpha=True) with scene.GaussianModel (the raw-parameter route, activations in the kernels): maps on
    strict pixels and the gradient on the position leaf against the oracle."""
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    from util import raster_kwargs
    P, W, H, D, seed = 2048, 128, 128, 3, 105
    scene, cam = S.make_scene(P, W, H, D, seed, scale_lo=0.005, scale_hi=0.06), S.make_camera(W, H)
    kw = raster_kwargs(scene, cam)
    fr_sh = oracle.rasterize(dtype=np.float64, **kw)
    fr_aux, z = _aux_oracle(kw)
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    out = render(cam.to(DEV), gm, Pipe(), torch.zeros(3, device=DEV), depth_alpha=True)
    assert set(out) >= {"render", "radii", "depth", "alpha", "viewspace_points", "visibility_filter"}
    strict = (fr_sh.fragile_px == 0) & (fr_aux.fragile_px == 0)
    _check_maps(fr_aux, z, strict, out["depth"], out["alpha"])
    gc, gz, ga = _upstream(H, W, seed, float(np.abs(z).max()))
    gc, gz, ga = gc * strict[None], gz * strict, ga * strict
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV)
    torch.autograd.backward([out["render"], out["depth"], out["alpha"]], [t(gc), t(gz)[None], t(ga)[None]])
    want = _want(fr_sh, fr_aux, kw, gc, gz, ga)
    # the activations' chain rule (scene/gaussian_model.py getters) in binary64, on the raw values the model holds
    logit = scene.opacity_logits.double().numpy()
    sig = 1.0 / (1.0 + np.exp(-logit))
    r = scene.raw_rotations.double().numpy()
    rn = np.linalg.norm(r, axis=1, keepdims=True)
    q = r / rn
    g_rot = want["rotations"].reshape(q.shape)
    want_raw = {"means3D": want["means3D"], "means2D": want["means2D"], "shs": want["shs"],
                "opacities": want["opacities"].reshape(sig.shape) * sig * (1.0 - sig),
                "scales": want["scales"] * np.exp(scene.log_scales.double().numpy()),
                "rotations": (g_rot - q * (q * g_rot).sum(1, keepdims=True)) / rn}
    got = {"means3D": gm._xyz.grad, "means2D": out["viewspace_points"].grad, "shs": gm._features.grad,
           "opacities": gm._opacity.grad, "scales": gm._scaling.grad, "rotations": gm._rotation.grad}
    got = {k: v.detach().cpu().numpy() for k, v in got.items()}
    live, strict_live = _check_grads(fr_sh, want_raw, got, list(got), masked=True)
    assert live > 0 and strict_live == live


@pytest.mark.parametrize("frame", ["cfg3n", "cfg3 arc camera 0"])
def test_g2_full_size_bits(frame):
    """Full size: depth is bit for bit channel 0 of the frame rendered with colors_precomp = the record depths and bg = 0; alpha is
    bit for bit 1 - |final_T|; screen_grads slot 9 is that render's dL/dcolors_precomp[:, 0] for dL/dcolor = (g_z, 0, 0).
    cfg3n: one chunk, ~400 composited splats per pixel.  The training loop's arc frame (test_gpu_timed_path): a corner no splat
    covers, so every chunk runs - merged and live-filtered."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    from util import raster_kwargs
    if frame == "cfg3n":
        scene, cam = S.make_config("cfg3n")
    else:
        c = S.CONFIGS["cfg3"]
        scene, cam = S.make_config("cfg3")[0], S.arc_cameras(c["W"], c["H"], 8)[0]
    kw = raster_kwargs(scene, cam)
    rs = _settings(kw)
    inp = _inputs(kw, False)
    args = (inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, rs)
    color, radii, fr = dgr.rasterize_forward(*args, aux=True)
    torch.cuda.synchronize()
    if frame != "cfg3n":
        assert fr.plan.chunks_run > 1 and fr.plan.chunks_filtered != 0, (fr.plan.chunks_run, fr.plan.chunks_filtered)
        assert _planned_chunks(fr) > fr.plan.num_chunks, fr.plan.num_chunks          # chunks were merged
    v = N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan)
    zrec = v["splat_records"][:, 9].clone()
    assert torch.equal(fr.alpha[0], 1 - v["final_T"].abs())
    zc = torch.stack([zrec, zrec, zrec], 1).contiguous()
    rs0 = rs._replace(bg=torch.zeros(3, device=DEV))
    c2, r2, fr2 = dgr.rasterize_forward(inp["means3D"], None, zc, inp["opacities"], inp["scales"], inp["rotations"], None, rs0)
    torch.cuda.synchronize()
    assert torch.equal(r2, radii)
    assert torch.equal(fr.depth[0], c2[0])
    H, W = color.shape[1:]
    g = torch.Generator().manual_seed(5)
    gz = ((torch.rand(H, W, generator=g) - 0.5) / float(zrec.max())).to(DEV)
    screen = dgr.rasterize_backward_screen(fr, None, grad_depth=gz[None])
    screen2 = dgr.rasterize_backward_screen(fr2, torch.stack([gz, torch.zeros_like(gz), torch.zeros_like(gz)]))
    needs = (False, False, False, True, False, False, False, False)
    gcol = dgr.rasterize_backward_geom(fr2, screen2, needs)[3]
    want, got = gcol[:, 0].double(), screen[:, 9].double()
    vis = radii > 0
    err = (got - want).abs()[vis]
    bound = 1e-4 * want.abs().max() + 1e-4 * want.abs()[vis]
    assert (err <= bound).all(), f"{int((err > bound).sum())} Gaussians off, max err {err.max():.3e}"
    assert int((want[vis] != 0).sum()) > 1000


def test_g3_option_on_against_option_off():
    kw = _fixture_kwargs(dict(P=5000, W=256, H=192, D=3, seed=109))
    gimg = S.make_grad_image(256, 192, 9).to(DEV)
    (c0, r0), inp0, m0 = _render(kw, depth_alpha=False)
    (c1, r1, d1, a1), inp1, m1 = _render(kw, depth_alpha=True)
    assert torch.equal(c0, c1) and torch.equal(r0, r1)
    c0.backward(gimg)
    c1.backward(gimg, retain_graph=True)
    for k in inp0:
        assert torch.equal(inp0[k].grad, inp1[k].grad), k
    assert torch.equal(m0.grad, m1.grad)
    # two backwards of one aux frame give the same bits
    (_, _, d, a), inp, m = _render(kw)
    gz = torch.rand_like(d) / float(d.detach().max())
    ga = torch.rand_like(a)
    torch.autograd.backward([d, a], [gz, ga], retain_graph=True)
    first = {k: v.grad.clone() for k, v in inp.items()}
    for v in inp.values():
        v.grad = None
    torch.autograd.backward([d, a], [gz, ga])
    for k, v in inp.items():
        assert torch.equal(first[k], v.grad), k


def _child_maps(out):
    kw = _fixture_kwargs(dict(P=5000, W=256, H=192, D=3, seed=109))
    (color, radii, depth, alpha), _, _ = _render(kw, grad=False)
    np.save(out, np.stack([depth.cpu().numpy()[0], alpha.cpu().numpy()[0]]))


def test_g4_both_forward_kernels_render_the_same_maps(tmp_path):
    import subprocess
    outs = []
    for forced in ("0", "1"):
        out = str(tmp_path / f"maps{forced}.npy")
        env = dict(os.environ, GSR_FWD_GROUPS=forced, PYTHONPATH=os.pathsep.join(sys.path))
        subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, timeout=300)
        outs.append(np.load(out))
    assert outs[0][1].max() > 0.5
    assert np.array_equal(outs[0], outs[1])


def test_g5_edge_cases():
    import diff_gaussian_rasterization as dgr
    kw = _fixture_kwargs(dict(P=64, W=48, H=80, D=2, seed=103))
    # an empty scene and the uncovered pixels: depth 0, alpha 0
    empty = {k: (v[:0] if k in ("means3D", "opacities", "shs", "scales", "rotations") else v) for k, v in kw.items()}
    (c, r, d, a), _, _ = _render(empty, grad=False)
    assert float(d.abs().max()) == 0.0 and float(a.abs().max()) == 0.0
    (c, r, d, a), _, _ = _render(_fixture_kwargs(dict(P=2, W=32, H=32, D=1, seed=102)), grad=False)
    assert bool(((a == 0) == (d == 0)).all()) and bool((a == 0).any()) and bool((a > 0).any())
    # alpha-only, depth-only, and no colour gradient
    for which in ("alpha", "depth"):
        (c, r, d, a), inp, m2 = _render(kw)
        (a if which == "alpha" else d).sum().backward()
        assert inp["opacities"].grad.abs().max() > 0, which
        if which == "depth":
            assert inp["means3D"].grad.abs().max() > 0
    # retain_graph, then a second backward
    (c, r, d, a), inp, m2 = _render(kw)
    (c.sum() + a.sum()).backward(retain_graph=True)
    g1 = inp["means3D"].grad.clone()
    (c.sum() + a.sum()).backward()
    assert torch.allclose(inp["means3D"].grad, 2 * g1)
    # no_grad
    with torch.no_grad():
        (c, r, d, a), _, _ = _render(kw)
    assert not d.requires_grad
    # debug=True
    (c2, r2, d2, a2), inp, _ = _render(kw, debug=True)
    assert torch.equal(d2, d) and torch.equal(a2, a)
    (d2.sum() + a2.sum()).backward()
    # aux with tile_rows
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None,
                              _settings(kw), tile_rows=(0, 2), aux=True)


if __name__ == "__main__":          # child process of test_g4 (GSR_FWD_GROUPS is read when the library loads)
    _child_maps(sys.argv[1])
