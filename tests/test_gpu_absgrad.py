"""Absgrad on the device: GaussianRasterizer(absgrad=True) against the float64 reference (tests/absgrad_ref.py, anchored to the
oracle by tests/test_absgrad_ref.py), per element, on the smallest fixtures that reach every path of the abs blend backward:

    fixture 0  P=1     32x32     one entry
    fixture 2  P=64    48x80     lists under one batch of 64
    fixture 4  P=2048  128x128   every tile over 64 entries, one over the 128-entry segment
    fixture 6  P=2048  100x60    precomputed covariance, partial edge tiles, 23 of 28 tiles over 128
    fixture 8  P=5000  256x192   scale_modifier 1.7, lists up to 382: 2-3 segments per tile

Bound: the project's gradient bound GRAD_ATOL_REL max|want| + GRAD_RTOL |want| (1e-4).  The per-pixel terms of the absolute sums are
the signed gradient's terms without cancellation: their error is no larger, relative to a scale that is no smaller.
"""
import functools
import types

import numpy as np
import pytest
import torch

import absgrad_ref as AR
import oracle
import scene_synth as S
import test_gpu_parity as TP
from util import raster_kwargs

pytestmark = pytest.mark.gpu

DEV = TP.DEV
ABS_FIXTURES = (0, 2, 4, 6, 8)


def _run(kw, grad_img, absgrad, raw_scene=None):
    """Forward + backward through GaussianRasterizer(absgrad=...).  grad_img: array, or callable (color, radii) -> dL/dcolor.
    raw_scene: render through forward_raw (split SH tables) from that scene's raw parameters instead of kw's activated ones.
    Returns (color, radii, grads {name: array} incl. means2D, absgrad array or None)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    rs = TP._settings(kw)
    P = np.asarray(kw["means3D"]).shape[0]
    means2D = torch.zeros(P, 3, device=DEV, requires_grad=True)
    ras = GaussianRasterizer(rs, absgrad=absgrad)
    if raw_scene is None:
        inp = TP._inputs(kw, True)
        color, radii = ras(means2D=means2D, **inp)
    else:
        t = lambda a: a.detach().clone().float().to(DEV).requires_grad_(True)
        inp = dict(means3D=t(raw_scene.means3D), features_dc=t(raw_scene.shs[:, :1]), features_rest=t(raw_scene.shs[:, 1:]),
                   opacity_logits=t(raw_scene.opacity_logits), log_scales=t(raw_scene.log_scales), raw_rotations=t(raw_scene.raw_rotations))
        color, radii = ras.forward_raw(inp["means3D"], means2D, inp["features_dc"], inp["features_rest"], inp["opacity_logits"],
                                       inp["log_scales"], inp["raw_rotations"])
    if callable(grad_img):
        grad_img = grad_img(color.detach().cpu().numpy(), radii.cpu().numpy())
    color.backward(torch.as_tensor(np.ascontiguousarray(grad_img), dtype=torch.float32).to(DEV))
    torch.cuda.synchronize()
    grads = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    grads["means2D"] = means2D.grad.detach().cpu().numpy()
    ab = means2D.absgrad.detach().cpu().numpy() if hasattr(means2D, "absgrad") else None
    return color.detach().cpu().numpy(), radii.cpu().numpy(), grads, ab


@functools.lru_cache(maxsize=None)
def _fixture_result(i):
    """One fixture, computed once and shared: the oracle's frame, the masked gradient image, the float64 reference, and the device
    runs with absgrad on (twice) and off."""
    c = TP.FIXTURES[i]
    kw = TP._fixture_kwargs(c)
    fr64 = oracle.rasterize(dtype=np.float64, **kw)
    gimg = S.make_grad_image(c["W"], c["H"], c["seed"]).numpy()
    state = {}

    def masked(color, radii):
        state["strict"] = TP._strict_pixels(fr64, radii)
        return np.where(state["strict"][None], gimg, 0.0).astype(np.float32)
    color, radii, grads, ab = _run(kw, masked, True)
    gm = np.where(state["strict"][None], gimg, 0.0).astype(np.float32)
    _, _, grads2, ab2 = _run(kw, gm, True)
    _, _, grads_off, ab_off = _run(kw, gm, False)
    want = fr64.backward(gm.astype(np.float64))
    signed, absolute = AR.signed_and_abs_means2D(fr64, kw["bg"], gm.astype(np.float64))
    return types.SimpleNamespace(c=c, kw=kw, fr64=fr64, gm=gm, strict=state["strict"], radii=radii, grads=grads, ab=ab, grads2=grads2,
                                 ab2=ab2, grads_off=grads_off, ab_off=ab_off, want=want, signed=signed, absolute=absolute)


def _check_abs(ab, absolute, radii, label):
    """absgrad [P,3] against the reference's absolute sums [P,2]: every element within the gradient bound; column 2 and the rows of
    invisible Gaussians exactly zero."""
    assert ab is not None and ab.shape == (radii.shape[0], 3) and ab.dtype == np.float32
    err = np.abs(ab[:, :2].astype(np.float64) - absolute)
    scale = max(np.abs(absolute).max(initial=0.0), 1e-30)
    bound = TP.GRAD_ATOL_REL * scale + TP.GRAD_RTOL * np.abs(absolute)
    print(f"{label}: absgrad max err {err.max():.3e}, scale {scale:.3e}, worst err / bound {(err / bound).max():.3f}; "
          f"{int((absolute.max(1) > 0).sum())} Gaussians with a non-zero absgrad")
    assert (err <= bound).all(), f"{label}: {int((err > bound).sum())} elements off, worst ratio {(err / bound).max():.2f}"
    assert not ab[:, 2].any(), "column 2 must be exactly 0"
    assert not ab[radii == 0].any(), "rows of invisible Gaussians must be exactly 0"


def _triangle(ab, grad):
    a, g = ab[:, :2].astype(np.float64), np.abs(grad[:, :2].astype(np.float64))
    return (a >= g - 1e-5 * a - 1e-30).all()


@pytest.mark.parametrize("i", ABS_FIXTURES)
def test_absgrad_per_element_against_float64(i):
    r = _fixture_result(i)
    label = TP._fixture_id(r.c)
    frac = 1 - r.strict.mean()
    print(f"{label}: masked fraction {frac:.5f} (cap {TP.fragile_cap(r.c['frag']):.5f})")
    assert frac <= TP.fragile_cap(r.c["frag"])
    _check_abs(r.ab, r.absolute, r.radii, label)
    names = [n for n in TP.GRAD_NAMES if n in r.grads]
    live, strict_live = TP._check_grads(r.fr64, r.want, r.grads, names, masked=True)
    assert strict_live == live
    same = all(np.array_equal(r.grads[n], r.grads_off[n]) for n in r.grads)
    print(f"{label}: ordinary gradients of the absgrad=True run bit-equal to the absgrad=False run: {same}")


def test_absgrad_through_forward_raw():
    """Fixture 4 from its raw parameters (forward_raw, split SH tables): the same bounds."""
    r = _fixture_result(4)
    scene = TP._fixture_scene(r.c)[0]
    _, radii, grads, ab = _run(r.kw, r.gm, True, raw_scene=scene)
    np.testing.assert_array_equal(radii, r.fr64.radii)
    _check_abs(ab, r.absolute, radii, "fixture 4 forward_raw")
    # the screen-space gradient (the one ordinary gradient that is the same quantity in raw mode) against the oracle
    TP._check_grads(r.fr64, r.want, {"means2D": grads["means2D"]}, ["means2D"], masked=True)
    assert _triangle(ab, grads["means2D"])


@pytest.mark.parametrize("i", ABS_FIXTURES)
def test_triangle_inequality(i):
    r = _fixture_result(i)
    assert _triangle(r.ab, r.grads["means2D"])
    assert (r.absolute >= np.abs(r.signed)).all()


def test_symmetric_single_splat_on_the_device():
    """The symmetric splat of tests/test_absgrad_ref.py (b): the signed gradient cancels, |grad| <= 1e-4 absgrad."""
    kw = AR.single_splat_kwargs()
    gimg = np.ones((3, kw["image_height"], kw["image_width"]), np.float32) * np.array([0.3, -0.8, 0.5], np.float32)[:, None, None]
    _, radii, grads, ab = _run(kw, gimg, True)
    print(f"single splat: grad {grads['means2D'][0]}, absgrad {ab[0]}")
    assert radii[0] > 0 and (ab[0, :2] > 0).all() and ab[0, 2] == 0
    assert (np.abs(grads["means2D"][0, :2]) <= 1e-4 * ab[0, :2]).all()
    fr = oracle.rasterize(dtype=np.float64, **kw)
    _check_abs(ab, AR.signed_and_abs_means2D(fr, kw["bg"], gimg.astype(np.float64))[1], radii, "single splat")


@pytest.mark.parametrize("i", ABS_FIXTURES)
def test_absgrad_is_bitwise_deterministic(i):
    r = _fixture_result(i)
    assert np.array_equal(r.ab, r.ab2)
    for n in r.grads:
        assert np.array_equal(r.grads[n], r.grads2[n]), n
    assert r.ab_off is None


def test_frame_with_several_chunks_and_the_sparse_geometry_backward():
    """The posed uncovered half (test_gpu_parity._uncovered_half_posed): every planned chunk runs, the late ones through the live
    filter, so the geometry backward - and the absgrad extraction behind it - visit the binned prefix sparsely."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization import _native as N
    scene, cam = TP._uncovered_half_posed()
    kw = raster_kwargs(scene, cam)
    rs = TP._settings(kw)
    P = scene.P
    gimg = S.make_grad_image(cam.image_width, cam.image_height, 4).to(DEV)
    runs = []
    for absgrad in (True, True, False):
        inp = TP._inputs(kw, True)
        means2D = torch.zeros(P, 3, device=DEV, requires_grad=True)
        color, radii = GaussianRasterizer(rs, absgrad=absgrad)(means2D=means2D, **inp)
        fr = color.grad_fn.frame
        plan = fr.plan
        assert plan.chunks_run >= 2 and N.effective_binned_ranks(plan) * 4 < P, (plan.chunks_run, N.effective_binned_ranks(plan), P)
        order = N.frame_arrays(fr.desc, color.grad_fn.saved_tensors[0])[1][:N.binned_prefix(plan)].long().clone()
        color.backward(gimg)
        torch.cuda.synchronize()
        runs.append((radii, {k: v.grad for k, v in inp.items()} | {"means2D": means2D.grad}, getattr(means2D, "absgrad", None), order))
    (radii, g1, a1, order), (_, g2, a2, _), (_, g0, a0, _) = runs
    assert a0 is None and a1.shape == (P, 3) and bool(torch.isfinite(a1).all())
    outside = torch.ones(P, dtype=torch.bool, device=DEV)
    outside[order] = False
    assert not bool(a1[outside].any()) and not bool(a1[radii == 0].any()) and not bool(a1[:, 2].any())
    assert int((a1[:, 0] > 0).sum()) > 1000
    assert _triangle(a1.cpu().numpy(), g1["means2D"].cpu().numpy())
    assert torch.equal(a1, a2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
        w, g = g0[n].double(), g1[n].double()
        assert bool(((g - w).abs() <= TP.GRAD_ATOL_REL * w.abs().max() + TP.GRAD_RTOL * w.abs()).all()), n
    print("several chunks: ordinary gradients bit-equal to the absgrad=False run:", all(torch.equal(g0[n], g1[n]) for n in g0))


def test_contract():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    from gaussian_params import GaussianParams, Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    W, H, P = 160, 112, 4000
    scene, cam = S.make_scene(P, W, H, 1, 41, scale_lo=0.005, scale_hi=0.06), S.make_camera(W, H)
    kw = raster_kwargs(scene, cam)
    rs = TP._settings(kw)
    gimg = S.make_grad_image(W, H, 2).to(DEV)
    # off: no attribute
    inp, means2D = TP._inputs(kw, True), torch.zeros(P, 3, device=DEV, requires_grad=True)
    GaussianRasterizer(rs)(means2D=means2D, **inp)[0].backward(gimg)
    assert not hasattr(means2D, "absgrad")
    # set whether or not means2D requires grad; nothing under no_grad
    means2D = torch.zeros(P, 3, device=DEV)
    GaussianRasterizer(rs, absgrad=True)(means2D=means2D, **TP._inputs(kw, True))[0].backward(gimg)
    assert means2D.absgrad.shape == (P, 3) and means2D.grad is None
    with torch.no_grad():
        means2D = torch.zeros(P, 3, device=DEV)
        GaussianRasterizer(rs, absgrad=True)(means2D=means2D, **TP._inputs(kw, False))
        assert not hasattr(means2D, "absgrad")
    # refused combinations
    with pytest.raises(ValueError, match="depth_alpha"):
        GaussianRasterizer(rs, depth_alpha=True, absgrad=True)
    inp = TP._inputs(kw, False)
    fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, rs,
                               tile_rows=(0, 2))[2]
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_backward_screen(fr, gimg, absgrad=True)
    pipe = Pipe()
    pipe.absgrad = True
    model = GaussianParams(scene.to(DEV)).to(DEV)
    fake_dist = types.SimpleNamespace(get_backend=lambda group=None: "nccl")
    with pytest.raises(ValueError, match="absgrad"):
        ShardedRenderer(fake_dist, 1, 0).render(cam.to(DEV), model, pipe, torch.zeros(3, device=DEV))
    # render() with pipe.absgrad; a second backward under retain_graph reassigns the same bits
    for fused in (False, True):
        pipe.fused_activations = fused
        out = render(cam.to(DEV), model, pipe, torch.zeros(3, device=DEV))
        out["render"].backward(gimg, retain_graph=True)
        vsp = out["viewspace_points"]
        first = vsp.absgrad
        assert first.shape == (P, 3) and int((first[:, 0] > 0).sum()) > 100
        out["render"].backward(gimg)
        assert vsp.absgrad is not first and torch.equal(vsp.absgrad, first)
    # debug=True takes the same route
    means2D = torch.zeros(P, 3, device=DEV, requires_grad=True)
    GaussianRasterizer(TP._settings(kw, debug=True), absgrad=True)(means2D=means2D, **TP._inputs(kw, True))[0].backward(gimg)
    plain = torch.zeros(P, 3, device=DEV, requires_grad=True)
    GaussianRasterizer(rs, absgrad=True)(means2D=plain, **TP._inputs(kw, True))[0].backward(gimg)
    assert torch.equal(means2D.absgrad, plain.absgrad)
    # the native densification statistics with densify_absgrad equal the host rule on the same tensors
    from dataclasses import replace
    gm = GaussianModel(1)
    gm.adopt_scene(scene, device=DEV)
    gm.training_setup(replace(OptimizationDefaults(), densify_absgrad=True))
    radii = out["radii"]
    gm.update_densification_stats(vsp, radii)
    torch.cuda.synchronize()
    vis = radii > 0
    want_acc, want_den = torch.zeros(P, 1, device=DEV), torch.zeros(P, 1, device=DEV)
    want_acc[vis] = torch.norm(vsp.absgrad[vis, :2], dim=-1, keepdim=True)
    want_den[vis] = 1
    assert torch.equal(gm.denom, want_den)
    assert bool(((gm.xyz_gradient_accum - want_acc).abs() <= 1e-6 * want_acc.abs()).all())
    assert not torch.equal(want_acc, torch.norm(vsp.grad[:, :2], dim=-1, keepdim=True) * vis[:, None])
    vsp2 = torch.zeros(P, 3, device=DEV, requires_grad=True)
    vsp2.grad = vsp.grad.clone()
    with pytest.raises(ValueError, match="pipe.absgrad"):
        gm.update_densification_stats(vsp2, radii)
