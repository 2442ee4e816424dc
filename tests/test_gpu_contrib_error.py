"""The error-weighted blend statistics (GaussianRasterizer(..., contributions=ErrorStats, pixel_error=E)) on the GPU.

Against float64 (tests/contrib_error_ref.py, anchored by tests/test_contrib_error_ref.py) on the seven fixtures of test_gpu_contrib, two
of them 100 x 60 (neither a multiple of the 16-pixel tile: the out-of-image lanes): a Gaussian that reaches no fragile pixel of the
oracle has the reference's error sum within the project's gradient bound - the sum IS the colour gradient under the upstream E.  HIP
against HIP on the multi-chunk frame: the sum equals the plain frame's colors_precomp gradient under dL/dcolor[0] = E.  And bits: E = 1
gives the weight sum's bits (the association of the fourth total is the third's; this says nothing about contraction: a product with
1 is exact, fused or not), the clamp is the clamped map's bits, the frame and the three statistics are the plain statistics frame's,
and the integer accumulator and the fold make the same frames give the same tensors (the side-stream case lives in
tests/test_gpu_streams_contrib_error.py)."""
import functools
import math
import random
from dataclasses import replace

import numpy as np
import pytest
import torch

import contrib_error_ref as ER
import streams as ST
from test_gpu_contrib import (CONTRIB_FIXTURES, FRAGILE_G_CAP, _fresh, _model, _multi_chunk, _parent_loop, _plain_frame, _reference, _same_stats,
                              _stats_frame, _training_fixture, _two_cameras)
from test_gpu_parity import DEV, FIXTURES, GRAD_ATOL_REL, GRAD_RTOL, _fixture_id, _inputs, _settings

pytestmark = pytest.mark.gpu


def test_the_cap_and_the_odd_sized_fixture():
    assert FRAGILE_G_CAP <= 0.15
    assert len(CONTRIB_FIXTURES) == 7
    assert any(FIXTURES[i]["W"] % 16 or FIXTURES[i]["H"] % 16 for i in CONTRIB_FIXTURES)


def _new_stats(P):
    from diff_gaussian_rasterization.contrib import ErrorStats
    return ErrorStats(P, DEV)


def _seeded_map(kw, seed):
    return torch.rand(kw["image_height"], kw["image_width"], generator=torch.Generator().manual_seed(seed))


def _error_frame(kw, E, stats=None, debug=False):
    """One error frame through the standard API -> (color, radii, stats).  E: a host or device map, or None."""
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    stats = _new_stats(P) if stats is None else stats
    color, radii = GaussianRasterizer(_settings(kw, debug), contributions=stats, pixel_error=None if E is None else E.to(DEV))(
        means2D=torch.zeros(P, 3, device=DEV), **inp)
    return color, radii, stats


def _error_bits(st):
    return {"error_frame_q32": st.error_frame_q32, "error_sum_q32": st.error_sum_q32, "error_max": st.error_max}


def _same_errors(a, b):
    return all(ST.same_bits(x, y) for x, y in zip(_error_bits(a).values(), _error_bits(b).values()))


@functools.lru_cache(maxsize=None)
def _error_reference(i):
    """(E, esum float64 [P]) of fixture i under its seeded map: computed once, shared, never written."""
    kw, fr = _reference(i)[:2]
    E = _seeded_map(kw, 500 + i)
    return E, ER.error_sums(fr, E.double().numpy())[0]


# ---- against float64 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", CONTRIB_FIXTURES, ids=lambda i: _fixture_id(FIXTURES[i]))
def test_error_sum_against_float64(i):
    kw, fr = _reference(i)[:2]
    E, esum = _error_reference(i)
    frag = fr.fragile_g.astype(bool)
    assert frag.mean() <= FRAGILE_G_CAP, f"fragile_g marks {frag.mean():.3f} of the Gaussians: the strict check would cover too few"
    color, radii, st = _error_frame(kw, E)
    torch.cuda.synchronize()
    assert st.frames == 1
    got = st.error_sum.cpu().numpy()
    strict = ~frag
    bound = GRAD_ATOL_REL * np.abs(esum).max() + GRAD_RTOL * np.abs(esum)
    ratio = (np.abs(got - esum) / bound)[strict].max(initial=0.0)
    print(f"fixture {i}: {int((esum > 0).sum())} of {fr.P} Gaussians carry error, {int(frag.sum())} fragile; error_sum worst err / bound "
          f"{ratio:.3f} (max esum {esum.max():.4f})")
    assert (esum[strict] > 0).any()
    assert ratio <= 1.0
    # after one frame the maximum is the sum, rounded once, and the frame accumulator is clear
    assert ST.same_bits(st.error_max, st.error_sum.float())
    assert not st.error_frame_q32.any()
    assert ((st.error_sum_q32 > 0) <= (st.count > 0)).all()


# ---- bits: E = 1, E = 0, the clamp, the plain frame --------------------------------------------------------------------------------

@pytest.mark.parametrize("i", (4, 6), ids=lambda i: _fixture_id(FIXTURES[i]))
def test_unit_map_gives_the_weight_sum_and_zero_map_gives_zeros(i):
    kw = _reference(i)[0]
    H, W = kw["image_height"], kw["image_width"]
    st = _error_frame(kw, torch.ones(H, W))[2]
    assert int(st.weight_sum_q32.sum()) > 0
    assert torch.equal(st.error_sum_q32, st.weight_sum_q32)
    assert _same_errors(st, _error_frame(kw, torch.ones(1, H, W))[2])              # [1,H,W] is the same map
    st = _error_frame(kw, torch.zeros(H, W))[2]
    assert int(st.weight_sum_q32.sum()) > 0 and st.frames == 1
    assert not st.error_frame_q32.any() and not st.error_sum_q32.any() and not st.error_max.any()


@pytest.mark.parametrize("i", (4, 6), ids=lambda i: _fixture_id(FIXTURES[i]))
def test_the_map_is_read_clamped(i):
    kw = _reference(i)[0]
    E = _seeded_map(kw, 77).clone()
    flat = E.view(-1)
    pick = torch.randperm(flat.numel(), generator=torch.Generator().manual_seed(78))
    n = flat.numel() // 10
    for k, v in enumerate((-3.0, 7.0, float("nan"), float("inf"))):
        flat[pick[k * n:(k + 1) * n]] = v
    clamped = torch.where(torch.isnan(E), torch.zeros_like(E), E).clamp(0, 1)
    assert clamped.min() == 0 and clamped.max() == 1 and torch.isfinite(clamped).all() and not torch.isfinite(E).all()
    a, b = _error_frame(kw, E)[2], _error_frame(kw, clamped)[2]
    assert int(a.error_sum_q32.sum()) > 0 and _same_errors(a, b) and _same_stats(a, b)
    assert float(a.error_max.max()) <= float(a.weight_sum.max()) and torch.isfinite(a.error_max).all()


@pytest.mark.parametrize("i", (4, 6), ids=lambda i: _fixture_id(FIXTURES[i]))
def test_error_frame_is_the_plain_frame_and_the_plain_statistics_frame(i):
    kw = _reference(i)[0]
    color, radii, st = _error_frame(kw, _error_reference(i)[0])
    plain_color, plain_radii = _plain_frame(kw)
    assert ST.same_bits(color, plain_color) and ST.same_bits(radii, plain_radii)
    assert int(st.count.sum()) > 0 and _same_stats(st, _stats_frame(kw)[2])
    assert _same_errors(st, _error_frame(kw, _error_reference(i)[0], debug=True)[2])


def test_an_error_stats_without_a_map_is_a_plain_statistics_frame():
    kw = _reference(4)[0]
    st = _new_stats(np.asarray(kw["means3D"]).shape[0])
    st.error_frame_q32[:] = 5
    st.error_sum_q32[:] = 7
    st.error_max[:] = 0.25
    before = {k: v.clone() for k, v in _error_bits(st).items()}
    color, radii, st = _error_frame(kw, None, stats=st)
    assert st.frames == 1 and _same_stats(st, _stats_frame(kw)[2])
    assert all(torch.equal(v, before[k]) for k, v in _error_bits(st).items())


# ---- several chunks, HIP against HIP -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _multi_chunk_error():
    """The multi-chunk frame of test_gpu_contrib under a seeded map: its error frame, and the plain frame's colors_precomp gradient of
    channel 0 under dL/dcolor = (E, 0, 0).  Computed once, shared."""
    import diff_gaussian_rasterization as dgr
    m = _multi_chunk()
    kw = m["kw"]
    P = np.asarray(kw["means3D"]).shape[0]
    E = _seeded_map(kw, 93).to(DEV)
    leaves = _inputs(kw, True)
    plain_color, _ = dgr.GaussianRasterizer(_settings(kw))(means2D=torch.zeros(P, 3, device=DEV), **leaves)
    up = torch.zeros_like(plain_color)
    up[0] = E
    plain_color.backward(up)
    color, radii, st = _error_frame(kw, E)
    torch.cuda.synchronize()
    return dict(kw=kw, E=E, st=st, color=color, radii=radii, grad=leaves["colors_precomp"].grad[:, 0].double().cpu().numpy())


def test_multi_chunk_error_sum_is_the_colour_gradient_under_the_map():
    m, e = _multi_chunk(), _multi_chunk_error()
    assert m["plan"][0] > 1 and m["plan"][1] != 0, m["plan"]
    got, want = e["st"].error_sum.cpu().numpy(), e["grad"]
    bound = GRAD_ATOL_REL * np.abs(want).max() + GRAD_RTOL * np.abs(want)
    ratio = (np.abs(got - want) / bound).max()
    print(f"multi-chunk: {int((want != 0).sum())} of {want.size} Gaussians carry error; error_sum vs colour gradient worst err / bound {ratio:.3f}")
    assert (want != 0).sum() > 1000
    assert ratio <= 1.0
    assert ST.same_bits(e["color"], m["plain_color"]) and ST.same_bits(e["radii"], m["plain_radii"]) and _same_stats(e["st"], m["st"])
    assert ST.same_bits(e["st"].error_max, e["st"].error_sum.float()) and not e["st"].error_frame_q32.any()


def test_an_error_frame_that_outgrows_its_first_workspace_is_added_once():
    """With no workspace guess the first attempt blends the first chunk - adding its totals to the frame accumulator - and stops with
    GSR_ERR_WORKSPACE in front of a later chunk; the re-run must start from a clear accumulator, and the fold must run once."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    e = _multi_chunk_error()
    errors, folds, orig, orig_fold = [], [], N.forward_render, N.contrib_error_fold

    def spy(*a, **k):
        try:
            return orig(*a, **k)
        except N.GsrError as err:
            errors.append(err.status)
            raise

    def spy_fold(*a, **k):
        folds.append(1)
        return orig_fold(*a, **k)
    dgr._binning_guess.clear()
    N.forward_render, N.contrib_error_fold = spy, spy_fold
    try:
        st = _error_frame(e["kw"], e["E"])[2]
    finally:
        N.forward_render, N.contrib_error_fold = orig, orig_fold
    dgr._binning_guess.clear()
    assert errors == [N.ERR_WORKSPACE] and folds == [1], (errors, folds)
    assert st.frames == 1 and _same_errors(st, e["st"]) and _same_stats(st, e["st"])


def test_one_call_forward_equals_the_two_stage_frame():
    """gsr_forward_contrib_error (both stages in one call) on a workspace that holds every instance, then the fold: the two-stage
    frame's tensors."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    kw = _reference(6)[0]
    E = _error_reference(6)[0].to(DEV)
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    want = _new_stats(P)
    color, radii, fr = dgr.rasterize_forward(inp["means3D"], inp.get("shs"), inp.get("colors_precomp"), inp["opacities"], inp.get("scales"),
                                             inp.get("rotations"), inp.get("cov3D_precomp"), _settings(kw), contrib=want, pixel_error=E)
    R = fr.R
    got = _new_stats(P)
    tiles = ((kw["image_width"] + 15) // 16) * ((kw["image_height"] + 15) // 16)
    with torch.cuda.device(DEV):
        binning = torch.empty(dgr._binning_bytes(R, tiles), dtype=torch.uint8, device=DEV)
        color2, radii2 = torch.empty_like(color), torch.empty_like(radii)
        plan, done = N.forward_both(fr.desc, fr.cam, fr.gauss, torch.empty_like(fr.geom_ws), torch.empty_like(fr.image_ws), radii2, binning, R,
                                    color2, torch.device(DEV), contrib=got.native(), err=got.native_error(E))
        torch.cuda.synchronize()
        assert done and int(plan.num_rendered) == R
        assert int(got.error_frame_q32.sum()) > 0 and not got.error_sum_q32.any()          # the frame's totals, not yet folded
        assert torch.equal(got.error_frame_q32, want.error_sum_q32)
        got.fold()
    torch.cuda.synchronize()
    assert _same_errors(got, want) and _same_stats(got, want) and ST.same_bits(color2, color) and ST.same_bits(radii2, radii)


def test_frames_that_bin_nothing_read_no_map():
    """P = 0 (where the C ABI lets both members of gsr_contrib_error be NULL) and num_rendered = 0: nothing is blended, the frame
    runs the plain statistics kernel and never loads the map; the image is the background and every tensor stays zero."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizer, _native as N
    kw = _reference(6)[0]
    H, W = kw["image_height"], kw["image_width"]
    rs = _settings(kw)
    bg = torch.as_tensor(np.asarray(kw["bg"]), dtype=torch.float32, device=DEV)[:, None, None].expand(3, H, W)
    z = lambda *s: torch.zeros(*s, device=DEV)
    E = torch.ones(H, W, device=DEV)
    # P = 0 through the rasterizer (error_frame_q32 is an empty tensor: NULL at the C ABI), then the same frame's stage 2 with no map
    st = _new_stats(0)
    color, radii = GaussianRasterizer(rs, contributions=st, pixel_error=E)(means3D=z(0, 3), means2D=z(0, 3), opacities=z(0, 1), shs=z(0, 9, 3),
                                                                            scales=z(0, 3), rotations=z(0, 4))
    assert radii.numel() == 0 and st.frames == 1 and torch.equal(color, bg)
    color1, _, fr = dgr.rasterize_forward(z(0, 3), z(0, 9, 3), None, z(0, 1), z(0, 3), z(0, 4), None, rs, contrib=st, pixel_error=E)
    color2 = torch.full_like(color1, -1.0)
    with torch.cuda.device(DEV):
        N.forward_render(fr.desc, fr.cam, fr.gauss, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan, color2, torch.device(DEV),
                         contrib=N.ContribStats(None, None, None), err=N.ContribError(None, None))
    torch.cuda.synchronize()
    assert torch.equal(color2, bg)
    # everything behind the camera: P > 0, R = 0
    inp = _inputs(kw, False)
    inp["means3D"][:, 2] = -1.0
    P = inp["means3D"].shape[0]
    st = _new_stats(P)
    color, radii = GaussianRasterizer(rs, contributions=st, pixel_error=E)(means2D=z(P, 3), **inp)
    torch.cuda.synchronize()
    assert not radii.any() and torch.equal(color, bg) and st.frames == 1
    assert not st.count.any() and not any(t.any() for t in _error_bits(st).values())


def test_a_frame_that_raises_leaves_the_frame_accumulator_clear():
    """A stage 2 that fails for another reason than the workspace, behind chunks that have already added their totals: no fold
    follows, so the frame accumulator is cleared on the way out and the next frame into the same object is that frame alone."""
    from diff_gaussian_rasterization import _native as N
    kw, E = _reference(4)[0], _error_reference(4)[0]
    want = _error_frame(kw, E)[2]
    st = _new_stats(want.P)
    orig = N.forward_render

    def failing(*a, **k):
        orig(*a, **k)                                # the whole frame is blended and added, then the call reports a failure
        err = N.GsrError("gsr_forward_render_contrib_error failed (status -3): injected")
        err.status = -3
        raise err
    N.forward_render = failing
    try:
        with pytest.raises(N.GsrError, match="injected"):
            _error_frame(kw, E, stats=st)
    finally:
        N.forward_render = orig
    torch.cuda.synchronize()
    assert st.frames == 0 and int(st.count.sum()) > 0                      # (the three statistics keep what was added, as before)
    assert not st.error_frame_q32.any() and not st.error_sum_q32.any() and not st.error_max.any()
    _error_frame(kw, E, stats=st)
    assert _same_errors(st, want)


# ---- accumulation ----------------------------------------------------------------------------------------------------------------

def test_two_cameras_add_their_sums_and_keep_the_larger_maximum():
    kw_a, kw_b = _two_cameras()
    E_a, E_b = _seeded_map(kw_a, 41), _seeded_map(kw_b, 42)
    a, b = _error_frame(kw_a, E_a)[2], _error_frame(kw_b, E_b)[2]
    both = _error_frame(kw_b, E_b, stats=_error_frame(kw_a, E_a)[2])[2]
    swapped = _error_frame(kw_a, E_a, stats=_error_frame(kw_b, E_b)[2])[2]
    assert both.frames == 2 and int(a.error_sum_q32.sum()) > 0 and int(b.error_sum_q32.sum()) > 0
    assert not torch.equal(a.error_sum_q32, b.error_sum_q32)
    assert torch.equal(both.error_sum_q32, a.error_sum_q32 + b.error_sum_q32)
    assert ST.same_bits(both.error_max, torch.maximum(a.error_max, b.error_max))
    assert bool((a.error_max > b.error_max).any()) and bool((b.error_max > a.error_max).any())
    assert not both.error_frame_q32.any()
    assert _same_errors(both, swapped) and _same_stats(both, swapped)
    again = _error_frame(kw_b, E_b, stats=_error_frame(kw_a, E_a)[2])[2]
    assert _same_errors(both, again) and _same_stats(both, again)
    both.reset()
    assert both.frames == 0 and not any(t.any() for t in _error_bits(both).values()) and not both.count.any()


def test_two_runs_give_equal_bits():
    for i in (4, 6):
        kw, E = _reference(i)[0], _error_reference(i)[0]
        a, b = _error_frame(kw, E)[2], _error_frame(kw, E)[2]
        assert int(a.error_sum_q32.sum()) > 0 and _same_errors(a, b)
    e = _multi_chunk_error()
    assert _same_errors(_error_frame(e["kw"], e["E"])[2], e["st"])


# ---- entry points ----------------------------------------------------------------------------------------------------------------

def _camera_settings(gm, cam):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    return GaussianRasterizationSettings(int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                         torch.zeros(3, device=DEV), 1.0, cam.world_view_transform, cam.full_proj_transform, gm.active_sh_degree,
                                         cam.camera_center, False, False)


def test_forward_forward_raw_and_render_agree():
    """render(..., pixel_error=) adds exactly what the rasterizer adds when it is called with the getters' tensors.  forward_raw runs
    the activations in the kernels and differs from the getters in their last bit: its sums are held to the getters' by the rule
    test_gpu_contrib has for the two paths' weight sums (the gradient rule of the raw mode, on all but 2e-4 of the rows)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    from gaussian_params import Pipe
    from gaussian_renderer import render
    gm, cams = _model()
    cam = cams[0]
    P = gm.get_xyz.shape[0]
    E = torch.rand(int(cam.image_height), int(cam.image_width), generator=torch.Generator().manual_seed(61)).to(DEV)
    rs = _camera_settings(gm, cam)
    raw, get, via = _new_stats(P), _new_stats(P), _new_stats(P)
    z = torch.zeros(P, 3, device=DEV)
    with torch.no_grad():
        GaussianRasterizer(rs, contributions=raw, pixel_error=E).forward_raw(gm._xyz, z, gm._features, None, gm._opacity, gm._scaling, gm._rotation)
        c_get, r_get = GaussianRasterizer(rs, contributions=get, pixel_error=E)(
            means3D=gm.get_xyz, means2D=z, shs=gm.get_features, opacities=gm.get_opacity, scales=gm.get_scaling, rotations=gm.get_rotation)
    bg = torch.zeros(3, device=DEV)
    out = render(cam, gm, Pipe(), bg, contributions=via, pixel_error=E[None])
    assert via.frames == 1 and int(get.error_sum_q32.sum()) > 0
    assert _same_errors(via, get) and _same_stats(via, get)
    assert ST.same_bits(out["render"], c_get) and ST.same_bits(out["radii"], r_get)
    a, b = raw.error_sum, get.error_sum
    bad_rows = (a - b).abs() > 2e-5 * float(a.max()) + 2e-3 * a
    print(f"forward_raw vs forward: error_sum on {int(bad_rows.sum())} of {P} rows beyond the gradient rule")
    assert int(raw.error_sum_q32.sum()) > 0 and float(bad_rows.double().mean()) <= 2e-4
    assert ST.same_bits(raw.error_max, raw.error_sum.float())
    # render without the map: a plain statistics frame into the same object
    before = {k: v.clone() for k, v in _error_bits(via).items()}
    render(cam, gm, Pipe(), bg, contributions=via)
    assert via.frames == 2 and torch.equal(via.count, 2 * get.count) and all(torch.equal(v, before[k]) for k, v in _error_bits(via).items())


def test_every_refusal_of_the_python_layer():
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization.contrib import ContributionStats
    from gaussian_params import Pipe
    from gaussian_renderer import render
    kw = _reference(6)[0]
    H, W = kw["image_height"], kw["image_width"]
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    z = torch.zeros(P, 3, device=DEV)
    E = torch.zeros(H, W, device=DEV)
    rs = _settings(kw)
    with pytest.raises(ValueError, match="pixel_error without contributions"):
        GaussianRasterizer(rs, pixel_error=E)
    with pytest.raises(ValueError, match="ErrorStats"):
        GaussianRasterizer(rs, contributions=ContributionStats(P, DEV), pixel_error=E)
    for kwargs in (dict(depth_alpha=True), dict(absgrad=True)):
        with pytest.raises(ValueError, match="contributions"):
            GaussianRasterizer(rs, contributions=_new_stats(P), pixel_error=E, **kwargs)
    st = _new_stats(P)
    for bad, match in ((torch.zeros(W, H, device=DEV), "shape"), (torch.zeros(3, H, W, device=DEV), "shape"),
                       (torch.zeros(H, W + 1, device=DEV), "shape"), (torch.zeros(H, W, device=DEV, dtype=torch.float64), "float32"),
                       (torch.zeros(H, W), "lives on")):
        with pytest.raises(ValueError, match=match):
            GaussianRasterizer(rs, contributions=st, pixel_error=bad)(means2D=z, **inp)
    # everything a statistics frame refuses
    with pytest.raises(ValueError, match=f"{P + 1} Gaussians"):
        GaussianRasterizer(rs, contributions=_new_stats(P + 1), pixel_error=E)(means2D=z, **inp)
    with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
        GaussianRasterizer(rs, contributions=st, pixel_error=E)(means2D=z, **_inputs(kw, True))
    gm, cams = _model()
    n = gm.get_xyz.shape[0]
    with pytest.raises(ValueError, match="pixel_error without contributions"):
        render(cams[0], gm, Pipe(), torch.zeros(3, device=DEV), pixel_error=torch.zeros(96, 128, device=DEV))
    with pytest.raises(ValueError, match="contributions"):
        render(cams[0], gm, Pipe(), torch.zeros(3, device=DEV), depth_alpha=True, contributions=_new_stats(n),
               pixel_error=torch.zeros(96, 128, device=DEV))
    torch.cuda.synchronize()
    assert st.frames == 0 and not st.count.any() and not any(t.any() for t in _error_bits(st).values())      # nothing was launched


def test_model_error_stats_over_chosen_views_and_with_a_correction():
    from diff_gaussian_rasterization.contrib import l1_error_map
    from gaussian_params import Pipe
    from gaussian_renderer import render
    gm, cams = _model()
    P = gm.get_xyz.shape[0]
    bg = torch.zeros(3, device=DEV)
    g = torch.Generator().manual_seed(5)
    targets = [torch.rand(3, 96, 128, generator=g).to(DEV) for _ in cams]
    one = []
    with torch.no_grad():
        for cam, target in zip(cams, targets):
            st = _new_stats(P)
            render(cam, gm, Pipe(), bg, contributions=st, pixel_error=l1_error_map(render(cam, gm, Pipe(), bg)["render"], target))
            one.append(st)
    every = gm.error_stats(cams, targets)
    assert every.frames == 3 and every.P == P and int(every.error_sum_q32.sum()) > 0
    assert torch.equal(every.error_sum_q32, sum(s.error_sum_q32 for s in one))
    assert ST.same_bits(every.error_max, torch.stack([s.error_max for s in one]).max(0).values)
    assert torch.equal(every.count, sum(s.count for s in one))
    some = gm.error_stats(cams, targets, views=[2, 0])
    assert some.frames == 2 and torch.equal(some.error_sum_q32, one[0].error_sum_q32 + one[2].error_sum_q32)
    seen = []

    def correct(image, idx):
        seen.append(idx)
        return targets[idx]                       # a correction that makes the image the target: no error is left
    none = gm.error_stats(cams, targets, views=[1], correct=correct)
    assert seen == [1] and none.frames == 1 and int(none.count.sum()) > 0 and not none.error_sum_q32.any() and not none.error_max.any()
    with pytest.raises(ValueError, match="targets"):
        gm.error_stats(cams, targets[:2])


# ---- the training loop -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("score", ("max", "sum"))
def test_training_loop_grows_by_the_budget_at_every_refinement(score):
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, cams, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), densify_from_iter=5, densification_interval=10, densify_until_iter=35, densify_error_views=2,
                  densify_error_growth=0.05, densify_error_score=score)
    gm = _fresh(scene, opt)
    sizes, losses, expected, budgets, used = {}, [], {}, [], []
    body, prune, stats_of = gm._densify_hot_and_prune, gm.prune_points, gm.error_stats
    state = {}

    def spy_stats(cameras, targets_, pipe=None, bg=None, views=None, correct=None):
        used.append(list(views))
        state["stats"] = stats_of(cameras, targets_, pipe, bg, views=views, correct=correct)
        return state["stats"]

    def spy_prune(mask):
        state["dropped"].append(int(mask.sum()))
        return prune(mask)

    def spy_body(hot, big, *a):
        p0 = gm.get_xyz.shape[0]
        st = state["stats"]
        scores = st.error_max.double() if score == "max" else st.error_sum
        n = min(math.ceil(opt.densify_error_growth * p0), int((scores > 0).sum()))
        top = torch.sort(scores, stable=True, descending=True).indices[:n]
        want = torch.zeros(p0, dtype=torch.bool, device=DEV)
        want[top] = True
        assert torch.equal(hot, want)
        clones, splits = int((hot & ~big).sum()), int((hot & big).sum())
        state["dropped"] = []
        body(hot, big, *a)
        assert state["dropped"][0] == splits and len(state["dropped"]) == 2           # (the split originals, then the prune)
        budgets.append((p0, n, clones + splits))
        expected[state["it"]] = p0 + clones + 2 * splits - splits - state["dropped"][1]
    gm._densify_hot_and_prune, gm.prune_points, gm.error_stats = spy_body, spy_prune, spy_stats
    random.seed(1)
    torch.manual_seed(1)

    def note(it, loss, g):
        sizes[it] = g.get_xyz.shape[0]
        losses.append(float(loss.detach()))
        state["it"] = it + 1
    state["it"] = 1
    train(gm, cams, targets, opt, Pipe(), bg, iterations=40, scene_extent=3.0, on_iteration=note)
    assert sorted(expected) == [10, 20, 30] and len(losses) == 40 and all(np.isfinite(losses))
    p = 2000
    for it in range(1, 41):
        p = expected.get(it, p)
        assert sizes[it] == p, (it, sizes[it], p)
    for p0, n, grown in budgets:
        assert n == grown == math.ceil(0.05 * p0)                                   # the budget was there to be spent, and was
    assert budgets[0][0] == 2000 and sizes[40] > 2000
    assert all(len(v) == 2 and len(set(v)) == 2 and all(0 <= i < len(cams) for i in v) for v in used) and len(used) == 3
    for g in gm.optimizer.param_groups:
        for q in g["params"]:
            assert q.shape[0] == sizes[40] and gm.optimizer.state[q]["exp_avg"].shape == q.shape


def test_training_loop_with_a_bilateral_grid_scores_the_corrected_image():
    """opt.bilateral_grid with densify_error_views: at a refinement the camera's grid stands between the render and the error map
    (the BilateralGrid module is error_stats' `correct`, called under no_grad), and the loop refines and goes on."""
    from diff_gaussian_rasterization.contrib import l1_error_map
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import OptimizationDefaults
    from train_loop import train
    scene, cams, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), densify_from_iter=5, densification_interval=10, densify_until_iter=25, densify_error_views=2,
                  bilateral_grid=True, bilateral_grid_shape=(4, 4, 2))
    gm = _fresh(scene, opt)
    stats_of, calls, sizes, losses = gm.error_stats, [], {}, []

    def spy_stats(cameras, targets_, pipe=None, bg=None, views=None, correct=None):
        st = stats_of(cameras, targets_, pipe, bg, views=views, correct=correct)
        assert correct is gm.bilagrid and not torch.is_grad_enabled()
        # the same views by hand, through the grid: the loop's statistics
        by_hand = _new_stats(st.P)
        for idx in views:
            image = correct(render(cameras[idx], gm, pipe, bg)["render"], idx)
            assert not image.requires_grad
            render(cameras[idx], gm, pipe, bg, contributions=by_hand, pixel_error=l1_error_map(image, targets_[idx]))
        assert _same_errors(st, by_hand) and int(st.error_sum_q32.sum()) > 0
        calls.append(list(views))
        return st
    gm.error_stats = spy_stats
    random.seed(4)
    torch.manual_seed(4)

    def note(it, loss, g):
        sizes[it] = g.get_xyz.shape[0]
        losses.append(float(loss.detach()))
    train(gm, cams, targets, opt, Pipe(), bg, iterations=30, scene_extent=3.0, on_iteration=note)
    assert len(calls) == 2 and len(losses) == 30 and all(np.isfinite(losses))
    assert sizes[9] == 2000 and sizes[10] != 2000 and sizes[20] != sizes[19] and sizes[30] == sizes[20]
    assert gm.bilagrid.grids.grad is None or torch.isfinite(gm.bilagrid.grids.grad).all()


def test_with_error_views_off_the_loop_is_the_parents_bit_for_bit():
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, cams, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), densify_from_iter=10, densification_interval=10, densify_until_iter=35, densify_grad_threshold=1e-5,
                  densify_error_views=0)
    assert OptimizationDefaults().densify_error_views == 0
    runs = []
    for loop in (lambda gm: train(gm, cams, targets, opt, Pipe(), bg, iterations=40, scene_extent=3.0),
                 lambda gm: _parent_loop(gm, cams, targets, opt, Pipe(), bg, 40, 3.0)):
        gm = _fresh(scene, opt)
        random.seed(2)
        torch.manual_seed(2)
        loop(gm)
        torch.cuda.synchronize()
        runs.append(gm)
    a, b = runs
    assert a.get_xyz.shape[0] == b.get_xyz.shape[0] != 2000            # densification ran, and both runs took the same decisions
    for name in ("_xyz", "_features", "_opacity", "_scaling", "_rotation"):
        assert ST.same_bits(getattr(a, name).detach(), getattr(b, name).detach()), name
