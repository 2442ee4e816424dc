"""The per-Gaussian blend statistics (GaussianRasterizer(..., contributions=)) on the GPU.

Against float64 (tests/contrib_ref.py, anchored to the oracle's image by tests/test_contrib_ref.py) on seven fixtures of
test_gpu_parity: a Gaussian that reaches no fragile pixel of the oracle (`fragile_g == 0`) has the reference's count exactly, its
weight sum within the gradient bound (it IS the colour gradient under a unit upstream) and its largest weight within the
strict-pixel bound of the image; the others may differ by one decision per fragile pixel.  HIP against HIP on the 260 k-Gaussian
frame that runs several depth chunks and live-filters one: the sum equals the plain frame's colors_precomp gradient, its total the
alpha map's.  And bits: the integer accumulators make the same frames give the same tensors, in any order (the side-stream case
lives in tests/test_gpu_streams_contrib.py, behind test_gpu_streams.py, whose sensitivity tests depend on which torch streams the
session has handed out before them)."""
import functools
import math
import random
from dataclasses import replace

import numpy as np
import pytest
import torch

import contrib_ref as CR
import oracle
import scene_synth as S
import streams as ST
from test_gpu_depth_alpha import _uncovered_half_kwargs
from test_gpu_parity import DEV, FIXTURES, GRAD_ATOL_REL, GRAD_RTOL, _fixture_id, _fixture_kwargs, _inputs, _settings
from util import raster_kwargs

pytestmark = pytest.mark.gpu

CONTRIB_FIXTURES = (0, 2, 4, 6, 9, 11, 13)
FRAGILE_G_CAP = 0.15             # of a fixture's Gaussians (measured on the CPU: at most 12.5 % on these seven; fixtures 8 and 14 sit
#                                  at 59 % and 26 % and are left out for that reason)
WEIGHT_MAX_ATOL = 1e-5           # the strict-pixel bound of test_gpu_parity._check_forward (binary32 restatement: 4.4e-6 at most here)


def _new_stats(P):
    from diff_gaussian_rasterization.contrib import ContributionStats
    return ContributionStats(P, DEV)


def _stats_frame(kw, stats=None, antialiasing=False, debug=False):
    """One statistics frame through the standard API -> (color, radii, stats)."""
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    stats = _new_stats(P) if stats is None else stats
    color, radii = GaussianRasterizer(_settings(kw, debug), antialiasing=antialiasing, contributions=stats)(
        means2D=torch.zeros(P, 3, device=DEV), **inp)
    return color, radii, stats


def _plain_frame(kw, **flags):
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, False)
    return GaussianRasterizer(_settings(kw), **flags)(means2D=torch.zeros(inp["means3D"].shape[0], 3, device=DEV), **inp)


def _bits(stats):
    return {"count": stats.count, "weight_sum_q32": stats.weight_sum_q32, "weight_max": stats.weight_max}


def _same_stats(a, b):
    return all(ST.same_bits(x, y) for x, y in zip(_bits(a).values(), _bits(b).values()))


@functools.lru_cache(maxsize=None)
def _reference(i):
    """(kw, fr64, count, weight_sum, weight_max) of fixture i: computed once, shared, never written."""
    kw = _fixture_kwargs(FIXTURES[i])
    fr = oracle.rasterize(dtype=np.float64, **kw)
    return (kw, fr) + CR.contributions(fr)


# ---- against float64 -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("i", CONTRIB_FIXTURES, ids=lambda i: _fixture_id(FIXTURES[i]))
def test_statistics_against_float64(i):
    kw, fr, count, wsum, wmax = _reference(i)
    frag = fr.fragile_g.astype(bool)
    assert frag.mean() <= FRAGILE_G_CAP, f"fragile_g marks {frag.mean():.3f} of the Gaussians: the strict checks would cover too few"
    color, radii, st = _stats_frame(kw)
    torch.cuda.synchronize()
    assert st.frames == 1
    np.testing.assert_array_equal(radii.cpu().numpy(), fr.radii)
    got_n, got_s, got_m = st.count.cpu().numpy(), st.weight_sum.cpu().numpy(), st.weight_max.double().cpu().numpy()
    strict = ~frag
    n_fragile_px = int((fr.fragile_px != 0).sum())
    d_count = np.abs(got_n - count)
    s_bound = GRAD_ATOL_REL * np.abs(wsum).max() + GRAD_RTOL * np.abs(wsum)
    s_ratio = (np.abs(got_s - wsum) / s_bound)[strict].max(initial=0.0)
    m_err = np.abs(got_m - wmax)[strict].max(initial=0.0)
    print(f"fixture {i}: {int((count > 0).sum())} of {fr.P} Gaussians composited, {int(frag.sum())} fragile ({frag.mean():.4f}), "
          f"{n_fragile_px} fragile pixels; count: {int((d_count[strict] != 0).sum())} strict off, worst fragile |delta| "
          f"{int(d_count[frag].max(initial=0))} (bound {n_fragile_px}); weight_sum worst err / bound {s_ratio:.3f}; "
          f"weight_max worst err {m_err:.3e} (err / bound {m_err / WEIGHT_MAX_ATOL:.3f})")
    assert (count[strict] > 0).any()
    np.testing.assert_array_equal(got_n[strict], count[strict])
    assert (d_count[frag] <= n_fragile_px).all()           # a Gaussian enters a pixel at most once
    assert s_ratio <= 1.0
    assert m_err <= WEIGHT_MAX_ATOL


# ---- the frame is otherwise the plain frame; several chunks, HIP against HIP ------------------------------------------------------

def test_statistics_frame_is_the_plain_frame_on_a_fixture():
    kw = _reference(4)[0]
    color, radii, _ = _stats_frame(kw)
    plain_color, plain_radii = _plain_frame(kw)
    assert ST.same_bits(color, plain_color) and ST.same_bits(radii, plain_radii)


@functools.lru_cache(maxsize=None)
def _multi_chunk():
    """The uncovered-half frame with a colour per Gaussian in place of the SH: its statistics frame, the plain frame's
    colors_precomp gradient under dL/dpix = (1, 0, 0), and the alpha map.  Computed once, shared."""
    import diff_gaussian_rasterization as dgr
    kw = {k: v for k, v in _uncovered_half_kwargs().items() if k != "shs"}
    P = np.asarray(kw["means3D"]).shape[0]
    kw["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(91)).numpy()
    inp = _inputs(kw, False)
    st = _new_stats(P)
    color, radii, fr = dgr.rasterize_forward(inp["means3D"], None, inp["colors_precomp"], inp["opacities"], inp["scales"], inp["rotations"],
                                             None, _settings(kw), contrib=st)
    plan = (int(fr.plan.chunks_run), int(fr.plan.chunks_filtered))
    leaves = _inputs(kw, True)
    plain_color, plain_radii = dgr.GaussianRasterizer(_settings(kw))(means2D=torch.zeros(P, 3, device=DEV), **leaves)
    up = torch.zeros_like(plain_color)
    up[0] = 1.0
    plain_color.backward(up)
    alpha = _plain_frame(kw, depth_alpha=True)[3]
    torch.cuda.synchronize()
    return dict(kw=kw, W=kw["image_width"], H=kw["image_height"], plan=plan, st=st, color=color, radii=radii,
                plain_color=plain_color.detach(), plain_radii=plain_radii, grad=leaves["colors_precomp"].grad[:, 0].double().cpu().numpy(),
                alpha_sum=float(alpha.double().sum()))


def test_multi_chunk_frame_runs_several_chunks_and_is_the_plain_frame():
    m = _multi_chunk()
    chunks_run, chunks_filtered = m["plan"]
    assert chunks_run > 1 and chunks_filtered != 0, m["plan"]
    assert m["st"].frames == 1
    assert ST.same_bits(m["color"], m["plain_color"]) and ST.same_bits(m["radii"], m["plain_radii"])


def test_multi_chunk_weight_sum_is_the_colour_gradient_and_totals_the_alpha_map():
    m = _multi_chunk()
    got, want = m["st"].weight_sum.cpu().numpy(), m["grad"]
    bound = GRAD_ATOL_REL * np.abs(want).max() + GRAD_RTOL * np.abs(want)
    ratio = (np.abs(got - want) / bound).max()
    total, alpha_sum = float(got.sum()), m["alpha_sum"]
    print(f"multi-chunk: {int((want != 0).sum())} of {want.size} Gaussians composited; weight_sum vs colour gradient worst err / bound "
          f"{ratio:.3f}; sum of weight_sum {total:.4f} vs alpha.sum() {alpha_sum:.4f} (|delta| {abs(total - alpha_sum):.3e}, bound "
          f"{1e-5 * m['W'] * m['H']:.3e})")
    assert (want != 0).sum() > 1000
    assert ratio <= 1.0
    assert abs(total - alpha_sum) <= 1e-5 * m["W"] * m["H"]
    np.testing.assert_array_equal(m["st"].count.cpu().numpy() > 0, want != 0)
    assert ((m["st"].count > 0) == (m["st"].weight_max > 0)).all()


def test_a_frame_that_outgrows_its_first_workspace_is_added_once():
    """The first attempt of this frame (no workspace guess yet) sizes the binning workspace for the first chunk, blends it - adding
    its statistics - and stops with GSR_ERR_WORKSPACE in front of a later chunk; the re-run must not add the first chunk again."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    m = _multi_chunk()
    errors, orig = [], N.forward_render

    def spy(*a, **k):
        try:
            return orig(*a, **k)
        except N.GsrError as e:
            errors.append(e.status)
            raise
    dgr._binning_guess.clear()
    N.forward_render = spy
    try:
        st = _stats_frame(m["kw"])[2]
        first = list(errors)
        before = {k: v.clone() for k, v in _bits(st).items()}
        dgr._binning_guess.clear()
        _stats_frame(m["kw"], stats=st)
    finally:
        N.forward_render = orig
    dgr._binning_guess.clear()
    assert first == [N.ERR_WORKSPACE] and errors == [N.ERR_WORKSPACE] * 2, errors
    assert _same_stats(_multi_chunk()["st"], type("S", (), before)) and st.frames == 2
    assert torch.equal(st.count, 2 * before["count"]) and torch.equal(st.weight_sum_q32, 2 * before["weight_sum_q32"])
    assert ST.same_bits(st.weight_max, before["weight_max"])


def test_one_call_forward_equals_the_two_stage_frame():
    """gsr_forward_contrib (both stages in one call) on a workspace that holds every instance: the two-stage frame's statistics."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    kw = _reference(4)[0]
    inp = _inputs(kw, False)
    P = inp["means3D"].shape[0]
    want = _new_stats(P)
    color, radii, fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None,
                                             _settings(kw), contrib=want)
    R = fr.R
    got = _new_stats(P)
    tiles = ((kw["image_width"] + 15) // 16) * ((kw["image_height"] + 15) // 16)
    with torch.cuda.device(DEV):
        binning = torch.empty(dgr._binning_bytes(R, tiles), dtype=torch.uint8, device=DEV)
        color2, radii2 = torch.empty_like(color), torch.empty_like(radii)
        plan, done = N.forward_both(fr.desc, fr.cam, fr.gauss, torch.empty_like(fr.geom_ws), torch.empty_like(fr.image_ws), radii2, binning, R,
                                    color2, torch.device(DEV), contrib=got.native())
    torch.cuda.synchronize()
    assert done and int(plan.num_rendered) == R
    assert _same_stats(got, want) and ST.same_bits(color2, color) and ST.same_bits(radii2, radii)
    assert int(want.count.sum()) > 0


# ---- bits ------------------------------------------------------------------------------------------------------------------------

def _two_cameras():
    W, H = 128, 96
    scene = S.make_scene(3000, W, H, 2, 31, scale_lo=0.005, scale_hi=0.06)
    return [raster_kwargs(scene, cam, bg=(0.1, 0.2, 0.3)) for cam in S.arc_cameras(W, H, 2)]


def test_two_runs_give_equal_bits():
    for kw in (_reference(4)[0], _multi_chunk()["kw"]):
        a, b = _stats_frame(kw)[2], _stats_frame(kw)[2]
        assert int(a.count.sum()) > 0 and _same_stats(a, b)
    assert _same_stats(_stats_frame(_multi_chunk()["kw"])[2], _multi_chunk()["st"])


def test_accumulating_two_cameras_is_the_sum_and_the_maximum():
    kw_a, kw_b = _two_cameras()
    a, b = _stats_frame(kw_a)[2], _stats_frame(kw_b)[2]
    both = _stats_frame(kw_b, stats=_stats_frame(kw_a)[2])[2]
    swapped = _stats_frame(kw_a, stats=_stats_frame(kw_b)[2])[2]
    assert both.frames == 2 and int(a.count.sum()) > 0 and int(b.count.sum()) > 0 and not torch.equal(a.count, b.count)
    assert torch.equal(both.count, a.count + b.count)
    assert torch.equal(both.weight_sum_q32, a.weight_sum_q32 + b.weight_sum_q32)
    assert ST.same_bits(both.weight_max, torch.maximum(a.weight_max, b.weight_max))
    assert _same_stats(both, swapped)
    both.reset()
    assert both.frames == 0 and not both.count.any() and not both.weight_sum_q32.any() and not both.weight_max.any()


# ---- layers ----------------------------------------------------------------------------------------------------------------------

def _model(P=3000, W=128, H=96, D=2, seed=33, opt=None):
    from scene import GaussianModel
    scene = S.make_scene(P, W, H, D, seed, scale_lo=0.005, scale_hi=0.06)
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    if opt is not None:
        gm.training_setup(opt)
    return gm, [c.to(DEV) for c in S.arc_cameras(W, H, 3)]


def _render_frame(gm, cam, P, **flags):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    pipe = Pipe()
    for k, v in flags.items():
        setattr(pipe, k, v)
    st = _new_stats(P)
    out = render(cam, gm, pipe, torch.zeros(3, device=DEV), contributions=st)
    assert not out["render"].requires_grad and st.frames == 1
    return out, st


def _direct_frames(gm, cam, antialiasing=False):
    """The two frames render() hands to the rasterizer, called directly: forward_raw on the raw leaves, forward on the getters."""
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    P = gm.get_xyz.shape[0]
    rs = GaussianRasterizationSettings(int(cam.image_height), int(cam.image_width), math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                       torch.zeros(3, device=DEV), 1.0, cam.world_view_transform, cam.full_proj_transform, gm.active_sh_degree,
                                       cam.camera_center, False, False)
    raw, get = _new_stats(P), _new_stats(P)
    z = torch.zeros(P, 3, device=DEV)
    with torch.no_grad():
        GaussianRasterizer(rs, antialiasing=antialiasing, contributions=raw).forward_raw(gm._xyz, z, gm._features, None, gm._opacity, gm._scaling,
                                                                                        gm._rotation)
        GaussianRasterizer(rs, antialiasing=antialiasing, contributions=get)(means3D=gm.get_xyz, means2D=z, shs=gm.get_features,
                                                                             opacities=gm.get_opacity, scales=gm.get_scaling,
                                                                             rotations=gm.get_rotation)
    return raw, get


def test_render_passes_contributions_through_and_antialiasing_changes_them():
    """render(..., contributions=) adds exactly what the rasterizer adds when it is called with the getters' tensors, and returns the
    getter path's frame, under either setting of pipe.fused_activations (a statistics frame always takes the getters: next test).
    The rasterizer itself takes contributions on forward_raw too: that frame differs from the getters' in the last bit of the
    activations, so its statistics are held to the getters' by the rule test_gpu_parity._raw_mode_vs_getters has for the two paths -
    counts equal but for flipped decisions, sums by the gradient rule, maxima by the pixel rule."""
    from gaussian_params import Pipe
    from gaussian_renderer import render
    gm, cams = _model()
    bg = torch.zeros(3, device=DEV)
    P = gm.get_xyz.shape[0]
    (fused_out, fused), (get_out, get) = _render_frame(gm, cams[0], P), _render_frame(gm, cams[0], P, fused_activations=False)
    getters_pipe = Pipe()
    getters_pipe.fused_activations = False
    with torch.no_grad():
        plain = render(cams[0], gm, getters_pipe, bg)
    for out in (fused_out, get_out):
        assert ST.same_bits(out["render"], plain["render"]) and ST.same_bits(out["radii"], plain["radii"])
    direct_raw, direct_get = _direct_frames(gm, cams[0])
    assert int(get.count.sum()) > 0 and _same_stats(get, direct_get) and _same_stats(fused, direct_get)
    a, b = direct_raw.weight_sum, direct_get.weight_sum
    bad_rows = (a - b).abs() > 2e-5 * float(a.max()) + 2e-3 * a
    d_max = (direct_raw.weight_max - direct_get.weight_max).abs()
    print(f"forward_raw vs forward: count differs on {int((direct_raw.count != direct_get.count).sum())} of {P} Gaussians, weight_sum on "
          f"{int(bad_rows.sum())} rows beyond the gradient rule (worst relative {float(((a - b).abs() / a.clamp_min(1e-30)).max()):.3e}), "
          f"weight_max by {float(d_max.max()):.3e} at most")
    assert int(direct_raw.count.sum()) > 0
    assert float(bad_rows.double().mean()) <= 2e-4
    assert float((d_max > 2e-5).double().mean()) <= 1e-4 and float(d_max.max()) <= 8e-3
    assert float((direct_raw.count != direct_get.count).double().mean()) <= 2e-4
    (_, aa_fused), (_, aa_get) = _render_frame(gm, cams[0], P, antialiasing=True), _render_frame(gm, cams[0], P, antialiasing=True, fused_activations=False)
    aa_direct_raw, aa_direct_get = _direct_frames(gm, cams[0], antialiasing=True)
    assert _same_stats(aa_get, aa_direct_get) and _same_stats(aa_fused, aa_direct_get)
    for plain_st, aa_st in ((get, aa_get), (direct_raw, aa_direct_raw)):
        assert not torch.equal(aa_st.weight_sum_q32, plain_st.weight_sum_q32) and not torch.equal(aa_st.count, plain_st.count)
        assert int(aa_st.weight_sum_q32.sum()) < int(plain_st.weight_sum_q32.sum())          # the compensation only lowers opacities
    # debug=True: the same frame, synchronised
    assert _same_stats(_stats_frame(_reference(4)[0], debug=True)[2], _stats_frame(_reference(4)[0])[2])
    with pytest.raises(ValueError, match="contributions"):
        render(cams[0], gm, Pipe(), bg, depth_alpha=True, contributions=_new_stats(P))
    with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
        _stats_frame_with_grad(_reference(4)[0])


def test_render_raw_and_getter_paths_give_equal_statistics():
    """render(..., contributions=) under pipe.fused_activations unset / True (the raw path of any other frame) and False (the getter
    path) gives EQUAL statistics, bit for bit, for this package's model and for a store with torch getters: a statistics frame takes
    the getters under either setting.  (Rendered through forward_raw the frame itself differs in the last bit - the activations run
    in the preprocess kernel there - and so would the sums: measured on this model, weight_sum_q32 on 1 694 of 3 000 Gaussians, by
    1.0e-5 relative at most, count on none.)"""
    from gaussian_params import GaussianParams
    gm, cams = _model()
    P = gm.get_xyz.shape[0]
    store = GaussianParams(S.make_scene(P, 128, 96, 2, 33, scale_lo=0.005, scale_hi=0.06).to(DEV), max_sh_degree=2).to(DEV)
    store.active_sh_degree = 2
    for model in (gm, store):
        (_, unset), (_, fused), (_, get) = (_render_frame(model, cams[0], P), _render_frame(model, cams[0], P, fused_activations=True),
                                            _render_frame(model, cams[0], P, fused_activations=False))
        assert int(get.count.sum()) > 0
        assert torch.equal(unset.count, get.count) and torch.equal(fused.count, get.count)
        assert _same_stats(unset, get) and _same_stats(fused, get)


def _stats_frame_with_grad(kw):
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, True)
    P = inp["means3D"].shape[0]
    return GaussianRasterizer(_settings(kw), contributions=_new_stats(P))(means2D=torch.zeros(P, 3, device=DEV), **inp)


def test_model_statistics_over_three_cameras_then_prune_the_lower_half():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import OptimizationDefaults
    gm, cams = _model(opt=OptimizationDefaults())
    P = gm.get_xyz.shape[0]
    stats = gm.contribution_stats(cams)
    assert stats.frames == 3 and stats.P == P
    one = [_new_stats(P) for _ in cams]
    bg = torch.zeros(3, device=DEV)
    for st, cam in zip(one, cams):
        render(cam, gm, Pipe(), bg, contributions=st)
    assert torch.equal(stats.count, sum(s.count for s in one)) and torch.equal(stats.weight_sum_q32, sum(s.weight_sum_q32 for s in one))
    scores = gm.significance(stats)
    assert scores.dtype == torch.float64 and scores.shape == (P,) and int((scores > 0).sum()) > P // 4
    tag = gm.get_xyz.detach().clone()
    order = torch.sort(scores, stable=True).indices
    assert gm.prune_by_significance(scores, fraction=0.5) == P // 2
    keep = torch.ones(P, dtype=torch.bool, device=DEV)
    keep[order[:P // 2]] = False
    assert torch.equal(gm.get_xyz.detach(), tag[keep])
    assert float(scores[keep].min()) >= float(scores[~keep].max())
    with torch.no_grad():
        out = render(cams[0], gm, Pipe(), bg)
    assert out["radii"].shape[0] == P - P // 2 and torch.isfinite(out["render"]).all() and int((out["radii"] > 0).sum()) > 0


def _training_fixture():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    W = H = 64
    cams = [c.to(DEV) for c in S.arc_cameras(W, H, 4)]
    scene = S.make_scene(2000, W, H, 2, 30, scale_lo=0.01, scale_hi=0.08)
    truth = GaussianModel(2)
    truth.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    start = S.make_scene(2000, W, H, 2, 31, scale_lo=0.01, scale_hi=0.08)
    return start, cams, targets, bg


def _fresh(scene, opt):
    from scene import GaussianModel
    gm = GaussianModel(2)
    gm.adopt_scene(scene, device=DEV)
    gm.training_setup(opt)
    return gm


@pytest.mark.parametrize("filter_3d", (False, True), ids=("plain", "filter_3d"))
def test_training_loop_prunes_by_significance_at_the_listed_iterations(filter_3d):
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, cams, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), densify_from_iter=10 ** 9, densify_until_iter=0, significance_prune_iterations=(20, 30),
                  filter_3d=filter_3d)
    gm = _fresh(scene, opt)
    sizes, losses = {}, []
    random.seed(1)
    torch.manual_seed(1)

    def note(it, loss, g):
        sizes[it] = g.get_xyz.shape[0]
        losses.append(float(loss.detach()))
    train(gm, cams, targets, opt, Pipe(), bg, iterations=40, scene_extent=3.0, on_iteration=note)
    p1 = 2000 - math.floor(opt.significance_prune_fraction * 2000)
    p2 = p1 - math.floor(opt.significance_prune_fraction * opt.significance_prune_decay * p1)
    assert (p1, p2) == (800, 512)
    assert len(losses) == 40 and all(np.isfinite(losses))
    assert all(sizes[it] == 2000 for it in range(1, 20)) and all(sizes[it] == p1 for it in range(20, 30))
    assert all(sizes[it] == p2 for it in range(30, 41))
    for g in gm.optimizer.param_groups:
        for p in g["params"]:
            assert p.shape[0] == p2 and gm.optimizer.state[p]["exp_avg"].shape == p.shape
    assert (gm.filter_3D is not None and gm.filter_3D.shape[0] == p2) if filter_3d else gm.filter_3D is None


def _parent_loop(gaussians, cameras, targets, opt, pipe, background, iterations, scene_extent):
    """train_loop.train as it stood before the significance options, for the default strategy without grids or filters."""
    from gaussian_renderer import render
    from loss_utils import training_loss
    stack = []
    for it in range(1, iterations + 1):
        gaussians.update_learning_rate(it)
        if it % 1000 == 0:
            gaussians.oneupSHdegree()
        if not stack:
            stack = list(range(len(cameras)))
        idx = stack.pop(random.randint(0, len(stack) - 1))
        pkg = render(cameras[idx], gaussians, pipe, background)
        loss = training_loss(pkg["render"], targets[idx], opt.lambda_dssim)
        loss.backward()
        with torch.no_grad():
            if it < opt.densify_until_iter:
                gaussians.update_densification_stats(pkg["viewspace_points"], pkg["radii"])
                if it > opt.densify_from_iter and it % opt.densification_interval == 0:
                    gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, scene_extent, 20 if it > opt.opacity_reset_interval else None)
                if it % opt.opacity_reset_interval == 0:
                    gaussians.reset_opacity()
            if it < iterations:
                gaussians.optimizer.step()
                gaussians.optimizer.zero_grad(set_to_none=True)
    return gaussians


def test_without_listed_iterations_the_loop_is_the_parents_bit_for_bit():
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, cams, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), densify_from_iter=10, densification_interval=10, densify_until_iter=35, densify_grad_threshold=1e-5)
    assert opt.significance_prune_iterations == ()
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
