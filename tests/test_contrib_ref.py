"""CPU checks of the blend statistics (diff_gaussian_rasterization.contrib): the float64 reference the GPU tests
use (tests/contrib_ref.py) is anchored to the oracle's own image; the C ABI is additive (two symbols declared, exported and in
EXPORTS, the struct mirrored, the version unchanged) and refuses what it must without touching a device; and the host logic - scores,
pruning, options, the loop's and the rasterizer's refusals - on CPU tensors with hand-made statistics."""
import ctypes as C
import os
import re
from dataclasses import replace

import numpy as np
import pytest
import torch

import contrib_ref as CR
import oracle
import scene_synth as S
from scene import GaussianModel, OptimizationDefaults
from test_gpu_parity import FIXTURES, _fixture_id, _fixture_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_forward_contrib", "gsr_forward_render_contrib")
CONTRIB_FIXTURES = [FIXTURES[i] for i in (0, 2, 4, 6, 9, 11, 13)]


# ---- the reference ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("c", CONTRIB_FIXTURES, ids=_fixture_id)
def test_reference_walk_reproduces_the_oracles_image(c):
    kw = _fixture_kwargs(c)
    fr = oracle.rasterize(dtype=np.float64, **kw)
    count, wsum, wmax, px_w, px_c = CR.contributions(fr, per_pixel=True)
    bg = np.asarray(kw["bg"], np.float64).reshape(3, 1, 1)
    assert np.abs(px_w - (1.0 - fr.final_T)).max() <= 1e-12
    assert np.abs(px_c + fr.final_T[None] * bg - fr.color).max() <= 1e-12
    # the three statistics hang together: every composited pixel adds at least alpha_min T_cutoff and at most 0.99
    assert count.sum() > 0 and ((count > 0) == (wsum > 0)).all() and ((count > 0) == (wmax > 0)).all()
    assert (wmax <= 0.99).all() and (wsum <= count * wmax + 1e-12).all() and (wsum >= wmax).all()
    assert abs(wsum.sum() - px_w.sum()) <= 1e-9 * max(px_w.sum(), 1.0)
    assert (count[fr.radii == 0] == 0).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_contrib_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert "gsr_contrib_stats" in hdr
    assert [f for f, _ in native.ContribStats._fields_] == ["count", "weight_sum_q32", "weight_max_bits"]
    assert lib.gsr_version() == 12
    assert re.search(r"#define\s+GSR_VERSION\s+12\b", hdr)


def _render_contrib(native, desc, stats, gauss=None):
    lib = native.load()
    cam = native.Camera(1, 1, 1, 1)
    g = native.Gaussians(1, 1, None, 1, 1, 1, None) if gauss is None else gauss
    one = C.c_void_p(1)
    plan = native.FramePlan()
    plan.num_rendered, plan.num_chunks = 10, 1
    rc = lib.gsr_forward_render_contrib(C.byref(desc), C.byref(cam), C.byref(g), one, one, one, C.byref(plan), one,
                                        None if stats is None else C.byref(stats), None)
    return rc, lib.gsr_last_error()


def _forward_contrib(native, desc, stats, gauss=None):
    lib = native.load()
    cam = native.Camera(1, 1, 1, 1)
    g = native.Gaussians(1, 1, None, 1, 1, 1, None) if gauss is None else gauss
    one = C.c_void_p(1)
    plan = native.FramePlan()
    rc = lib.gsr_forward_contrib(C.byref(desc), C.byref(cam), C.byref(g), one, one, one, C.byref(plan), one, C.c_int64(10), one, None,
                                 None if stats is None else C.byref(stats), None)
    return rc, lib.gsr_last_error()


def test_null_members_and_slabs_are_refused_without_a_device(native):
    """Every case is refused on the host: the pointers are the address 1, and nothing here has a device to dereference them on."""
    whole = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3))
    full = native.ContribStats(1, 1, 1)
    for call in (_render_contrib, _forward_contrib):
        for k in range(3):
            members = [1, 1, 1]
            members[k] = None
            rc, msg = call(native, whole, native.ContribStats(*members))
            assert rc == -1 and b"weight_sum_q32" in msg and b"required" in msg, (call.__name__, k, rc, msg)
        rc, msg = call(native, slab, full)
        assert rc == -1 and b"whole images" in msg, (call.__name__, rc, msg)
    # P = 0: there is nothing to accumulate into, NULL members are fine (the call then fails on the plain call's own grounds or not at all)
    empty = native.make_desc(0, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3))
    rc, msg = _render_contrib(native, empty, native.ContribStats(None, None, None))
    assert rc == -1 and b"whole images" in msg


def test_null_stats_is_the_plain_call_without_gpu(native):
    """stats = NULL takes the plain calls' path: on arguments they reject, the new entry points return the same status and message
    (a slab included: the plain calls render slabs)."""
    lib = native.load()
    no_colour = native.Gaussians(1, None, None, 1, 1, 1, None)
    cam = native.Camera(1, 1, 1, 1)
    one = C.c_void_p(1)
    for d in (native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3)),
              native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)):
        plan = native.FramePlan()
        plan.num_rendered, plan.num_chunks = 10, 1
        rc0 = lib.gsr_forward_render(C.byref(d), C.byref(cam), C.byref(no_colour), one, one, one, C.byref(plan), one, None)
        msg0 = lib.gsr_last_error()
        rc1, msg1 = _render_contrib(native, d, None, no_colour)
        assert rc0 < 0 and (rc0, msg0) == (rc1, msg1), (rc0, msg0, rc1, msg1)
        rc0 = lib.gsr_forward(C.byref(d), C.byref(cam), C.byref(no_colour), one, one, one, C.byref(plan), one, C.c_int64(10), one, None, None)
        msg0 = lib.gsr_last_error()
        rc1, msg1 = _forward_contrib(native, d, None, no_colour)
        assert rc0 < 0 and (rc0, msg0) == (rc1, msg1), (rc0, msg0, rc1, msg1)


# ---- host logic ------------------------------------------------------------------------------------------------------------------

def _model(P=200, D=1, seed=7):
    gm = GaussianModel(D)
    gm.adopt_scene(S.make_scene(P, 64, 64, D, seed), device="cpu")
    gm.training_setup(OptimizationDefaults())
    return gm


def _stats(P, seed=3):
    from diff_gaussian_rasterization.contrib import ContributionStats
    st = ContributionStats(P, "cpu")
    g = torch.Generator().manual_seed(seed)
    st.count[:] = torch.randint(0, 5000, (P,), generator=g)
    st.weight_sum_q32[:] = torch.randint(0, 2 ** 44, (P,), generator=g)
    st.weight_max[:] = torch.rand(P, generator=g) * 0.99
    st.frames = 3
    return st


def test_contribution_stats_object():
    from diff_gaussian_rasterization.contrib import ContributionStats
    st = ContributionStats(5, "cpu")
    assert (st.count.dtype, st.weight_sum_q32.dtype, st.weight_max.dtype) == (torch.int64, torch.int64, torch.float32)
    assert all(t.shape == (5,) and not t.any() for t in (st.count, st.weight_sum_q32, st.weight_max)) and st.frames == 0
    st.weight_sum_q32[1] = 3 * 2 ** 32 + 2 ** 31
    st.weight_sum_q32[2] = 1
    assert st.weight_sum.dtype == torch.float64
    assert st.weight_sum.tolist() == [0.0, 3.5, 2.0 ** -32, 0.0, 0.0]
    st.count[0], st.weight_max[3], st.frames = 7, 0.5, 2
    st.reset()
    assert all(not t.any() for t in (st.count, st.weight_sum_q32, st.weight_max)) and st.frames == 0
    n = st.native()
    assert n.count == st.count.data_ptr() and n.weight_sum_q32 == st.weight_sum_q32.data_ptr() and n.weight_max_bits == st.weight_max.data_ptr()


def test_the_three_scores_and_the_reference_volume():
    P = 200
    gm, st = _model(P), _stats(P)
    assert torch.equal(gm.significance(st, "weight_sum"), st.weight_sum_q32.double() * 2.0 ** -32)
    assert torch.equal(gm.significance(st, "weight_max"), st.weight_max.double())
    V = gm.get_scaling.detach().double().prod(1)
    order = np.argsort(-V.numpy(), kind="stable")
    V_ref = V[order[int(0.9 * P)]]
    assert int((V > V_ref).sum()) == int(0.9 * P)                    # (distinct volumes: exactly 180 of 200 are larger)
    for v_pow in (0.1, 0.5):
        want = st.weight_sum * (V / V_ref) ** v_pow
        got = gm.significance(st, "volume_weighted", v_pow=v_pow)
        assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=1e-14, atol=0)
    assert torch.equal(gm.significance(st), gm.significance(st, "volume_weighted", 0.1))
    with pytest.raises(ValueError, match="score"):
        gm.significance(st, "opacity")
    with pytest.raises(ValueError, match="200"):
        gm.significance(_stats(199))


def test_fraction_threshold_ties_and_exactly_one_of_them():
    P = 10
    scores = torch.tensor([5.0, 1.0, 3.0, 1.0, 9.0, 1.0, 3.0, 0.0, 7.0, 1.0], dtype=torch.float64)
    gm = _model(P)
    tag = gm._xyz.detach().clone()
    for bad in (dict(), dict(fraction=0.5, threshold=1.0)):
        with pytest.raises(ValueError, match="exactly one"):
            gm.prune_by_significance(scores, **bad)
    with pytest.raises(ValueError, match="scores"):
        gm.prune_by_significance(scores[:9], fraction=0.5)
    # floor(0.35 * 10) = 3 lowest: the 0, then the FIRST two of the four tied 1s (indices 1, 3)
    assert gm.prune_by_significance(scores, fraction=0.35) == 3
    keep = [0, 2, 4, 5, 6, 8, 9]
    assert torch.equal(gm._xyz.detach(), tag[keep])
    gm = _model(P)
    assert gm.prune_by_significance(scores, threshold=3.0) == 5          # strictly below: the 3s stay
    assert torch.equal(gm._xyz.detach(), tag[[0, 2, 4, 6, 8]])
    gm = _model(P)
    assert gm.prune_by_significance(scores, fraction=0.0) == 0 and gm._xyz.shape[0] == P
    assert gm.prune_by_significance(scores, fraction=0.09) == 0 and gm._xyz.shape[0] == P      # floor(0.9) = 0
    assert gm.prune_by_significance(scores, fraction=1.0) == P and gm._xyz.shape[0] == 0


def test_adam_moments_and_densification_statistics_follow_the_kept_rows():
    torch.manual_seed(0)
    P = 120
    gm, st = _model(P), _stats(P)
    groups = [g for g in gm.optimizer.param_groups if g["params"]]
    for g in groups:
        g["params"][0].grad = torch.randn_like(g["params"][0])
    gm.optimizer.step()
    gm.denom[:] = torch.arange(P, dtype=torch.float32)[:, None]
    gm.xyz_gradient_accum[:] = torch.arange(P, dtype=torch.float32)[:, None] * 0.5
    gm.max_radii2D[:] = torch.arange(P, dtype=torch.float32) + 1
    gm.filter_3D = torch.ones(P, 1)
    before = {g["name"]: (g["params"][0].detach().clone(), gm.optimizer.state[g["params"][0]]["exp_avg"].clone(),
                          gm.optimizer.state[g["params"][0]]["exp_avg_sq"].clone()) for g in groups}
    scores = gm.significance(st, "weight_sum")
    n = gm.prune_by_significance(scores, fraction=0.5)
    assert n == 60 and gm._xyz.shape[0] == 60
    keep = torch.ones(P, dtype=torch.bool)
    keep[torch.sort(scores, stable=True).indices[:60]] = False
    assert float(scores[keep].min()) >= float(scores[~keep].max())       # the survivors are the top half
    for g in groups:
        p = g["params"][0]
        param, m, v = before[g["name"]]
        assert torch.equal(p.detach(), param[keep]), g["name"]
        assert torch.equal(gm.optimizer.state[p]["exp_avg"], m[keep]) and torch.equal(gm.optimizer.state[p]["exp_avg_sq"], v[keep]), g["name"]
    idx = torch.nonzero(keep)[:, 0].float()
    assert torch.equal(gm.denom[:, 0], idx) and torch.equal(gm.xyz_gradient_accum[:, 0], idx * 0.5) and torch.equal(gm.max_radii2D, idx + 1)
    with pytest.raises(ValueError, match="compute_3D_filter"):          # the 3D filter went stale, as after any structural edit
        gm.checked_filter_3D()


def test_option_defaults():
    d = OptimizationDefaults()
    assert d.significance_prune_iterations == () and d.significance_prune_fraction == 0.6
    assert d.significance_prune_decay == 0.6 and d.significance_prune_score == "volume_weighted"


def test_train_refuses_significance_pruning_with_mcmc():
    from train_loop import train
    gm = _model(50)
    opt = replace(OptimizationDefaults(), densify_strategy="mcmc", significance_prune_iterations=(5,))
    with pytest.raises(ValueError, match="mcmc"):
        train(gm, [], [], opt, None, torch.zeros(3), iterations=10)


def _settings(requires_grad=False):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(32, 32, .5, .5, torch.zeros(3), 1.0, torch.eye(4).requires_grad_(requires_grad), torch.eye(4), 0,
                                             torch.zeros(3), False, False)


def test_rasterizer_refusals_that_need_no_device():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization.contrib import ContributionStats
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    st = ContributionStats(4, "cpu")
    for kw in (dict(depth_alpha=True), dict(absgrad=True)):
        with pytest.raises(ValueError, match="contributions"):
            dgr.GaussianRasterizer(_settings(), contributions=st, **kw)
    with pytest.raises(ValueError, match="ContributionStats"):
        dgr.GaussianRasterizer(_settings(), contributions=torch.zeros(4))
    z = torch.zeros(4, 3)
    args = dict(means3D=z, means2D=z, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=z, rotations=torch.zeros(4, 4))
    r = dgr.GaussianRasterizer(_settings(), contributions=ContributionStats(5, "cpu"))
    with pytest.raises(ValueError, match="5 Gaussians"):
        r(**args)
    with pytest.raises(ValueError, match="5 Gaussians"):
        r.forward_raw(z, z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4))
    r = dgr.GaussianRasterizer(_settings(), contributions=st)
    for name in ("means3D", "opacities", "shs", "scales", "rotations"):
        with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
            r(**{**args, name: args[name].clone().requires_grad_(True)})
    with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
        dgr.GaussianRasterizer(_settings(requires_grad=True), contributions=st)(**args)
    with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
        r.forward_raw(z.clone().requires_grad_(True), z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4))
    # host tensors keep the error they always had, with and without grad mode
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(**args)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU path"):
        r(**{**args, "means3D": z.clone().requires_grad_(True)})
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="lives on"):
            dgr.GaussianRasterizer(_settings(), contributions=ContributionStats(4, "cuda:0"))(**args)
    # the low-level entry point: slabs and aux
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, _settings(), tile_rows=(0, 1),
                              contrib=st)
    with pytest.raises(ValueError, match="depth_alpha"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, _settings(), aux=True, contrib=st)
    sharded = ShardedRenderer.__new__(ShardedRenderer)
    with pytest.raises(ValueError, match="ShardedRenderer"):
        sharded.render(None, None, None, torch.zeros(3), contributions=st)
    with pytest.raises(ValueError, match="ShardedRenderer"):
        sharded.rasterize(_settings(), contributions=st, **args)
