"""CPU checks of the error-weighted blend statistics (diff_gaussian_rasterization.contrib.ErrorStats): the float64
reference the GPU tests use (tests/contrib_error_ref.py) is anchored to the oracle's own transmittance and to tests/contrib_ref.py; the
C ABI is additive (three symbols declared, exported and in EXPORTS, the struct mirrored, the version unchanged) and refuses what it
must without touching a device; and the host logic - the error map, the budgeted selection, the options, the loop's and the
rasterizer's refusals - on CPU tensors."""
import ctypes as C
import functools
import os
import re
from dataclasses import replace

import numpy as np
import pytest
import torch

import contrib_error_ref as ER
import contrib_ref as CR
import oracle
import scene_synth as S
from scene import GaussianModel, OptimizationDefaults
from test_contrib_ref import CONTRIB_FIXTURES, _forward_contrib, _render_contrib
from test_gpu_parity import _fixture_id, _fixture_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_forward_contrib_error", "gsr_forward_render_contrib_error", "gsr_contrib_error_fold")


# ---- the reference ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _frame(k):
    kw = _fixture_kwargs(CONTRIB_FIXTURES[k])
    return kw, oracle.rasterize(dtype=np.float64, **kw)


@pytest.mark.parametrize("k", range(len(CONTRIB_FIXTURES)), ids=lambda k: _fixture_id(CONTRIB_FIXTURES[k]))
def test_reference_anchors(k):
    kw, fr = _frame(k)
    E = np.random.default_rng(100 + k).random((fr.H, fr.W))
    E[::7, ::5] = -3.0
    E[1::9, 2::4] = 7.0
    E[3::11, ::6] = np.nan
    Ec = ER.clamp_map(E)
    assert Ec.min() == 0.0 and Ec.max() == 1.0 and np.isfinite(Ec).all()
    esum, final_T = ER.error_sums(fr, E)
    assert np.abs(final_T - fr.final_T).max() <= 1e-12
    total = float((Ec * (1.0 - fr.final_T)).sum())
    assert total > 0 and abs(esum.sum() - total) <= 1e-9 * total
    ones, _ = ER.error_sums(fr, np.ones((fr.H, fr.W)))
    wsum = CR.contributions(fr)[1]
    assert np.abs(ones - wsum).max() <= 1e-12 * max(wsum.max(), 1.0)
    # values above 1 read as 1, negatives and NaN as 0
    assert np.array_equal(ER.error_sums(fr, np.full((fr.H, fr.W), 7.0))[0], ones)
    for v in (0.0, -3.0, np.nan):
        assert not ER.error_sums(fr, np.full((fr.H, fr.W), v))[0].any()
    assert (esum <= ones + 1e-15).all() and ((esum > 0) <= (ones > 0)).all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_error_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert "gsr_contrib_error" in hdr
    assert [f for f, _ in native.ContribError._fields_] == ["pixel_error", "error_frame_q32"]
    assert lib.gsr_version() == 12
    assert re.search(r"#define\s+GSR_VERSION\s+12\b", hdr)
    assert [f for f, _ in native.ContribStats._fields_] == ["count", "weight_sum_q32", "weight_max_bits"]


def _render_error(native, desc, stats, err, gauss=None):
    lib = native.load()
    cam = native.Camera(1, 1, 1, 1)
    g = native.Gaussians(1, 1, None, 1, 1, 1, None) if gauss is None else gauss
    one = C.c_void_p(1)
    plan = native.FramePlan()
    plan.num_rendered, plan.num_chunks = 10, 1
    rc = lib.gsr_forward_render_contrib_error(C.byref(desc), C.byref(cam), C.byref(g), one, one, one, C.byref(plan), one,
                                              None if stats is None else C.byref(stats), None if err is None else C.byref(err), None)
    return rc, lib.gsr_last_error()


def _forward_error(native, desc, stats, err, gauss=None):
    lib = native.load()
    cam = native.Camera(1, 1, 1, 1)
    g = native.Gaussians(1, 1, None, 1, 1, 1, None) if gauss is None else gauss
    one = C.c_void_p(1)
    plan = native.FramePlan()
    rc = lib.gsr_forward_contrib_error(C.byref(desc), C.byref(cam), C.byref(g), one, one, one, C.byref(plan), one, C.c_int64(10), one, None,
                                       None if stats is None else C.byref(stats), None if err is None else C.byref(err), None)
    return rc, lib.gsr_last_error()


def test_every_refusal_comes_back_without_a_device(native):
    """Every case is refused on the host: the pointers are the address 1, and nothing here has a device to dereference them on."""
    whole = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3))
    stats, err = native.ContribStats(1, 1, 1), native.ContribError(1, 1)
    for call in (_render_error, _forward_error):
        rc, msg = call(native, whole, None, err)
        assert rc == -1 and b"stats" in msg and b"required" in msg, (call.__name__, rc, msg)
        rc, msg = call(native, whole, stats, native.ContribError(None, 1))
        assert rc == -1 and b"pixel_error" in msg and b"required" in msg, (call.__name__, rc, msg)
        rc, msg = call(native, whole, stats, native.ContribError(1, None))
        assert rc == -1 and b"error_frame_q32" in msg and b"required" in msg, (call.__name__, rc, msg)
        rc, msg = call(native, slab, stats, err)
        assert rc == -1 and b"whole images" in msg, (call.__name__, rc, msg)
        # the statistics' own members are still asked for
        rc, msg = call(native, whole, native.ContribStats(1, None, 1), err)
        assert rc == -1 and b"weight_sum_q32" in msg and b"required" in msg, (call.__name__, rc, msg)
    # P = 0: there is nothing to accumulate into and no splat to weight, NULL members are not what gets such a call refused (that
    # it is then carried out without reading a map needs a device: tests/test_gpu_contrib_error.py) - the other refusals stand
    empty_slab = native.make_desc(0, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3))
    empty = native.make_desc(0, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    for call in (_render_error, _forward_error):
        rc, msg = call(native, empty_slab, native.ContribStats(None, None, None), native.ContribError(None, None))
        assert rc == -1 and b"whole images" in msg and b"required" not in msg, (call.__name__, rc, msg)
        rc, msg = call(native, empty, None, native.ContribError(None, None))
        assert rc == -1 and b"stats" in msg and b"required" in msg, (call.__name__, rc, msg)
    lib = native.load()
    one = C.c_void_p(1)
    assert lib.gsr_contrib_error_fold(C.c_int64(-1), one, one, one, None) == -1 and b"P = -1" in lib.gsr_last_error()
    for k in range(3):
        ptrs = [one, one, one]
        ptrs[k] = None
        assert lib.gsr_contrib_error_fold(C.c_int64(5), *ptrs, None) == -1
        assert b"error_sum_q32" in lib.gsr_last_error() and b"required" in lib.gsr_last_error()
    assert lib.gsr_contrib_error_fold(C.c_int64(0), None, None, None, None) == 0          # nothing to fold: no launch


def test_null_err_is_the_contrib_call_without_gpu(native):
    """err = NULL takes the _contrib calls' path: on arguments they reject, the same status and message - their own refusals (which
    name the _contrib call) and the plain calls' behind them."""
    whole = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(1, 3))
    bad_degree = native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)
    no_colour = native.Gaussians(1, None, None, 1, 1, 1, None)
    full = native.ContribStats(1, 1, 1)
    cases = [(whole, native.ContribStats(1, None, 1), None), (slab, full, None), (slab, None, no_colour), (bad_degree, None, no_colour),
             (bad_degree, full, None), (whole, full, no_colour)]
    for old, new in ((_render_contrib, _render_error), (_forward_contrib, _forward_error)):
        for desc, stats, gauss in cases:
            rc0, msg0 = old(native, desc, stats, gauss)
            rc1, msg1 = new(native, desc, stats, None, gauss)
            assert rc0 < 0 and (rc0, msg0) == (rc1, msg1), (old.__name__, rc0, msg0, rc1, msg1)


# ---- host logic ------------------------------------------------------------------------------------------------------------------

def test_l1_error_map_against_numpy():
    from diff_gaussian_rasterization.contrib import l1_error_map
    g = torch.Generator().manual_seed(5)
    image = (torch.rand(3, 37, 50, generator=g) * 4 - 1).requires_grad_(True)
    target = torch.rand(3, 37, 50, generator=g)
    E = l1_error_map(image, target)
    assert E.shape == (37, 50) and E.dtype == torch.float32 and not E.requires_grad
    assert torch.equal(E, (image.detach() - target).abs().mean(0).clamp(0, 1))
    want = np.clip(np.abs(image.detach().numpy().astype(np.float64) - target.numpy().astype(np.float64)).mean(0), 0, 1)
    # below the clamp the channel sum is under 3: three subtractions and two adds of at most half an ulp of 4 (2^-23) each, divided
    # by 3, and the division's own rounding (2^-25): under 2^-21
    assert float(E.max()) == 1.0 and np.abs(E.numpy() - want).max() <= 2.0 ** -21
    assert not l1_error_map(target, target).any()


def test_error_stats_object():
    from diff_gaussian_rasterization.contrib import ContributionStats, ErrorStats
    st = ErrorStats(5, "cpu")
    assert isinstance(st, ContributionStats)
    assert (st.error_frame_q32.dtype, st.error_sum_q32.dtype, st.error_max.dtype) == (torch.int64, torch.int64, torch.float32)
    tensors = (st.count, st.weight_sum_q32, st.weight_max, st.error_frame_q32, st.error_sum_q32, st.error_max)
    assert all(t.shape == (5,) and not t.any() for t in tensors) and st.frames == 0
    st.error_sum_q32[1] = 3 * 2 ** 32 + 2 ** 31
    st.error_sum_q32[2] = 1
    assert st.error_sum.dtype == torch.float64 and st.error_sum.tolist() == [0.0, 3.5, 2.0 ** -32, 0.0, 0.0]
    st.count[0], st.weight_max[3], st.error_frame_q32[4], st.error_max[0], st.frames = 7, 0.5, 9, 0.25, 2
    st.reset()
    assert all(not t.any() for t in tensors) and st.frames == 0
    E = torch.zeros(4, 4)
    n = st.native_error(E)
    assert n.pixel_error == E.data_ptr() and n.error_frame_q32 == st.error_frame_q32.data_ptr()
    # a plain ContributionStats is what it was
    plain = ContributionStats(5, "cpu")
    assert sorted(vars(plain)) == ["P", "count", "device", "frames", "weight_max", "weight_sum_q32"]


def _model(P=200, D=1, seed=7):
    gm = GaussianModel(D)
    gm.adopt_scene(S.make_scene(P, 64, 64, D, seed), device="cpu")
    gm.training_setup(OptimizationDefaults())
    return gm


def _tables(gm):
    return {n: getattr(gm, n).detach().clone() for n in ("_xyz", "_features", "_opacity", "_scaling", "_rotation")}


def test_selection_takes_the_top_count_ties_to_the_lower_index_and_never_a_zero():
    P = 10
    scores = torch.tensor([5.0, 1.0, 3.0, 1.0, 9.0, 1.0, 3.0, 0.0, 7.0, 0.0], dtype=torch.float64)
    picked = {}
    orig = GaussianModel._densify_hot_and_prune

    def spy(self, hot, big, *a):
        picked["hot"] = torch.nonzero(hot)[:, 0].tolist()
        return orig(self, hot, big, *a)
    GaussianModel._densify_hot_and_prune = spy
    try:
        for count, want in ((0, []), (1, [4]), (4, [0, 2, 4, 8]), (6, [0, 1, 2, 4, 6, 8]), (7, [0, 1, 2, 3, 4, 6, 8]),
                            (8, [0, 1, 2, 3, 4, 5, 6, 8]), (10, [0, 1, 2, 3, 4, 5, 6, 8]), (1000, [0, 1, 2, 3, 4, 5, 6, 8])):
            gm = _model(P)
            torch.manual_seed(0)
            gm.densify_and_prune_by_score(scores, count, 0.0, 1e9, None)
            assert picked["hot"] == want, (count, picked["hot"])
            assert gm._xyz.shape[0] == P + len(want)          # a clone adds one row, a split two and removes one; nothing pruned
        gm = _model(P)
        gm.densify_and_prune_by_score(torch.tensor([float("nan")] * 5 + [-1.0] * 5), 5, 0.0, 1e9, None)
        assert picked["hot"] == [] and gm._xyz.shape[0] == P
    finally:
        GaussianModel._densify_hot_and_prune = orig
    with pytest.raises(ValueError, match="scores"):
        _model(P).densify_and_prune_by_score(scores[:9], 3, 0.005, 3.0, None)


@pytest.mark.parametrize("max_screen_size", (None, 20))
def test_with_the_gradient_rules_mask_the_tables_equal_densify_and_prune(max_screen_size):
    P, max_grad, extent = 300, 0.5, 3.0
    runs = []
    for by_score in (False, True):
        gm = _model(P, seed=11)
        g = torch.Generator().manual_seed(3)
        gm.xyz_gradient_accum[:] = torch.rand(P, 1, generator=g) * 4
        gm.denom[:] = torch.randint(0, 5, (P, 1), generator=g).float()             # (0 / 0: the NaN rows of the rule)
        gm.max_radii2D[:] = torch.rand(P, generator=g) * 40
        with torch.no_grad():
            gm._scaling[:60] += 4.0                                                 # some large ones: both clones and splits
        grads = gm.xyz_gradient_accum / gm.denom
        grads[grads.isnan()] = 0.0
        hot = torch.norm(grads, dim=-1) >= max_grad
        big = gm.get_scaling.detach().max(dim=1).values > gm.percent_dense * extent
        assert 0 < int((hot & big).sum()) and 0 < int((hot & ~big).sum()) and int(hot.sum()) < P
        torch.manual_seed(9)
        if by_score:
            gm.densify_and_prune_by_score(hot.double(), int(hot.sum()), 0.005, extent, max_screen_size)
        else:
            gm.densify_and_prune(max_grad, 0.005, extent, max_screen_size)
        runs.append(gm)
    a, b = (_tables(gm) for gm in runs)
    assert a["_xyz"].shape[0] != P
    for name in a:
        assert a[name].shape == b[name].shape and torch.equal(a[name], b[name]), name
    assert torch.equal(runs[0].max_radii2D, runs[1].max_radii2D) and torch.equal(runs[0].denom, runs[1].denom)


def test_option_defaults():
    d = OptimizationDefaults()
    assert (d.densify_error_views, d.densify_error_growth, d.densify_error_score) == (0, 0.05, "max")
    assert GaussianModel.DENSIFY_ERROR_SCORES == ("max", "sum")


def test_train_refuses_what_does_not_go_with_the_error_score():
    from train_loop import train
    for bad, match in ((dict(densify_strategy="mcmc"), "mcmc"), (dict(densify_absgrad=True), "densify_absgrad"),
                       (dict(densify_error_score="mean"), "densify_error_score")):
        opt = replace(OptimizationDefaults(), densify_error_views=2, **bad)
        with pytest.raises(ValueError, match=match):
            train(_model(50), [], [], opt, None, torch.zeros(3), iterations=10)
    # off: none of the three is looked at
    opt = replace(OptimizationDefaults(), densify_error_views=0, densify_error_score="mean")
    assert train(_model(50), [], [], opt, None, torch.zeros(3), iterations=0) is not None


def _settings():
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(32, 48, .5, .5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)


def test_rasterizer_refusals_that_need_no_device():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization.contrib import ContributionStats, ErrorStats
    E = torch.zeros(32, 48)
    with pytest.raises(ValueError, match="pixel_error without contributions"):
        dgr.GaussianRasterizer(_settings(), pixel_error=E)
    with pytest.raises(ValueError, match="ErrorStats"):
        dgr.GaussianRasterizer(_settings(), contributions=ContributionStats(4, "cpu"), pixel_error=E)
    for kw in (dict(depth_alpha=True), dict(absgrad=True)):
        with pytest.raises(ValueError, match="contributions"):
            dgr.GaussianRasterizer(_settings(), contributions=ErrorStats(4, "cpu"), pixel_error=E, **kw)
    z = torch.zeros(4, 3)
    args = dict(means3D=z, means2D=z, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1, 3), scales=z, rotations=torch.zeros(4, 4))
    raw_args = (z, z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4))
    st = ErrorStats(4, "cpu")
    for bad, match in ((torch.zeros(48, 32), "shape"), (torch.zeros(3, 32, 48), "shape"), (torch.zeros(32 * 48), "shape"),
                       (torch.zeros(32, 48, dtype=torch.float64), "float32"), (torch.zeros(32, 48, dtype=torch.float16), "float32"),
                       (np.zeros((32, 48), np.float32), "tensor")):
        r = dgr.GaussianRasterizer(_settings(), contributions=st, pixel_error=bad)
        with pytest.raises(ValueError, match=match):
            r(**args)
        with pytest.raises(ValueError, match=match):
            r.forward_raw(*raw_args)
    if torch.cuda.is_available():
        with pytest.raises(ValueError, match="lives on"):
            dgr.GaussianRasterizer(_settings(), contributions=st, pixel_error=E.to("cuda:0"))(**args)
    # what a statistics frame refuses is refused with a map too
    with pytest.raises(ValueError, match="5 Gaussians"):
        dgr.GaussianRasterizer(_settings(), contributions=ErrorStats(5, "cpu"), pixel_error=E)(**args)
    with pytest.raises(ValueError, match=r"torch\.no_grad\(\)"):
        dgr.GaussianRasterizer(_settings(), contributions=st, pixel_error=E)(**{**args, "means3D": z.clone().requires_grad_(True)})
    # a good map on host tensors gets as far as the plain call does; [1,H,W] is accepted
    for good in (E, E[None]):
        with pytest.raises(RuntimeError, match="no CPU path"):
            dgr.GaussianRasterizer(_settings(), contributions=st, pixel_error=good)(**args)
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, _settings(), tile_rows=(0, 1),
                              contrib=st, pixel_error=E)
    with pytest.raises(ValueError, match="pixel_error without contributions"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, _settings(), pixel_error=E)
    assert not any(t.any() for t in (st.error_frame_q32, st.error_sum_q32, st.error_max)) and st.frames == 0
