"""CPU checks of the median depth's float64 reference (tests/median_ref.py), which the GPU tests hold the kernels
to: the walk is anchored to the oracle's own image, the selection obeys the rule's defining inequalities at every pixel, a two-splat
scene has its closed form, and on every frame the GPU tests use the pixels whose selection float32 may legitimately flip
(gap < 1e-4) are at most 1 % of the frame."""
import numpy as np
import pytest

import median_ref as MR
import oracle
from test_gpu_depth_alpha import G1_CASES, _uncovered_half_kwargs
from test_gpu_parity import _fixture_kwargs

GAP = 1e-4               # ten times the bound the project holds alpha to: nearer than that float32 may choose the neighbouring splat
FRAMES = G1_CASES + ["uncovered half"]
_ids = lambda c: c if isinstance(c, str) else f"P{c['P']}_{c['W']}x{c['H']}_s{c['seed']}" + (f"_pose{c['pose']}" if "pose" in c else "")


def frame_kwargs(c):
    return _uncovered_half_kwargs() if isinstance(c, str) else _fixture_kwargs(c)


@pytest.mark.parametrize("c", FRAMES, ids=_ids)
def test_walk_selection_and_gap_on_the_gpu_tests_frames(c):
    kw = frame_kwargs(c)
    fr = oracle.rasterize(dtype=np.float64, parallel=isinstance(c, str), **kw)
    r = MR.median_depth(fr)
    # the walk is the oracle's blend
    assert np.abs(r["wsum"] - (1.0 - fr.final_T)).max() <= 1e-12
    has = r["index"] >= 0
    # a pixel has a median exactly when something was composited; these frames cover every pixel they touch with a median
    assert (has == (r["wsum"] > 0)).all() and has.any()
    assert (r["median"][~has] == 0).all() and not np.signbit(r["median"][~has]).any()
    assert (r["median"][has] == fr.depth[r["index"][has]]).all() and (r["median"][has] > 0.2).all()
    # the defining inequalities: the chosen splat's front transmittance is above one half, no later composited splat's is
    assert (r["t_med"][has] > 0.5).all()
    assert (r["t_next"][has] <= 0.5).all()
    # what float32 may flip
    share = float((r["gap"] < GAP).mean())
    print(f"gap < {GAP}: {int((r['gap'] < GAP).sum())} of {has.size} pixels ({100 * share:.2f} %), {int(has.sum())} with a median")
    assert share <= 0.01


@pytest.mark.parametrize("front,median,index", [(0.4, 3.0, 1), (0.6, 1.0, 0)])
def test_two_splats_closed_form(front, median, index):
    kw = MR.two_splat_kwargs(front)
    fr = oracle.rasterize(dtype=np.float64, **kw)
    r = MR.median_depth(fr)
    c = kw["image_height"] // 2
    assert r["index"][c, c] == index and r["median"][c, c] == median
    # the expected depth of the same pixel, from the frame rendered with colours (z, 1, 0): a depth at which nothing exists
    z = np.array([1.0, 3.0])
    akw = {k: v for k, v in kw.items() if k != "shs"}
    aux = oracle.rasterize(dtype=np.float64, **{**akw, "colors_precomp": np.stack([z, np.ones(2), np.zeros(2)], 1), "bg": np.zeros(3)})
    mean = aux.color[0, c, c] / aux.color[1, c, c]
    want = (front * 1.0 + (1.0 - front) * 0.9 * 3.0) / (front + (1.0 - front) * 0.9)
    assert abs(mean - want) <= 1e-6 and 1.0 < mean < 3.0
    if front == 0.4:
        assert abs(want - (0.4 * 1 + 0.6 * 0.9 * 3) / 0.94) <= 1e-15
    assert abs(r["gap"][c, c] - 0.1) <= 1e-6                     # T in front of the second splat is 1 - front: 0.1 from one half
