"""A statistics frame (GaussianRasterizer(..., contributions=)) where the caller issues it: one case through
tests/streams.py - on a side stream, behind a delay, the frame and the three accumulators equal the default-stream run bit for bit.

A file of its own, collected behind tests/test_gpu_streams.py: that module's sensitivity tests need an op on a second stream to run
WHILE the side stream sits in its delay, which depends on the hardware queues the two streams share, and so on how many streams
the session has taken from torch's pool before them.  A stream taken here, behind them, cannot move theirs."""
import pytest
import torch

import streams as ST
from test_gpu_streams import DEV, _frame_make, _frame_staged

pytestmark = pytest.mark.gpu


def _run(st):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from diff_gaussian_rasterization.contrib import ContributionStats
    m = st["meta"]
    rs = GaussianRasterizationSettings(m["H"], m["W"], m["tanfovx"], m["tanfovy"], st["bg"], 1.0, st["viewmatrix"], st["projmatrix"], m["D"],
                                       st["campos"], False, False)
    stats = ContributionStats(m["P"], DEV)
    geom = {k: st[k] for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    color, radii = GaussianRasterizer(rs, contributions=stats)(means2D=torch.zeros(m["P"], 3, device=DEV), **geom)
    return dict(color=color, radii=radii, count=stats.count, weight_sum_q32=stats.weight_sum_q32, weight_max=stats.weight_max)


def test_statistics_frame_on_a_side_stream():
    case = ST.Case("contrib frame", _frame_make(4000, 160, 96, 2), _frame_staged, _run, blocking=True)
    got = ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)
    assert int(got["count"].sum()) > 0
