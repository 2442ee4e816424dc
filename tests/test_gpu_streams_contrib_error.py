"""An error frame (GaussianRasterizer(..., contributions=ErrorStats, pixel_error=)) where the caller issues it: one
case through tests/streams.py - on a side stream, behind a delay, the frame, the statistics and the folded error tensors equal the
default-stream run bit for bit (the blend and the fold both name the caller's stream).

A file of its own, collected behind tests/test_gpu_streams.py, for the reason tests/test_gpu_streams_contrib.py gives."""
import pytest
import torch

import streams as ST
from test_gpu_streams import DEV, _frame_make, _frame_staged

pytestmark = pytest.mark.gpu


def _run(st):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from diff_gaussian_rasterization.contrib import ErrorStats
    m = st["meta"]
    rs = GaussianRasterizationSettings(m["H"], m["W"], m["tanfovx"], m["tanfovy"], st["bg"], 1.0, st["viewmatrix"], st["projmatrix"], m["D"],
                                       st["campos"], False, False)
    stats = ErrorStats(m["P"], DEV)
    geom = {k: st[k] for k in ("means3D", "opacities", "shs", "scales", "rotations")}
    E = st["target"][1]                      # a staged buffer: the decoy's until the side stream has copied the real one in
    color, radii = GaussianRasterizer(rs, contributions=stats, pixel_error=E)(means2D=torch.zeros(m["P"], 3, device=DEV), **geom)
    return dict(color=color, radii=radii, count=stats.count, weight_sum_q32=stats.weight_sum_q32, weight_max=stats.weight_max,
                error_frame_q32=stats.error_frame_q32, error_sum_q32=stats.error_sum_q32, error_max=stats.error_max)


def test_error_frame_on_a_side_stream():
    case = ST.Case("contrib error frame", _frame_make(4000, 160, 96, 2), _frame_staged, _run, blocking=True)
    got = ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)
    assert int(got["error_sum_q32"].sum()) > 0 and float(got["error_max"].max()) > 0 and not got["error_frame_q32"].any()
