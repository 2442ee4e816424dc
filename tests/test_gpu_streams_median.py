"""The median-depth frame on a side stream and on a second one (tests/streams.py's protocol, as tests/test_gpu_streams.py runs it for
every other op): the forward and the backward of GaussianRasterizer(depth_alpha=True, median_depth=True), issued on a side stream
behind a delay while the inputs are still the decoy's, give the bits of the default-stream run.  A launch, memset or copy of the feature
on any other stream - the two median maps carried between chunks, the backward's read of median_enc - would run early and show."""
import pytest
import torch

import streams as ST
from test_gpu_streams import DEV, FRAME_A, _frame_make, _frame_staged, _leaf, _seed_a

pytestmark = pytest.mark.gpu


def _make(seed, device):
    st = _frame_make(**FRAME_A, seed_of=_seed_a)(seed, device)
    m = st["meta"]
    g = torch.Generator().manual_seed(2000 + seed)
    st["gmedian"] = (torch.rand(1, m["H"], m["W"], generator=g) - 0.5).to(device)
    return st


def _run(st):
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from test_gpu_streams import CAM, GEOM
    m = st["meta"]
    leaves = {k: _leaf(st[k]) for k in GEOM if k in st}
    rs = GaussianRasterizationSettings(m["H"], m["W"], m["tanfovx"], m["tanfovy"], st["bg"], 1.0, *(st[k] for k in CAM[:2]), m["D"], st[CAM[2]],
                                       False, False)
    leaves["means2D"] = torch.zeros(m["P"], 3, device=st["bg"].device, requires_grad=True)
    out = GaussianRasterizer(rs, depth_alpha=True, median_depth=True)(**leaves)
    res = dict(color=out[0], radii=out[1], depth=out[2], alpha=out[3], median=out[4])
    ups = [st["gimg"], st["gdepth"], st["galpha"], st["gmedian"]]
    ST.between(*ups)
    grads = torch.autograd.grad([out[0], out[2], out[3], out[4]], list(leaves.values()), ups)
    res.update({"d_" + k: g for k, g in zip(leaves, grads)})
    return res


CASE = ST.Case("frame_median_depth", _make, _frame_staged, _run, blocking=True)


@pytest.mark.parametrize("which", ["a side stream", "a second stream"])
def test_median_frame_on_another_stream(which):
    want = ST.default_run(CASE, DEV)
    assert float(want["median"].max()) > 0.2 and float(want["d_means3D"].abs().max()) > 0
    d = ST.Delay.on(DEV)
    host_ms = ST.HOST_MS.get(CASE.name + " (backward)", 0.0)
    d.set(max(ST.DELAY_MS, 10.0 * host_ms))
    assert d.ms >= 10.0 * host_ms
    side = torch.cuda.Stream(device=DEV)
    if which == "a second stream":                  # another stream than the first side stream, which stays alive beside it
        first, side = side, torch.cuda.Stream(device=DEV)
        assert first.cuda_stream != side.cuda_stream
    got = ST.check_on_side_stream(CASE, side, DEV)
    assert set(got) == set(want)
