"""The depth-distortion ops (diff_gaussian_rasterization/distortion.py) where the caller issues them: each of the
three ops with its backward through tests/streams.py - on a side stream, behind a delay, every output and gradient equals the
default-stream run bit for bit.  The loss forward is two launches on the caller's stream with a workspace of the call's own between
them: the side stream's call shares nothing with the default stream's.

A file of its own, collected behind tests/test_gpu_streams.py, for the reason tests/test_gpu_streams_contrib.py gives."""
import pytest
import torch

import distortion_ref as DR
import streams as ST
from test_gpu_streams import DEV, _all, _dev, _leaf

pytestmark = pytest.mark.gpu

H, W = 130, 257             # 33 blocks of the map kernels


def _maps_make(seed, device):
    mom, alpha = DR.make_maps(H, W, "holes", seed=seed)
    g = torch.Generator().manual_seed(1700 + seed)
    return _dev(dict(mom=mom, alpha=alpha[None], gD=DR.make_upstream(H, W, seed=seed)[None], up=torch.rand((), generator=g) + 0.5), device)


def _map_run(st):
    from diff_gaussian_rasterization.distortion import distortion_map
    M, a = _leaf(st["mom"]), _leaf(st["alpha"])
    D = distortion_map(M, a, native=True)
    gM, ga = torch.autograd.grad(D, (M, a), st["gD"])
    return dict(D=D, dmoments=gM, dalpha=ga)


def _loss_run(st):
    from diff_gaussian_rasterization.distortion import distortion_loss
    M, a = _leaf(st["mom"]), _leaf(st["alpha"])
    loss = distortion_loss(M, a, native=True)
    gM, ga = torch.autograd.grad(loss, (M, a), st["up"])
    return dict(loss=loss, dmoments=gM, dalpha=ga)


def _gauss_make(seed, device):
    means, V, g = DR.make_gaussians(1000, seed=seed)
    return _dev(dict(means=means, V=V, g=g), device)


def _gauss_run(st):
    from diff_gaussian_rasterization.distortion import depth_moments
    m = _leaf(st["means"])
    out = depth_moments(m, st["V"], native=True)
    (dm,) = torch.autograd.grad(out, m, st["g"])
    return dict(out=out, dmeans=dm)


CASES = [ST.Case("distortion_map", _maps_make, _all, _map_run),
         ST.Case("distortion_loss", _maps_make, _all, _loss_run),
         ST.Case("depth_moments", _gauss_make, _all, _gauss_run)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_distortion_ops_on_a_side_stream(case):
    got = ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got[next(iter(got))].abs().sum()) > 0
