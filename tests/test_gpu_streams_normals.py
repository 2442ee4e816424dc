"""The normal-map ops (diff_gaussian_rasterization/normals.py) where the caller issues them: each of the three ops
with its backward through tests/streams.py - on a side stream, behind a delay, every output and gradient equals the default-stream
run bit for bit.  The loss forward keeps a per-stream workspace (its ticket word): the side stream gets its own.

A file of its own, collected behind tests/test_gpu_streams.py, for the reason tests/test_gpu_streams_contrib.py gives."""
import pytest
import torch

import normals_ref as NR
import streams as ST
from test_gpu_streams import DEV, _all, _dev, _leaf

pytestmark = pytest.mark.gpu

H, W = 37, 70
TX, TY = NR.TANFOV


def _maps_make(seed, device):
    depth, alpha = NR.make_maps(H, W, "holes", seed=seed)
    gn, Nm = NR.make_upstream(H, W, seed=seed)
    g = torch.Generator().manual_seed(1500 + seed)
    return _dev(dict(depth=depth[None], alpha=alpha[None], gn=gn, Nm=Nm, up=torch.rand((), generator=g) + 0.5), device)


def _depth_normal_run(st):
    from diff_gaussian_rasterization.normals import depth_to_normal
    d, a = _leaf(st["depth"]), _leaf(st["alpha"])
    n = depth_to_normal(d, a, TX, TY, native=True)
    gd, ga = torch.autograd.grad(n, (d, a), st["gn"])
    return dict(n=n, ddepth=gd, dalpha=ga)


def _loss_run(st):
    from diff_gaussian_rasterization.normals import normal_consistency_loss
    N, d, a = _leaf(st["Nm"]), _leaf(st["depth"]), _leaf(st["alpha"])
    loss = normal_consistency_loss(N, d, a, TX, TY, native=True)
    gN, gd, ga = torch.autograd.grad(loss, (N, d, a), st["up"])
    return dict(loss=loss, dN=gN, ddepth=gd, dalpha=ga)


def _gauss_make(seed, device):
    s, q, m, g = NR.make_gaussians(1000, seed=seed)
    V, c = NR.make_camera(seed=seed)
    return _dev(dict(s=s, q=q, m=m, g=g, V=V, c=c), device)


def _gauss_run(st):
    from diff_gaussian_rasterization.normals import gaussian_normals
    q = _leaf(st["q"])
    out = gaussian_normals(st["s"], q, st["m"], st["V"], st["c"], native=True)
    (dq,) = torch.autograd.grad(out, q, st["g"])
    return dict(out=out, dq=dq)


CASES = [ST.Case("depth_to_normal", _maps_make, _all, _depth_normal_run),
         ST.Case("normal_consistency_loss", _maps_make, _all, _loss_run),
         ST.Case("gaussian_normals", _gauss_make, _all, _gauss_run)]


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_normal_ops_on_a_side_stream(case):
    got = ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert float(got[next(iter(got))].abs().sum()) > 0
