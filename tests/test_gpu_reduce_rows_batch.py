"""The wide row reduction's batched loop (csrc/gsr_render.hip k_reduce_rows<64>) against its plain loop and the float64 oracle.

A lane of a 64-lane group sums the rows sl, sl + 64, sl + 128, ... of its Gaussian in that order.  The batched loop loads eight trips'
rows together (and the next eight valid bytes with them) and adds them in the same order; GSR_REDUCE_ROWS_PLAIN=1 runs the loop it
replaced, one trip at a time.  The two must give the same bits.

Frames are 16 T pixels wide and 16 high: one row of T tiles.  One opaque, flat Gaussian in front of the camera covers every tile, so
it owns T rows: T = 1, 63, 64, 65 (one trip of a lane, with and without idle lanes), 255, 256, 257 (four trips: half a batch), 300, and
511, 512, 513, 600 (eight trips are one batch: the second batch runs on the bytes fetched beside the first one's rows).  Which variant a chunk takes is the launch rule's (launch_reduce_rows: 64 lanes when the chunk's instance bound is at
least 48 per Gaussian), read here from the frame's plan.  A few small splats sit beside the big one where the rule leaves room for
them: 48 instances per Gaussian on T tiles allow at most T / 48 Gaussians, so the frames of 63 to 65 tiles hold the big one alone,
and the one-tile frame cannot reach the wide variant at all - there the hook must change nothing, and the frame is held to the oracle
like the others.
"""
import os

import numpy as np
import pytest
import torch

import oracle
import scene_synth as S
from util import raster_kwargs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILES = [1, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 600]


def _frame(T):
    W, H = 16 * T, 16
    k = 2 if T < 48 else min(3, (T - 48) // 48)
    sc = S.make_scene(1 + k, W, H, 1, 500 + T, zmin=2.0, zmax=3.0)
    sc.means3D[0] = torch.tensor([0.0, 0.0, 1.0])
    # focal length 16 px (tan(fov_y / 2) = 0.5 at 16 rows): sigma = 16 T / 5 px, so alpha at the frame's ends, 8 T px away, is
    # 0.99 exp(-25 / 8) = 0.043 > 1 / 255 - every tile takes the splat; flat along the view axis, and a quarter as tall as wide (the
    # radius of a splat that is round on screen comes from lambda = mid + sqrt(mid^2 - det) with the root's argument all cancellation:
    # at sigma = 1600 px float32 is 0.6 px off, and the radius, a ceil, may differ from the oracle's by one)
    s = max(T / 5.0, 0.5)
    sc.log_scales[0] = torch.log(torch.tensor([s, s / 4, 0.01]))
    sc.raw_rotations[0] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc.opacity_logits[0] = float(np.log(0.99 / 0.01))
    # the small ones: behind it and close to the optical axis.  (Spread over the width of a 255-tile frame, tan(fov_x / 2) = 127, their
    # float32 projection is ill-conditioned: the rotation gradients then miss the oracle's bound by 1.8x with the parent's loop as well.)
    for i in range(k):
        z = 2.0
        sc.means3D[1 + i] = torch.tensor([((i + 1) / (k + 1) - 0.5) * min(3.0, 0.8 * T) * z, 0.0, z])
        sc.log_scales[1 + i] = float(np.log(0.02))
    return raster_kwargs(sc, S.make_camera(W, H)), W, H


def _settings(kw):
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV)
    return GaussianRasterizationSettings(
        image_height=kw["image_height"], image_width=kw["image_width"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"],
        bg=t(kw["bg"]), scale_modifier=kw["scale_modifier"], viewmatrix=t(kw["viewmatrix"]), projmatrix=t(kw["projmatrix"]),
        sh_degree=kw["sh_degree"], campos=t(kw["campos"]), prefiltered=False, debug=False)


def _inputs(kw, requires_grad):
    return {k: torch.as_tensor(np.asarray(kw[k]), dtype=torch.float32).to(DEV).requires_grad_(requires_grad)
            for k in ("means3D", "opacities", "shs", "scales", "rotations")}


def _run(kw, gimg):
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, True)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    color, radii = GaussianRasterizer(_settings(kw))(means2D=means2D, **inp)
    color.backward(torch.as_tensor(gimg, dtype=torch.float32, device=DEV))
    grads = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    grads["means2D"] = means2D.grad.detach().cpu().numpy()             # viewspace_points.grad of the training loop
    torch.cuda.synchronize()
    return color.detach().cpu().numpy(), radii.cpu().numpy(), grads


@pytest.mark.parametrize("T", TILES)
def test_batched_loop_equals_plain_loop_and_oracle(T):
    import diff_gaussian_rasterization as dgr
    kw, W, H = _frame(T)
    P = kw["means3D"].shape[0]
    inp = _inputs(kw, False)
    plan = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None,
                                 _settings(kw))[2].plan
    n = plan.chunk_rank_begin[1] - plan.chunk_rank_begin[0]
    assert plan.num_chunks == 1 and plan.chunks_run == 1 and plan.chunks_filtered == 0 and n == P, (plan.num_chunks, n, P)
    # the big Gaussian's rectangle is the whole row of tiles; the launch rule's choice follows from the plan
    assert plan.chunk_instances_max[0] >= T
    wide = plan.chunk_instances_max[0] // n >= 48
    assert wide == (T >= 63), (T, plan.chunk_instances_max[0], n)

    fr = oracle.rasterize(dtype=np.float64, **kw)
    strict = fr.fragile_px == 0
    # dL/dcolor > 0 everywhere: the big Gaussian's gradients are sums over up to 77 000 pixels, and with a gradient image of random
    # sign they cancel to a thousandth of their terms - the float32 sums then miss a bound relative to the RESULT in any order
    # (opacity at 257 tiles: 1.1x the bound, with the loop this one replaced as well)
    gimg = np.where(strict[None], np.abs(S.make_grad_image(W, H, 7).numpy()), 0.0)
    c1, r1, g1 = _run(kw, gimg)
    os.environ["GSR_REDUCE_ROWS_PLAIN"] = "1"
    try:
        c2, r2, g2 = _run(kw, gimg)
    finally:
        del os.environ["GSR_REDUCE_ROWS_PLAIN"]
    assert np.array_equal(c1, c2) and np.array_equal(r1, r2)
    for name in g1:
        assert np.array_equal(g1[name], g2[name]), (T, name)

    assert np.array_equal(r1, fr.radii)
    err = np.abs(c1 - fr.color).max(0)
    print(f"T={T}: P={P} instances<={plan.chunk_instances_max[0]} wide={wide} fragile {int((~strict).sum())} px, pixel err {err[strict].max():.2e}")
    assert err[strict].max() <= 1e-5
    want = fr.backward(gimg.astype(np.float64))
    for name, got in g1.items():
        w = want[name].reshape(got.shape)
        e = np.abs(got - w)
        bound = 1e-4 * np.abs(w).max() + 1e-4 * np.abs(w)
        print(f"  {name}: max |want| {np.abs(w).max():.3e}, max err {e.max():.3e}, worst err / bound {(e / np.maximum(bound, 1e-300)).max():.3f}")
        assert (e <= bound).all(), (T, name)
    assert np.abs(want["means3D"][0]).max() > 0
