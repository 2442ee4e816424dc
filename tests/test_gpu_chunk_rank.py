"""The chunk order by ranking (csrc/gsr_select.hip k_chunk_rank) against its twin and against a stable sort.

A chunk of up to 16384 Gaussians without a live filter is ordered by a grid of blocks: every element counts the (key, position) pairs
in front of it and sums their tile counts.  GSR_SORT_FORCE_RADIX=1 runs the one-block LDS sort's radix passes instead (the kernel this
replaced): image, radii and every gradient of the two must agree bit for bit.  The library's own arrays are checked as well: the
binned prefix of the depth order is torch.sort(stable=True) of the visible Gaussians' depth keys, and the tile scan beside it is the
cumulative sum of their tile counts inside each chunk.

Chunk sizes straddle every edge of the kernel: the 16-lane group (1, 15, 16, 17), the 256-thread block of 16 elements (255, 256,
257), the cfg3-like size (5000), the 8192-entry LDS slab (8192, 8193), a chunk between the slab and the kernel's limit (12336) and one just above the limit (16385: the multi-launch radix sort, which the hook does not
touch).  Faint 2 px splats never saturate a 256x192 frame and their tile instances stay below the 2^18 a first chunk may not be
smaller than, so the n visible Gaussians of a frame are one chunk by rule, asserted from the frame's plan.
"""
import math
import os

import numpy as np
import pytest
import torch

import scene_synth as S
from util import raster_kwargs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
W, H = 256, 192
P_POOL = 20000
SIZES = [1, 15, 16, 17, 255, 256, 257, 5000, 8192, 8193, 12336, 16385]


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
    """Image, radii and the gradients of every input through the drop-in rasterizer."""
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw, True)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    color, radii = GaussianRasterizer(_settings(kw))(means2D=means2D, **inp)
    color.backward(gimg)
    grads = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    grads["means2D"] = means2D.grad.detach().cpu().numpy()
    torch.cuda.synchronize()
    return color.detach().cpu().numpy(), radii.cpu().numpy(), grads


def _forward_arrays(kw):
    """(plan, depth keys [P], order [P], tile scan [P], tiles touched [P]) of one forward, read from the frame's workspaces."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    inp = _inputs(kw, False)
    fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, _settings(kw))[2]
    torch.cuda.synchronize()
    v = N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan)
    keys = N.frame_arrays(fr.desc, fr.geom_ws)[0].cpu().numpy().astype(np.int64)
    return (fr.plan, keys, v["depth_order"].cpu().numpy().astype(np.int64), v["point_offsets"].cpu().numpy().view(np.uint32).astype(np.int64),
            v["tiles_touched"].cpu().numpy().astype(np.int64))


def _check_order_and_scan(kw, label):
    """The binned prefix of the order is the stable sort of the visible keys; the scan restarts at every chunk.  Returns the plan."""
    plan, keys, order, offs, tiles = _forward_arrays(kw)
    vis = np.nonzero(keys >= 0)[0]                              # -1: invisible; view depths are positive floats, their bits ascend with them
    assert plan.num_visible == vis.size, label
    k_sorted, idx = torch.sort(torch.as_tensor(keys[vis]), stable=True)
    want = vis[idx.numpy()]
    rb = [int(plan.chunk_rank_begin[c]) for c in range(plan.num_chunks + 1)]
    assert plan.chunks_run >= 1 and plan.chunks_filtered == 0, (label, plan.chunks_run, plan.chunks_filtered)
    for c in range(plan.chunks_run):
        got = order[rb[c]:rb[c + 1]]
        assert np.array_equal(got, want[rb[c]:rb[c + 1]]), f"{label}: chunk {c} order differs from the stable sort"
        assert np.array_equal(offs[rb[c]:rb[c + 1]], np.cumsum(tiles[got]) & 0xFFFFFFFF), f"{label}: chunk {c} tile scan"
    return plan


def _twin_equal(kw, gimg, label):
    c1, r1, g1 = _run(kw, gimg)
    os.environ["GSR_SORT_FORCE_RADIX"] = "1"
    try:
        c2, r2, g2 = _run(kw, gimg)
    finally:
        del os.environ["GSR_SORT_FORCE_RADIX"]
    assert np.isfinite(c1).all()
    assert np.array_equal(c1, c2) and np.array_equal(r1, r2), label
    for k in g1:
        assert np.array_equal(g1[k], g2[k]), (label, k)
    return g1


@pytest.fixture(scope="module")
def pool():
    """20 000 faint 2 px splats and the indices of those the library sees, in index order (visibility is per Gaussian: a frame of the
    first n of them has exactly n visible)."""
    sc = S.make_scene(P_POOL, W, H, 0, 137, zmin=2.0, zmax=6.0)
    sc.log_scales = torch.log(2.0 * sc.means3D[:, 2:3] / (H / (2 * 0.5))).expand(P_POOL, 3).contiguous()      # sigma = 2 px
    sc.opacity_logits = torch.full((P_POOL, 1), math.log(0.3 / 0.7))
    keys = _forward_arrays(raster_kwargs(sc, S.make_camera(W, H)))[1]
    vis = np.nonzero(keys >= 0)[0]
    assert vis.size >= max(SIZES), vis.size
    return sc, vis


@pytest.fixture(scope="module")
def gimg():
    return S.make_grad_image(W, H, 9).to(DEV)


def _subset(sc, idx):
    i = torch.as_tensor(idx)
    return S.Scene(sc.means3D[i].contiguous(), sc.log_scales[i].contiguous(), sc.raw_rotations[i].contiguous(),
                   sc.opacity_logits[i].contiguous(), sc.shs[i].contiguous(), sc.sh_degree)


@pytest.mark.parametrize("n", SIZES)
def test_one_chunk_of_n_gaussians(pool, gimg, n):
    sc, vis = pool
    kw = raster_kwargs(_subset(sc, vis[:n]), S.make_camera(W, H))
    plan = _check_order_and_scan(kw, f"n={n}")
    assert plan.num_chunks == 1 and plan.chunk_rank_begin[1] - plan.chunk_rank_begin[0] == n, (n, plan.num_chunks, list(plan.chunk_rank_begin))
    g = _twin_equal(kw, gimg, f"n={n}")
    assert n < 100 or np.abs(g["means3D"]).max() > 0            # (a handful of splats may all lie off the image)


def test_cfg3_like_frame_of_5000(gimg):
    """The 5000-Gaussian fixture of test_gpu_parity's chunk sort test: opaque splats of every size, chunks by the mass rule."""
    kw = raster_kwargs(S.make_scene(5000, W, H, 3, 109), S.make_camera(W, H))
    plan = _check_order_and_scan(kw, "p5000")
    assert 0 < plan.chunk_rank_begin[1] - plan.chunk_rank_begin[0] <= 8192
    g = _twin_equal(kw, gimg, "p5000")
    assert np.abs(g["means3D"]).max() > 0


def test_equal_depths_keep_index_order(gimg):
    """4000 Gaussians at bit-identical depth: equal keys rank by position, which is index order."""
    sc = S.make_scene(6000, W, H, 1, 131)
    sc.means3D[:4000, 2] = 1.5                                  # S.make_camera looks down +z from the origin: view depth = z
    kw = raster_kwargs(sc, S.make_camera(W, H))
    plan, keys, order, _, _ = _forward_arrays(kw)
    same = keys[:4000][keys[:4000] >= 0]
    assert same.size > 1000 and np.unique(same).size == 1       # (x and y were drawn for the old depths: under half stay in the frustum)
    # they sit behind one another in the order, ascending by index
    at = np.nonzero(keys[order[:plan.chunk_rank_begin[plan.chunks_run]]] == same[0])[0]
    assert at.size == same.size and np.array_equal(at, np.arange(at[0], at[0] + at.size))
    assert (np.diff(order[at]) > 0).all()
    _check_order_and_scan(kw, "equal depths")
    _twin_equal(kw, gimg, "equal depths")
