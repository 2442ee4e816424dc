"""A float64 reference for the median depth map, built on a frame of the oracle (which stays as it is), the way tests/contrib_ref.py
is: per pixel, the LAST composited splat whose front transmittance is above one half (2DGS's rule).

Each tile's list is walked for all of its in-image pixels at once with the A.8 rules - a pixel composites entry i exactly when
position < n_contrib, not power > 0 and not alpha < 1/255 (the 0.99 clamp applied) - with T_i the transmittance in front of the entry.
tests/test_median_ref.py anchors the walk to the oracle's own image (per pixel sum_i w_i = 1 - final_T within 1e-12) and to the rule's
defining inequalities.
"""
import numpy as np

TILE = 16


def median_depth(fr):
    """fr: oracle.rasterize(dtype=np.float64, ...) frame.  Returns per pixel ([H,W] each):
    index  int64: the median splat's Gaussian (-1: nothing composited),
    median: its fr.depth (+0.0 where index is -1),
    gap:    min over the composited splats of |T_i - 0.5| (inf where nothing composited): how far the selection is from flipping,
    wsum:   sum_i w_i of the same walk,
    t_med:  the chosen splat's front transmittance (nan where none),
    t_next: the largest front transmittance among the composited splats BEHIND the chosen one (-inf where there is none)."""
    assert fr.dtype == np.float64
    W, H = fr.W, fr.H
    index = np.full((H, W), -1, np.int64)
    median, wsum = np.zeros((H, W)), np.zeros((H, W))
    gap, t_med, t_next = np.full((H, W), np.inf), np.full((H, W), np.nan), np.full((H, W), -np.inf)
    for tile in range(fr.Gx * fr.Gy):
        r0, r1 = (int(v) for v in fr.ranges[tile])
        if r1 <= r0:
            continue
        ty, tx = divmod(tile, fr.Gx)
        ys, xs = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, H)), np.arange(tx * TILE, min((tx + 1) * TILE, W)), indexing="ij")
        ys, xs = ys.ravel(), xs.ravel()
        ids = fr.point_list[r0:r1].astype(np.int64)                       # [L]
        A, B, Cc, op = (fr.conic_opacity[ids, k][:, None] for k in range(4))
        dx = fr.xy[ids, 0][:, None] - xs[None, :].astype(np.float64)      # [L, n]: d = xy - pix
        dy = fr.xy[ids, 1][:, None] - ys[None, :].astype(np.float64)
        power = -0.5 * (A * dx * dx + Cc * dy * dy) - B * dx * dy
        alpha = np.minimum(0.99, op * np.exp(np.minimum(power, 0.0)))
        pos = np.arange(r1 - r0)[:, None]
        valid = (pos < fr.n_contrib[ys, xs][None, :]) & ~(power > 0) & ~(alpha < 1.0 / 255.0)
        a = np.where(valid, alpha, 0.0)
        T = np.cumprod(1.0 - a, axis=0)
        T = np.concatenate((np.ones((1, T.shape[1])), T[:-1]), axis=0)      # in front of each entry
        wsum[ys, xs] = (a * T).sum(0)
        cand = valid & (T > 0.5)                                          # T is non-increasing: the candidates are a prefix of the composited
        any_c = cand.any(0)
        last = (r1 - r0 - 1) - np.argmax(cand[::-1], axis=0)              # the last candidate's position
        cols = np.arange(len(xs))
        index[ys, xs] = np.where(any_c, ids[last], -1)
        median[ys, xs] = np.where(any_c, fr.depth[ids[last]], 0.0)
        gap[ys, xs] = np.where(valid, np.abs(T - 0.5), np.inf).min(0)
        t_med[ys, xs] = np.where(any_c, T[last, cols], np.nan)
        behind = valid & (pos > last[None, :])
        t_next[ys, xs] = np.where(behind, T, -np.inf).max(0)
        assert (valid.any(0) == any_c).all()                              # the first composited splat has T = 1
    return dict(index=index, median=median, gap=gap, wsum=wsum, t_med=t_med, t_next=t_next)


def two_splat_scene(front_opacity, size=32, back_opacity=0.9):
    """The closed-form scene as (scene_synth.Scene, scene_synth.Camera): two splats on one pixel's ray, at z = 1 (opacity
    front_opacity) and z = 3 (back_opacity), in front of an identity camera with tan(fov / 2) = 1.  Both sit on the ray through the
    centre of pixel (size / 2, size / 2), where both Gaussians peak: alpha there is the opacity itself."""
    import math

    import torch

    import scene_synth as S
    n = int(size)
    # pixel n/2 has NDC (2 px + 1) / n - 1 = 1 / n: a point (z / n, z / n, z) projects onto its centre
    means = torch.tensor([[1.0 / n, 1.0 / n, 1.0], [3.0 / n, 3.0 / n, 3.0]], dtype=torch.float32)
    logit = lambda p: math.log(p / (1.0 - p))
    shs = torch.tensor([[[1.0, -0.5, 0.25]], [[-0.5, 1.0, 0.5]]], dtype=torch.float32)
    scene = S.Scene(means, torch.tensor([[0.25] * 3, [0.75] * 3]).log(), torch.tensor([[1.0, 0, 0, 0], [1.0, 0, 0, 0]]),
                    torch.tensor([[logit(front_opacity)], [logit(back_opacity)]], dtype=torch.float32), shs, 0)
    return scene, S.make_camera(n, n, tanfovy=1.0)


def two_splat_kwargs(front_opacity, size=32, back_opacity=0.9):
    from util import raster_kwargs
    return raster_kwargs(*two_splat_scene(front_opacity, size, back_opacity))
