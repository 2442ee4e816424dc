"""A float64 reference for the error-weighted blend total (diff_gaussian_rasterization.contrib.ErrorStats), built
on a frame of the oracle the way tests/contrib_ref.py is (that file stays as it is; its walk is restated here because it does not
hand out the per-pixel weights): per Gaussian, E_g = the sum over every pixel of the frame of w E, with w = alpha T the blend weight
of the A.8 rules and E the error map as the kernel reads it - clamped to [0, 1], a NaN as 0.

tests/test_contrib_error_ref.py anchors it: sum_g E_g = sum_u Ec(u) (1 - final_T(u)), E = 1 gives contrib_ref's weight_sum, E = 0
gives zeros.
"""
import numpy as np

TILE = 16


def clamp_map(E):
    """The map as the kernel reads it: fmin(fmax(x, 0), 1) with a NaN read as 0 (float64 [H,W])."""
    E = np.asarray(E, np.float64)
    return np.clip(np.where(np.isnan(E), 0.0, E), 0.0, 1.0)


def error_sums(fr, E):
    """fr: oracle.rasterize(dtype=np.float64, ...) frame; E [H,W].  Returns (esum [P], final_T [H,W] of the same walk)."""
    assert fr.dtype == np.float64
    W, H, P = fr.W, fr.H, fr.P
    Ec = clamp_map(E)
    assert Ec.shape == (H, W)
    esum = np.zeros(P)
    final_T = np.ones((H, W))
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
        final_T[ys, xs] = T[-1]
        T = np.concatenate((np.ones((1, T.shape[1])), T[:-1]), axis=0)      # in front of each entry
        w = a * T                                                         # [L, n]; > 0 exactly where valid
        np.add.at(esum, ids, (w * Ec[ys, xs][None, :]).sum(1))
    return esum, final_T
