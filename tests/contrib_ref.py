"""A float64 reference for the per-Gaussian blend statistics, built on a frame of the oracle (which stays as it is), the way
tests/absgrad_ref.py is: per Gaussian, over every pixel of the frame, the number of pixels that composited it, the sum of its blend
weights w = alpha T and the largest single w.

Each tile's list is walked for all of its in-image pixels at once with the A.8 rules - a pixel composites entry i exactly when
position < n_contrib, not power > 0 and not alpha < 1/255 (the 0.99 clamp applied) - and T_i the transmittance in front of the entry.
tests/test_contrib_ref.py anchors the walk to the oracle's own image: per pixel sum_i w_i = 1 - final_T and
sum_i w_i rgb_i + final_T bg = color, within 1e-12.
"""
import numpy as np

TILE = 16


def contributions(fr, per_pixel=False):
    """fr: oracle.rasterize(dtype=np.float64, ...) frame.  Returns (count int64 [P], weight_sum [P], weight_max [P]); with per_pixel
    also (sum of w [H,W], sum of w rgb [3,H,W]) of the same walk."""
    assert fr.dtype == np.float64
    W, H, P = fr.W, fr.H, fr.P
    count, wsum, wmax = np.zeros(P, np.int64), np.zeros(P), np.zeros(P)
    px_w, px_c = np.zeros((H, W)), np.zeros((3, H, W))
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
        w = a * T                                                         # [L, n]; > 0 exactly where valid
        assert ((w > 0) == valid).all()
        np.add.at(count, ids, valid.sum(1))
        np.add.at(wsum, ids, w.sum(1))
        np.maximum.at(wmax, ids, w.max(1))
        if per_pixel:
            px_w[ys, xs] = w.sum(0)
            px_c[:, ys, xs] = fr.rgb[ids].T @ w
    return (count, wsum, wmax, px_w, px_c) if per_pixel else (count, wsum, wmax)
