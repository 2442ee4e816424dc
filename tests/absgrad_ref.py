"""A float64 reference for absgrad, built on a frame of the oracle (which stays as it is): per Gaussian, the signed AND the absolute
sum over pixels of that pixel's dL/dmean2D, with the W/2, H/2 factors of means2D.grad.

The oracle's frame exposes the sorted tile lists (ranges, point_list), the per-Gaussian screen quantities (xy, conic_opacity, rgb)
and the forward's per-pixel results (n_contrib, final_T).  Each tile's list is walked for all of its in-image pixels at once:
forward for the transmittance T_i in front of every entry, then the colour behind it by a reverse running sum - A.9's back-to-front
recurrence in closed form - with the A.8 skip rules (power > 0, alpha < 1/255), position < n_contrib, and the 0.99 clamp not
differentiated.  The signed sums restate what the oracle's backward_screen computes, so tests/test_absgrad_ref.py anchors them to
it (<= 1e-12 of the tensor's scale); the absolute sums are the same per-pixel terms under |.|.
"""
import math

import numpy as np

import oracle
import scene_synth as S

TILE = 16


def signed_and_abs_means2D(fr, bg, dL_dcolor):
    """fr: oracle.rasterize(dtype=np.float64, ...) frame; bg [3]; dL_dcolor [3,H,W].  Returns (signed [P,2], absolute [P,2])."""
    assert fr.dtype == np.float64
    W, H, P = fr.W, fr.H, fr.P
    g = np.asarray(dL_dcolor, np.float64)
    bg = np.asarray(bg, np.float64).reshape(3)
    signed, absolute = np.zeros((P, 2)), np.zeros((P, 2))
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
        G = np.exp(np.minimum(power, 0.0))
        alpha = np.minimum(0.99, op * G)
        pos = np.arange(r1 - r0)[:, None]
        valid = (pos < fr.n_contrib[ys, xs][None, :]) & ~(power > 0) & ~(alpha < 1.0 / 255.0)
        a = np.where(valid, alpha, 0.0)
        T = np.cumprod(1.0 - a, axis=0)
        T = np.concatenate((np.ones((1, T.shape[1])), T[:-1]), axis=0)      # in front of each entry
        gp = g[:, ys, xs]                                                 # [3, n]
        cdp = fr.rgb[ids] @ gp                                            # <rgb_i, dL/dpix>  [L, n]
        w = a * T
        contrib = w * cdp
        behind = np.cumsum(contrib[::-1], axis=0)[::-1] - contrib        # what the entries behind i add to <pixel, dL/dpix>
        bgdot = (bg[:, None] * gp).sum(0)[None, :]
        dL_dalpha = T * cdp - (behind + fr.final_T[ys, xs][None, :] * bgdot) / (1.0 - a)
        dL_dG = np.where(valid, op * dL_dalpha, 0.0)
        gdx, gdy = G * dx, G * dy
        ux = dL_dG * (-gdx * A - gdy * B) * (0.5 * W)
        uy = dL_dG * (-gdy * Cc - gdx * B) * (0.5 * H)
        np.add.at(signed[:, 0], ids, ux.sum(1)); np.add.at(signed[:, 1], ids, uy.sum(1))
        np.add.at(absolute[:, 0], ids, np.abs(ux).sum(1)); np.add.at(absolute[:, 1], ids, np.abs(uy).sum(1))
    return signed, absolute


def single_splat_kwargs(W=64, H=48, px=37, py=21, opacity=0.2, scale=0.05, z=3.0):
    """One isotropic splat whose projected centre is the pixel centre (px, py), well inside the image, with a precomputed colour: its
    alpha >= 1/255 support (opacity <= 0.2: inside the 3 sigma rectangle) is point-symmetric about that pixel.  The centre is placed
    by Newton steps on the oracle's own projection (xy is affine in x, y at fixed z under the identity view)."""
    cam = S.make_camera(W, H)
    kw = dict(image_height=H, image_width=W, tanfovx=math.tan(cam.FoVx * 0.5), tanfovy=math.tan(cam.FoVy * 0.5),
              bg=np.array([0.1, 0.3, 0.2]), scale_modifier=1.0, viewmatrix=cam.world_view_transform.numpy().astype(np.float64),
              projmatrix=cam.full_proj_transform.numpy().astype(np.float64), sh_degree=0, campos=cam.camera_center.numpy().astype(np.float64),
              means3D=np.array([[0.0, 0.0, z]]), opacities=np.array([[opacity]]), colors_precomp=np.array([[0.7, 0.2, 0.5]]),
              scales=np.full((1, 3), scale), rotations=np.array([[1.0, 0.0, 0.0, 0.0]]))
    step = 1e-3
    for _ in range(3):
        xy0 = oracle.rasterize(dtype=np.float64, **kw).xy[0].copy()
        probe = dict(kw, means3D=kw["means3D"] + np.array([[step, step, 0.0]]))
        slope = (oracle.rasterize(dtype=np.float64, **probe).xy[0] - xy0) / step      # pixels per unit of x, of y
        kw["means3D"] = kw["means3D"] + np.array([[(px - xy0[0]) / slope[0], (py - xy0[1]) / slope[1], 0.0]])
    return kw
