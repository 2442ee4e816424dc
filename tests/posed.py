"""Posed cameras and edge-population frames for the projection / geometry layer (csrc/gsr_math.h ewa_project, geom_backward_one).

scene_synth.make_camera(W, H) is the identity camera: R = I, t = 0, so every off-diagonal term of the view matrix and PV[3], PV[7]
are zero and a transposed index in the projection or its backward is multiplied by zero.  posed_camera() turns about all three
axes (every |R_ij| >= 0.15) and moves the camera off the origin (every |t_k| >= 0.3).  to_world() keeps a scene generated in view
space (scene_synth's frustum recipe) and places it in front of such a camera: p_w = R (p_v - t).

edge_scene() builds one frame out of labelled populations, each defined in view space:
  clamp_x, clamp_y, clamp_xy  |tx/tz| and/or |ty/tz| in [1.35, 2.0] tanfov (beyond the GSR_FOV_CLAMP = 1.3 clamp), z in [0.4, 2.5],
                              large enough that alpha >= 1/255 reaches at least 16 px into the image
  near                        z in [0.2 (1 + 1e-3), 0.3], inside and outside the clamp
  culled                      z in [0.2 (1 - 1e-2), 0.2 (1 - 1e-3)], and z < 0
  needle_disc                 largest / smallest scale >= 1e3
  opaque                      opacity logits in [6, 12]: alpha reaches the 0.99 clamp
  sh_clamp                    SH degree 3, DC chosen so that one or two channels clamp at 0 seen from this camera
  ordinary                    the background, so that lists have a realistic depth
Two decisions have no fragile band in the oracle: the near cut (z > 0.2) and the clamp of tx/tz (ty/tz).  The builder asserts that
every Gaussian sits at least 1e-3 (relative) away from both thresholds, evaluated from the world coordinates in binary32 and in
binary64, so that the oracle and the kernels take the same decision.
"""
from __future__ import annotations

import math

import numpy as np
import torch

import scene_synth as S
from torch_ref import eval_sh_basis

NEAR = 0.2                 # csrc/gsr_math.h near cut (p_view.z <= 0.2 is culled)
FOV_CLAMP = 1.3            # GSR_FOV_CLAMP
MARGIN = 1e-3              # relative distance every Gaussian keeps from both thresholds
POPULATIONS = ("ordinary", "clamp_x", "clamp_y", "clamp_xy", "near", "culled", "needle_disc", "opaque", "sh_clamp")


def rotation(ax: float, ay: float, az: float) -> np.ndarray:
    """Rz(az) Ry(ay) Rx(ax)."""
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


POSES = {          # every |R_ij| >= 0.15, every |t_k| >= 0.3
    "a": ((0.7, -0.6, 0.9), (0.4, -0.35, 0.5)),
    "b": ((-0.45, -0.7, -0.45), (-0.6, 0.45, -0.3)),
    "c": ((1.1, 0.75, -1.1), (0.3, 0.8, 0.65)),
}


def posed_camera(W: int, H: int, pose: str = "a", tanfovy: float = 0.5, tanfovx: float | None = None) -> S.Camera:
    """make_camera with a rotation about all three axes and a translation: campos = -R t != 0."""
    angles, t = POSES[pose]
    R, t = rotation(*angles), np.asarray(t, np.float64)
    assert np.abs(R).min() >= 0.15 and np.abs(t).min() >= 0.3, (np.abs(R).min(), np.abs(t).min())
    return S.make_camera(W, H, R, t, tanfovy, tanfovx)


def view_rt(cam: S.Camera):
    """(M [3,3], t [3]) in binary64 from the camera's binary32 view matrix: p_view = p_world @ M + t (row vectors)."""
    V = cam.world_view_transform.double().numpy()
    return V[:3, :3], V[3, :3]


def to_world(scene: S.Scene, cam: S.Camera) -> S.Scene:
    """The scene generated in view space, placed in front of `cam`: centres p_w = R (p_v - t) (the inverse of the camera's own
    binary32 matrix, so that the view-space statistics are those of the identity-camera frame).  Raw quaternions and SH are
    isotropic random and stay as they are."""
    M, t = view_rt(cam)
    pw = (scene.means3D.double().numpy() - t) @ np.linalg.inv(M)
    return S.Scene(torch.tensor(pw, dtype=torch.float32).contiguous(), scene.log_scales.clone(), scene.raw_rotations.clone(),
                   scene.opacity_logits.clone(), scene.shs.clone(), scene.sh_degree)


def view_coords(means3D, cam: S.Camera, dtype=np.float64) -> np.ndarray:
    """p_view of binary32 world centres, evaluated in `dtype` in the kernels' order (x V[0] + y V[4] + z V[8] + V[12], ...)."""
    V = cam.world_view_transform.numpy().astype(dtype)
    p = np.asarray(means3D, np.float32).astype(dtype)
    return np.stack([p[:, 0] * V[0, j] + p[:, 1] * V[1, j] + p[:, 2] * V[2, j] + V[3, j] for j in range(3)], 1)


def assert_margins(means3D, cam: S.Camera, margin: float = MARGIN):
    """Every Gaussian keeps `margin` (relative) from the near cut, and every one in front of it from the tx/tz and ty/tz clamp,
    in binary32 and binary64 from the world coordinates."""
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    for dt in (np.float32, np.float64):
        pv = view_coords(means3D, cam, dt)
        z = pv[:, 2]
        dz = np.abs(z / dt(NEAR) - 1)
        assert dz.min() >= margin, f"{dt.__name__}: a Gaussian within {dz.min():.2e} of the near cut"
        front = z > NEAR
        for k, tan in ((0, tanx), (1, tany)):
            lim = dt(FOV_CLAMP) * dt(tan)
            r = np.abs(pv[front, k] / z[front]) / lim
            assert np.abs(r - 1).min(initial=1.0) >= margin, f"{dt.__name__}: a Gaussian within {np.abs(r - 1).min():.2e} of the clamp"


def _sign(g, n):
    return torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)


def _u(g, n, lo, hi):
    return torch.rand(n, generator=g, dtype=torch.float64) * (hi - lo) + lo


EDGE_COUNTS = dict(clamp_x=40, clamp_y=40, clamp_xy=32, near=64, culled=48, needle_disc=96, opaque=96, sh_clamp=96)


def edge_scene(W: int, H: int, cam: S.Camera, seed: int, n_ordinary: int, counts: dict | None = None):
    """(scene in world coordinates for `cam`, labels [P] of population names).  SH degree 3; the populations above, each drawn
    in view space and placed with to_world()."""
    counts = dict(EDGE_COUNTS, **(counts or {}))
    g = torch.Generator().manual_seed(int(seed))
    tanx, tany = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
    fx, fy = W / (2 * tanx), H / (2 * tany)
    D, M = 3, 16
    parts, labels = [], []

    def add(label, xr, yr, z, log_scales, logits=None):
        n = z.shape[0]
        rots = torch.randn(n, 4, generator=g)
        logits = torch.randn(n, 1, generator=g) * 1.5 if logits is None else logits.view(n, 1)
        shs = torch.randn(n, M, 3, generator=g) * 0.1
        shs[:, 0, :] = torch.randn(n, 3, generator=g) * 0.25 / S.SH_C0
        means = torch.stack([xr * z, yr * z, z], 1)
        parts.append((means, log_scales, rots, logits.float(), shs))
        labels.extend([label] * n)

    def frustum(n, lim=1.1):      # tx/tz, ty/tz inside `lim` x the frustum (scene_synth.make_scene's recipe)
        return (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * lim * tanx, \
               (torch.rand(n, generator=g, dtype=torch.float64) * 2 - 1) * lim * tany

    def log_u(n, lo, hi, k=3):
        return (torch.rand(n, k, generator=g) * (math.log(hi) - math.log(lo)) + math.log(lo))

    n = n_ordinary
    z = _u(g, n, 0.5, 6.0)
    add("ordinary", *frustum(n), z, log_u(n, 0.004, 0.04))

    # clamp populations: the centre beyond 1.35 x the frustum, an isotropic-ish splat whose alpha >= 1/255 (opacity >= 0.5:
    # |d| / sigma <= 3.11) reaches 16 px past the image edge: sigma = (offset + 16 px) / 2.5
    for label, cx, cy in (("clamp_x", True, False), ("clamp_y", False, True), ("clamp_xy", True, True)):
        n = counts[label]
        z = _u(g, n, 0.4, 2.5)
        xr, yr = frustum(n, 1.0)
        off = torch.zeros(n, dtype=torch.float64)
        offx = torch.zeros(n, dtype=torch.float64)
        offy = torch.zeros(n, dtype=torch.float64)
        if cx:
            r = _u(g, n, 1.35, 2.0)
            xr = _sign(g, n).double() * r * tanx
            offx = (r - 1) * W / 2
        if cy:
            r = _u(g, n, 1.35, 2.0)
            yr = _sign(g, n).double() * r * tany
            offy = (r - 1) * H / 2
        off = torch.sqrt(offx * offx + offy * offy) + 16 * math.sqrt(2)
        sigma_px = off / 2.5
        s = sigma_px * z / min(fx, fy)
        ls = (torch.log(s).float()[:, None] + (torch.rand(n, 3, generator=g) * 0.2 - 0.1)).contiguous()
        add(label, xr, yr, z, ls, logits=_u(g, n, 0.0, 3.0).float())

    # near: just in front of the cut; about a third of them beyond the clamp in x, sized as the clamp populations
    n = counts["near"]
    z = _u(g, n, NEAR * (1 + 2 * MARGIN), 0.3)
    xr, yr = frustum(n, 1.2)
    far = torch.rand(n, generator=g) < 0.35
    r = _u(g, n, 1.35, 1.7)
    xr = torch.where(far, _sign(g, n).double() * r * tanx, xr)
    s_far = ((r - 1) * W / 2 + 16) / 2.5 * z / fx
    ls = torch.where(far[:, None], torch.log(s_far).float()[:, None].expand(n, 3), log_u(n, 0.001, 0.01))
    add("near", xr, yr, z, ls.contiguous())

    # culled: just behind the cut, and behind the camera
    n = counts["culled"]
    z = torch.where(torch.arange(n) % 2 == 0, _u(g, n, NEAR * (1 - 1e-2), NEAR * (1 - 2 * MARGIN)), -_u(g, n, 0.05, 3.0))
    add("culled", *frustum(n, 0.9), z, log_u(n, 0.004, 0.04))

    # needles (one long axis) and discs (one short axis): largest / smallest scale >= 1e3.  Seen edge-on, a disc's 2D covariance is
    # the 0.3 dilation across and its diameter along: the binary32 conic of a long one is ill-conditioned (the oracle's kappa), and
    # its alpha = 1/255 ring turns into a band of fragile pixels, so the long axis stays at a few pixels
    n = counts["needle_disc"]
    z = _u(g, n, 1.5, 5.0)
    big = log_u(n, 0.01, 0.04, 1)
    ratio = math.log(1e3) + torch.rand(n, 1, generator=g) * math.log(3.0)
    needle = torch.arange(n)[:, None] % 2 == 0
    ls = torch.cat([big, torch.where(needle, big - ratio, big), big - ratio], 1)
    perm = torch.argsort(torch.rand(n, 3, generator=g), 1)              # the long / short axes in random local slots
    add("needle_disc", *frustum(n, 1.0), z, torch.gather(ls, 1, perm).contiguous())

    n = counts["opaque"]
    add("opaque", *frustum(n, 1.0), _u(g, n, 1.0, 6.0), log_u(n, 0.01, 0.06), logits=_u(g, n, 6.0, 12.0).float())

    n = counts["sh_clamp"]
    add("sh_clamp", *frustum(n, 1.0), _u(g, n, 1.0, 6.0), log_u(n, 0.01, 0.05))

    means, log_scales, rots, logits, shs = (torch.cat([p[k] for p in parts]) for k in range(5))
    scene = to_world(S.Scene(means.float().contiguous(), log_scales.float().contiguous(), rots, logits, shs.contiguous(), D), cam)
    labels = np.array(labels)

    # sh_clamp: the DC term sets rgb = sum_k basis_k sh_k + 0.5 to -U(0.1, 0.4) on one or two channels (clamped at 0) and to
    # +U(0.2, 0.8) on the others, from this camera's direction
    sel = np.nonzero(labels == "sh_clamp")[0]
    d = scene.means3D[sel].double() - cam.camera_center.double()[None]
    d = d / d.norm(dim=1, keepdim=True)
    basis = eval_sh_basis(D, d)
    rest = torch.einsum("pk,pkc->pc", basis[:, 1:], scene.shs[sel, 1:].double())
    target = _u(g, sel.size * 3, 0.2, 0.8).view(-1, 3)
    k = torch.randint(1, 3, (sel.size,), generator=g)
    chans = torch.argsort(torch.rand(sel.size, 3, generator=g), 1)
    neg = torch.zeros(sel.size, 3, dtype=torch.bool)
    for j in range(2):
        neg[torch.arange(sel.size)[k > j], chans[k > j, j]] = True
    target = torch.where(neg, -_u(g, sel.size * 3, 0.1, 0.4).view(-1, 3), target)
    scene.shs[sel, 0] = ((target - 0.5 - rest) / S.SH_C0).float()

    assert_margins(scene.means3D.numpy(), cam)
    return scene, labels


def population_masks(labels: np.ndarray) -> dict:
    return {p: labels == p for p in POPULATIONS if (labels == p).any()}
