"""Binary64 restatement of Mip-Splatting's 3D smoothing filter (diff_gaussian_rasterization/filter3d.py, csrc/gsr_filter3d_math.h;
DESIGN.md section 19), the fixtures and the error rules of tests/test_filter3d_ref.py and tests/test_gpu_filter3d.py.

Filter size.  The restatement evaluates every comparison of valid(p,c) in binary64 from the binary32 inputs and classes it as true,
false or undecided: undecided = within the binary32 error of that comparison, bounded per (Gaussian, camera) pair from the magnitudes
of its terms.  With u = 2^-24 and, per coordinate, T = |x V0j| + |y V1j| + |z V2j| + |V3j|:
    B_j = 4 u T_j                      a view coordinate: three fused multiply-adds (3 roundings; 4 covers separate products and adds)
    near:    |z - 0.2| <= B_z + 0.2 u                                          (0.2 itself is rounded to binary32)
    screen:  ||x| fx - 0.65 W z| <= fx B_x + 0.65 W B_z + 4 u (|x| fx + 0.65 W z)
                                       (the product x fx: 1 rounding; 0.65 rounded, times W, times z: 3; 4 u on both sides covers them)
d_hi = min z over the decidedly valid cameras, d_lo = min z over the valid-or-undecided ones; the result must lie in
[d_lo - B, d_hi + B], B the largest B_z of the cameras in play, and the filter has 4 more roundings, relative (sqrt, the division by F,
the product; one spare).

Application.  `apply()` is the rule in binary64 with autograd's gradient.  A binary32 result is held to K u times the sum of the
magnitudes of its terms, K the count of roundings on the way (a libm call counts 2: its error is below 1 ulp = 2 u):
    K_U = 10   u'_i = u_i - g_i, g_i = -0.5 log1p(w^2), w = f exp(-u_i):  exp 2, product 1, square 2 (3 + 3) + 1 = 7, log1p 2 -> 9 on
               |g_i|, the subtraction 1 on |u_i| + |g_i|.  Terms: |u_i| + |log f| + |g_i|.
    K_L = 20   l' = l + log c - log1p(e^l (1 - c)):  log c = sum g_i: 9 + 2 adds = 11; 1 - c = -expm1(log c): 11 + 2 = 13 (its
               condition number is below 1); e^l 2, the product 1 -> 16 on the argument, log1p 2 -> 18 on that term; the two adds 2:
               20 on the largest.  Terms: |l| + |log c| + log1p(e^l (1 - c)) + 1.
    K_S = 4    s'_i = m sqrt(1 + (n/m)^2): quotient 1, square 3, the sum 2.5, sqrt 2.25, product 3.25.  Terms: s'_i.
    K_O = 16   o' = o prod rho_i, rho_i = (1 or n/m) / sqrt(1 + (n/m)^2): 4.25 each, two products, one more: 15.75.  Terms: o'.
    + 6        on each of K_U, K_L, K_G where a log-scale is under -87 (s itself under binary32's normal range): exp(-u) alone would
               overflow, so w = (f E) E with E = exp(-u/2): exp 2, product 1, product 1 + 2 = 6 where f exp(-u) has 3; its square 13.
    K_G = 33   a gradient: r_i and 1 - r_i 9, 1 / (1 - p') = (1 + e^l) / (1 + e^l (1 - c)): 21, two products and the add: 9 + 21 + 3.
               Terms: the two products of each gradient (one for dL/dl and dL/do).
"""
from __future__ import annotations

import math

import numpy as np
import torch

import posed
import scene_synth as S

U = 2.0 ** -24
NEAR, VARIANCE, MARGIN = 0.2, 0.2, 0.15
K_U, K_L, K_S, K_O, K_G = 10, 20, 4, 16, 33
K_DEEP = 6                  # more, each, for a log-scale under EXP_SWITCH (below)
EXP_SWITCH = -87.0          # csrc/gsr_filter3d_math.h kF3dExpSwitch
CAM_CHUNK = 64              # csrc/gsr_filter3d.hip kF3dCamChunk: cameras the kernel stages at once
F64, F32 = torch.float64, torch.float32


# ---- cameras and fixtures -----------------------------------------------------------------------------------------------------------
def look_at_camera(W, H, position, tanfovy, roll=0.0):
    """A camera at `position` looking at the origin."""
    c = np.asarray(position, np.float64)
    fwd = -c / np.linalg.norm(c)
    up = np.array([0.0, 1.0, 0.0]) if abs(fwd[1]) < 0.9 else np.array([1.0, 0.0, 0.0])
    right = np.cross(up, fwd); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    cr, sr = math.cos(roll), math.sin(roll)
    R = np.stack([cr * right + sr * down, -sr * right + cr * down, fwd], 1)           # columns: the camera's axes in the world
    return S.make_camera(W, H, R, -R.T @ c, tanfovy)


def cap_cameras(n, seed):
    """n cameras in a cap of 40 degrees around +z at distance 3.5 .. 5, looking at the origin, of four image sizes and focal lengths."""
    g = np.random.default_rng(seed)
    shapes = ((64, 48, 0.5), (80, 80, 0.4), (48, 64, 0.7), (96, 40, 0.3))
    cams = []
    for i in range(n):
        th, ph, r = g.uniform(0, math.radians(40)), g.uniform(0, 2 * math.pi), g.uniform(3.5, 5.0)
        W, H, tan = shapes[i % len(shapes)]
        cams.append(look_at_camera(W, H, (r * math.sin(th) * math.cos(ph), r * math.sin(th) * math.sin(ph), r * math.cos(th)), tan, g.uniform(-0.5, 0.5)))
    return cams


def posed_trio():
    return [posed.posed_camera(64, 48, "a", 0.5), posed.posed_camera(80, 80, "b", 0.4), posed.posed_camera(48, 64, "c", 0.7)]


def _behind(cam, n, g):
    """n centres behind `cam`, in world coordinates."""
    pv = torch.stack([torch.rand(n, generator=g) * 2 - 1, torch.rand(n, generator=g) * 2 - 1, -torch.rand(n, generator=g) * 3 - 0.3], 1)
    M, t = posed.view_rt(cam)
    return torch.tensor((pv.double().numpy() - t) @ np.linalg.inv(M), dtype=F32)


def fixture(name: str, P: int):
    """-> (xyz [P,3] binary32, cameras).  posed1: one posed camera and a scene made in its view space (z in (0, 6): some in front of
    the near cut), a tenth of it behind the camera.  posed3: the three posed cameras, a third of the scene in front of each.
    cap70: CAM_CHUNK + 6 cameras around a box of centres, a tenth of them beyond the cameras (behind every one)."""
    g = torch.Generator().manual_seed(1000 + P)
    if name == "posed1":
        cams = posed_trio()[:1]
        xyz = posed.to_world(S.make_scene(P, 64, 48, 0, 11 + P), cams[0]).means3D
        n = P // 10
        if n:
            xyz = torch.cat((xyz[:P - n], _behind(cams[0], n, g)))
        elif P == 1:
            xyz = posed.to_world(S.make_scene(1, 64, 48, 0, 11, zmin=1.0), cams[0]).means3D
        return xyz.contiguous(), cams
    if name == "posed3":
        cams = posed_trio()
        parts = [posed.to_world(S.make_scene((P + 2 - k) // 3, c.image_width, c.image_height, 0, 21 + k + P, tanfovy=math.tan(c.FoVy / 2),
                                             zmin=0.3 if P < 3 else 0.0), c).means3D for k, c in enumerate(cams)]
        return torch.cat(parts).contiguous(), cams
    if name == "cap70":
        cams = cap_cameras(CAM_CHUNK + 6, 5)
        xyz = torch.rand(P, 3, generator=g) * 3 - 1.5
        n = P // 10
        if n:
            xyz[P - n:, 2] = 40.0 + 10 * torch.rand(n, generator=g)
        return xyz.contiguous(), cams
    raise KeyError(name)


FIXTURES = ("posed1", "posed3", "cap70")


def edge_fixture():
    """257 centres for the identity camera 64 x 64 (fx = fy = 64 exactly, so 0.65 W and every product below are exact in binary32):
    247 ordinary ones, then ten rows one binary32 step inside and outside each of the five bounds: z > 0.2 at x = y = 0, and
    |x| <= 0.65 z, |y| <= 0.65 z at z = 1.  -> (xyz, [camera], rows of the ten, expected `seen` of the ten)."""
    cam = S.make_camera(64, 64)
    xyz = S.make_scene(247, 64, 64, 0, 5, zmin=0.5).means3D
    near, half, one = np.float32(NEAR), np.float32(0.5 + MARGIN), np.float32(1.0)
    up, dn = (lambda v: np.nextafter(v, np.float32(np.inf))), (lambda v: np.nextafter(v, np.float32(-np.inf)))
    rows = [(0, 0, up(near)), (0, 0, dn(near)),
            (dn(half), 0, one), (up(half), 0, one), (-dn(half), 0, one), (-up(half), 0, one),
            (0, dn(half), one), (0, up(half), one), (0, -dn(half), one), (0, -up(half), one)]
    xyz = torch.cat((xyz, torch.tensor(np.array(rows, np.float32))))
    return xyz.contiguous(), [cam], torch.arange(247, 257), torch.tensor([True, False] * 5)


def intrinsics(cam):
    W, H = int(cam.image_width), int(cam.image_height)
    return float(np.float32(W / (2.0 * math.tan(cam.FoVx * 0.5)))), float(np.float32(H / (2.0 * math.tan(cam.FoVy * 0.5)))), float(W), float(H)


# ---- the filter size: a bracket ----------------------------------------------------------------------------------------------------
def compute_bracket(xyz, cameras):
    """-> dict of [P] binary64 tensors: d_lo, d_hi (inf where no camera is valid-or-undecided / decidedly valid), B, seen_sure,
    seen_maybe, and the filter's bracket f_lo, f_hi (fill rule and scale applied)."""
    p = xyz.to(F64)
    P = p.shape[0]
    inf = torch.full((P,), math.inf, dtype=F64)
    d_hi, d_lo, z_maybe_max, B = inf.clone(), inf.clone(), -inf.clone(), torch.zeros(P, dtype=F64)
    half = 0.5 + MARGIN
    focal_max = 0.0
    for cam in cameras:
        fx, fy, W, H = intrinsics(cam)
        focal_max = max(focal_max, fx)
        V = torch.as_tensor(cam.world_view_transform).to(F64)
        co = [p @ V[:3, j] + V[3, j] for j in range(3)]
        Bj = [4 * U * (p.abs() @ V[:3, j].abs() + V[3, j].abs()) for j in range(3)]
        x, y, z = co
        t_near, f_near = z - NEAR > Bj[2] + NEAR * U, NEAR - z > Bj[2] + NEAR * U
        sure, false = t_near, f_near
        for v, Bv, f, n in ((x, Bj[0], fx, W), (y, Bj[1], fy, H)):
            L, R = v.abs() * f, half * n * z
            E = f * Bv + half * n * Bj[2] + 4 * U * (L + R.abs())
            sure = sure & (L <= R - E)
            false = false | (L > R + E)
        maybe = ~false
        d_hi = torch.where(sure & (z < d_hi), z, d_hi)
        d_lo = torch.where(maybe & (z < d_lo), z, d_lo)
        z_maybe_max = torch.where(maybe & (z > z_maybe_max), z, z_maybe_max)
        B = torch.where(maybe, torch.maximum(B, Bj[2]), B)
    seen_sure, seen_maybe = d_hi < math.inf, d_lo < math.inf
    lo = d_lo - B                                                  # of a Gaussian that is seen
    hi = torch.where(seen_sure, d_hi, z_maybe_max) + B
    if not bool(seen_maybe.any()):
        return dict(seen_sure=seen_sure, seen_maybe=seen_maybe, none=True)
    fill_lo = lo[seen_sure].max() if bool(seen_sure.any()) else lo[seen_maybe].min()
    fill_hi = hi[seen_maybe].max()
    # decidedly seen: its own bracket; decidedly unseen: the fill's; undecided: either
    r_lo = torch.where(seen_sure, lo, torch.where(seen_maybe, torch.minimum(lo, fill_lo), fill_lo))
    r_hi = torch.where(seen_sure, hi, torch.where(seen_maybe, torch.maximum(hi, fill_hi), fill_hi))
    k = math.sqrt(VARIANCE) / focal_max
    return dict(d_lo=d_lo, d_hi=d_hi, B=B, seen_sure=seen_sure, seen_maybe=seen_maybe, none=False, focal_max=focal_max,
                f_lo=r_lo * k * (1 - 4 * U), f_hi=r_hi * k * (1 + 4 * U), decided=(d_lo == d_hi))


def check_compute(filter_3D, br, what=""):
    """The bracket, and its own condition: at least 95 % of the Gaussians decided."""
    f = filter_3D.detach().cpu().to(F64).reshape(-1)
    assert float(br["decided"].double().mean()) >= 0.95, f"{what}: the fixture leaves {int((~br['decided']).sum())} Gaussians undecided"
    bad = (f < br["f_lo"]) | (f > br["f_hi"]) | ~torch.isfinite(f)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} filters outside the bracket, first row {int(torch.nonzero(bad)[0])}"


# ---- the application ----------------------------------------------------------------------------------------------------------------
def apply(opacities, scales, filter_3D, raw):
    """Binary64 rule, differentiable.  opacities [P,1], scales [P,3], filter_3D [P,1] (any float dtype: converted)."""
    o, s, f = opacities.to(F64), scales.to(F64), filter_3D.detach().to(F64).reshape(-1, 1)
    on = f > 0
    fs = torch.where(on, f, torch.ones_like(f))
    if raw:
        g = -0.5 * torch.logaddexp(torch.zeros_like(s), 2 * (torch.log(fs) - s))              # log(s / s')
        lc = g.sum(1, keepdim=True)
        x = -torch.expm1(lc)
        o_out = torch.where(o <= 0, o + lc - torch.log1p(torch.exp(o.clamp(max=0)) * x),
                            lc - torch.log(torch.exp(-o.clamp(min=0)) + torch.where(x == 0, torch.ones_like(x), x)))
        o_out = torch.where(x == 0, o, o_out)
        s_out = s - g
    else:
        s_out = torch.hypot(s, fs)
        o_out = o * (s / s_out).prod(1, keepdim=True)
    return torch.where(on, o_out, o), torch.where(on, s_out, s)


def apply_bounds(opacities, scales, filter_3D, g_o, g_s, raw):
    """-> (outputs, gradients, bounds): the binary64 (o', s', dL/do, dL/ds) and the bound of each, K u (sum of term magnitudes)."""
    o = opacities.to(F64).reshape(-1, 1).clone().requires_grad_(True)
    s = scales.to(F64).clone().requires_grad_(True)
    f = filter_3D.to(F64).reshape(-1, 1)
    go, gs = g_o.to(F64).reshape(-1, 1), g_s.to(F64)
    o_out, s_out = apply(o, s, f, raw)
    d_o, d_s = torch.autograd.grad((o_out, s_out), (o, s), (go, gs))
    with torch.no_grad():
        on = f > 0
        fs = torch.where(on, f, torch.ones_like(f))
        sd, od = s.detach(), o.detach()
        if raw:
            t = torch.log(fs) - sd
            g = -0.5 * torch.logaddexp(torch.zeros_like(sd), 2 * t)
            r = torch.sigmoid(-2 * t)
            lc = g.sum(1, keepdim=True)
            x = -torch.expm1(lc)
            log_term = torch.where(od <= 0, torch.log1p(torch.exp(od.clamp(max=0)) * x), od + torch.log(torch.exp(-od.clamp(min=0)) + x + (x == 0)))
            # under EXP_SWITCH w = (f E) E, E = exp(-u/2): 6 roundings where f exp(-u) has 3, so its square has 13, not 7
            deep = (sd < EXP_SWITCH) * K_DEEP
            deep_any = deep.max(1, keepdim=True).values
            b_s = (K_U + deep) * U * (sd.abs() + torch.log(fs).abs() + g.abs())
            b_o = (K_L + deep_any) * U * (od.abs() + lc.abs() + log_term.abs() + 1)
            a = torch.where(od <= 0, (1 + torch.exp(od.clamp(max=0))) / (1 + torch.exp(od.clamp(max=0)) * x),
                            (torch.exp(-od.clamp(min=0)) + 1) / (torch.exp(-od.clamp(min=0)) + x + (x == 0)))
            dl = torch.where(od <= 0, 1 / (1 + torch.exp(od.clamp(max=0)) * x), torch.exp(-od.clamp(min=0)) / (torch.exp(-od.clamp(min=0)) + x + (x == 0)))
            dl = torch.where(x == 0, torch.ones_like(dl), dl)
            b_ds = (K_G + deep_any) * U * ((gs * r).abs() + (go * (1 - r) * a).abs())
            b_do = (K_G + deep_any) * U * (go * dl).abs()
        else:
            so = torch.hypot(sd, fs)
            rho = sd / so
            c = rho.prod(1, keepdim=True)
            b_s = K_S * U * so
            b_o = K_O * U * (od * c).abs()
            others = torch.stack([rho[:, 1] * rho[:, 2], rho[:, 0] * rho[:, 2], rho[:, 0] * rho[:, 1]], 1)
            b_ds = K_G * U * ((gs * rho).abs() + (go * od * others * (1 - rho * rho) / so).abs())
            b_do = K_G * U * (go * c).abs()
        zero = torch.zeros_like
        # a result under binary32's normal range has no relative precision: 2^-120 absolute.  f == 0: bit for bit
        b_s, b_o, b_ds, b_do = (torch.where(on, b + 2.0 ** -120, zero(b)) for b in (b_s, b_o, b_ds, b_do))
    return (o_out.detach(), s_out.detach()), (d_o, d_s), dict(o=b_o, s=b_s, d_o=b_do, d_s=b_ds)


def check_apply(inputs, g_o, g_s, got, raw, what=""):
    """got = (o', s', dL/do, dL/ds) in binary32 (any of the last two may be None) -> the largest error / bound ratio per result."""
    (o_ref, s_ref), (do_ref, ds_ref), b = apply_bounds(*inputs, g_o, g_s, raw)
    ratios = {}
    for name, have, want, bound in (("o", got[0], o_ref, b["o"]), ("s", got[1], s_ref, b["s"]), ("d_o", got[2], do_ref, b["d_o"]),
                                    ("d_s", got[3], ds_ref, b["d_s"])):
        if have is None:
            continue
        have = have.detach().cpu().to(F64).reshape(want.shape)
        assert bool(torch.isfinite(have).all()), f"{what} {name}: not finite"
        err = (have - want).abs()
        exact = bound == 0
        assert bool((err[exact] == 0).all()), f"{what} {name}: a row with f = 0 is not bit for bit"
        ratios[name] = float((err[~exact] / bound[~exact]).max()) if bool((~exact).any()) else 0.0
        print(f"{what} {name}: worst error / bound = {ratios[name]:.3f}")
        assert ratios[name] <= 1.0, f"{what} {name}: error / bound = {ratios[name]:.3f}"
    return ratios


def apply_case(P, seed, raw):
    """Random inputs of a training run's ranges: log-scales U(ln .003, ln .3), logits N(0, 2.5^2), filters log-uniform over
    [1e-3, 1e-1] with every 7th (from row 3) zero, both gradients N(0, 1).  -> (opacities [P,1], scales [P,3], filter [P,1]), g_o, g_s."""
    g = torch.Generator().manual_seed(seed)
    u = torch.rand(P, 3, generator=g) * (math.log(0.3) - math.log(0.003)) + math.log(0.003)
    l = torch.randn(P, 1, generator=g) * 2.5
    f = torch.exp(torch.rand(P, 1, generator=g) * (math.log(1e-1) - math.log(1e-3)) + math.log(1e-3))
    f[3::7] = 0.0
    g_o, g_s = torch.randn(P, 1, generator=g), torch.randn(P, 3, generator=g)
    if raw:
        return (l, u, f), g_o, g_s
    return (torch.sigmoid(l), torch.exp(u), f), g_o, g_s


def extreme_case(raw):
    """Every combination of u in {-50, 0, 50} (one axis, the others 0), f in {0, 1e-6, 1e3} and l in {-30, 0, 30}; then the rows
    that reach the forms' remaining branches: u = -85 on every axis beside f = 1e-36 and 1e-30 (the smallest scales the activated
    mode can hold), in raw mode u = -95 and -90 beside f = 1e-37 and 1e-35 (under EXP_SWITCH: exp(-u) in two halves), and logits of +-100 (e^l beyond binary32) beside a negligible, a small and a dominant filter."""
    rows = [((u, 0.0, 0.0), l, f) for u in (-50.0, 0.0, 50.0) for f in (0.0, 1e-6, 1e3) for l in (-30.0, 0.0, 30.0)]
    rows += [((-85.0, -85.0, -85.0), l, f) for f in (1e-36, 1e-30) for l in (-30.0, 0.0, 30.0)]
    if raw:                    # under EXP_SWITCH (raw mode's own branch; exp(-95) is no binary32 number for the activated mode)
        rows += [((-95.0, -95.0, -90.0), l, f) for f in (1e-37, 1e-35) for l in (-30.0, 0.0, 30.0)]
    rows += [((u, 0.0, 0.0), l, f) for (u, f) in ((50.0, 1e-6), (0.0, 1e-6), (0.0, 1e3)) for l in (-100.0, 100.0)]
    rows += [((50.0, 50.0, 50.0), l, 1e-6) for l in (-100.0, 100.0)]          # c rounds to 1: the 1 + e^l of filter3d_logit
    u = torch.tensor([r[0] for r in rows], dtype=F32)
    l = torch.tensor([[r[1]] for r in rows], dtype=F32)
    f = torch.tensor([[r[2]] for r in rows], dtype=F32)
    if raw:
        return l, u, f
    return torch.sigmoid(l), torch.exp(u), f
