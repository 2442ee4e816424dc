"""Binary64 references for the camera gradients (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos), two tiers.

Tier A, end to end, small frames: torch_ref.render_autograd with the three camera tensors as leaves; autograd through the whole
blend (tier_a).

Tier B, any size: per-Gaussian screen-space gradient rows (the oracle's backward_screen; for an aux frame also dL/dz, the channel-0
colour gradient of the colors_precomp = (z, 1, 0) frame) contracted with d(ndc, conic, rgb, z) / d(camera) of a torch restatement
of the projection (project) that keeps A.10's three conventions: a clamped tx/tz (ty/tz) is detached, the conic's derivative
carries den^2 / (den^2 + 1e-7), and the stored gB is half the derivative w.r.t. the scalar B (the chain takes 2 gB).  The camera
tensors are expanded per Gaussian (V.expand(n, 4, 4).clone()), so that .grad holds every Gaussian's own contribution t_i: tier_b
returns sum_i t_i and A = sum_i |t_i| entry by entry.  The sums cancel (A / |sum| of several hundred on deep frames), which is
why the GPU tests bound the error by A and not by the tensor's largest entry.
"""
from __future__ import annotations

import numpy as np
import torch

from torch_ref import eval_sh_basis, quat_to_rot, render_autograd

NAMES = ("viewmatrix", "projmatrix", "campos")
SETTINGS = ("image_height", "image_width", "tanfovx", "tanfovy", "scale_modifier", "sh_degree")


def project(V, PV, cp, kw, sel, dt):
    """(ndc [n,2], conic [n,3], rgb [n,3], z [n]) of the Gaussians `sel` of kw, each with its own camera V [n,4,4], PV [n,4,4],
    cp [n,3]; A.1-A.6 in dtype dt with the gradient conventions of A.10."""
    t = lambda a: torch.as_tensor(np.asarray(a)[sel], dtype=dt)
    H, W = int(kw["image_height"]), int(kw["image_width"])
    tanfovx, tanfovy = float(kw["tanfovx"]), float(kw["tanfovy"])
    m = t(kw["means3D"])
    n = m.shape[0]
    ph = torch.cat([m, torch.ones(n, 1, dtype=dt)], 1)
    pv = torch.einsum("nr,nrc->nc", ph, V)
    hom = torch.einsum("nr,nrc->nc", ph, PV)
    ndc = hom[:, :2] / (hom[:, 3:4] + 1e-7)
    if kw.get("cov3D_precomp") is None:
        L = quat_to_rot(t(kw["rotations"])) @ torch.diag_embed(t(kw["scales"]) * float(kw["scale_modifier"]))
        Sigma = L @ L.transpose(1, 2)
    else:
        c = t(kw["cov3D_precomp"])
        Sigma = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4], c[:, 5]], 1).view(-1, 3, 3)
    fx, fy = W / (2 * tanfovx), H / (2 * tanfovy)
    limx, limy = 1.3 * tanfovx, 1.3 * tanfovy
    tz = pv[:, 2]
    txtz, tytz = pv[:, 0] / tz, pv[:, 1] / tz
    cx, cy = (txtz < -limx) | (txtz > limx), (tytz < -limy) | (tytz > limy)
    tx = torch.where(cx, (txtz.clamp(-limx, limx) * tz).detach(), pv[:, 0])
    ty = torch.where(cy, (tytz.clamp(-limy, limy) * tz).detach(), pv[:, 1])
    zero = torch.zeros_like(tz)
    J = torch.stack([fx / tz, zero, -fx * tx / (tz * tz), zero, fy / tz, -fy * ty / (tz * tz)], 1).view(-1, 2, 3)
    T = J @ V[:, :3, :3].transpose(1, 2)
    cov2 = T @ Sigma @ T.transpose(1, 2)
    a, b, c_ = cov2[:, 0, 0] + 0.3, cov2[:, 0, 1], cov2[:, 1, 1] + 0.3
    det = a * c_ - b * b
    kfix = (det * det / (det * det + 1e-7)).detach()
    con = torch.stack([c_ / det, -b / det, a / det], 1)
    con = con.detach() + kfix[:, None] * (con - con.detach())
    if kw.get("colors_precomp") is None:
        d = m - cp
        d = d / d.norm(dim=1, keepdim=True)
        D = int(kw["sh_degree"])
        rgb = torch.einsum("pk,pkc->pc", eval_sh_basis(D, d), t(kw["shs"])[:, :(D + 1) ** 2, :]) + 0.5
        rgb = torch.clamp_min(rgb, 0.0)
    else:
        rgb = t(kw["colors_precomp"]) + 0 * cp
    return ndc, con, rgb, pv[:, 2]


def tier_b(kw, screen, radii, dz=None, dtype=torch.float64):
    """({name: sum_i t_i}, {name: A = sum_i |t_i|}, {name: t [n, ...]}, sel) in binary64 numpy, the contraction evaluated in
    `dtype`.  screen [P, >= 9]: (dmean2D.x, dmean2D.y, gA, gB, gC, dopacity, drgb[3]); dz [P] or None: dL/dz (an aux frame);
    radii [P]: Gaussians with radius 0 take no part."""
    sel = np.nonzero(np.asarray(radii) > 0)[0]
    n = sel.size
    ex = lambda a, *shape: torch.as_tensor(np.asarray(a), dtype=dtype).reshape(*shape).expand(n, *shape).clone().requires_grad_(True)
    V, PV, cp = ex(kw["viewmatrix"], 4, 4), ex(kw["projmatrix"], 4, 4), ex(kw["campos"], 3)
    out_sum, out_abs, terms = {}, {}, {}
    if n:
        ndc, con, rgb, z = project(V, PV, cp, kw, sel, dtype)
        sg = torch.as_tensor(np.asarray(screen)[sel], dtype=dtype)
        S = (sg[:, 0:2] * ndc).sum() + (sg[:, 2] * con[:, 0] + 2 * sg[:, 3] * con[:, 1] + sg[:, 4] * con[:, 2]).sum() + \
            (sg[:, 6:9] * rgb).sum()
        if dz is not None:
            S = S + (torch.as_tensor(np.asarray(dz)[sel], dtype=dtype) * z).sum()
        S.backward()
    for name, leaf in zip(NAMES, (V, PV, cp)):
        t = (leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)).double().numpy()
        terms[name] = t
        out_sum[name], out_abs[name] = t.sum(0), np.abs(t).sum(0)
    return out_sum, out_abs, terms, sel


def tier_a_leaves(kw):
    """kw's tensors in binary64; viewmatrix, projmatrix and campos as leaves that require grad."""
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    out = {k: (t(v) if isinstance(v, (np.ndarray, torch.Tensor)) else v) for k, v in kw.items()}
    for name in NAMES:
        out[name] = out[name].clone().requires_grad_(True)
    return out


def tier_a(kw, grad_color, grad_depth=None, grad_alpha=None):
    """{name: dL/dname} by autograd through torch_ref.render_autograd for L = <grad_color, C> (+ <grad_depth, depth> +
    <grad_alpha, alpha> of the aux frame: colors_precomp = (z, 1, 0), bg = 0, z built from the viewmatrix leaf in the same
    graph, so autograd carries the depth's chain into dL/dviewmatrix)."""
    tk = tier_a_leaves(kw)
    g = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float64)
    loss = 0.0
    if grad_color is not None:
        color = render_autograd(**tk)[0]
        loss = loss + (color * g(grad_color)).sum()
    if grad_depth is not None or grad_alpha is not None:
        m = tk["means3D"]
        z = (torch.cat([m, torch.ones(m.shape[0], 1, dtype=torch.float64)], 1) @ tk["viewmatrix"])[:, 2]
        akw = {k: v for k, v in tk.items() if k not in ("shs", "colors_precomp", "bg")}
        color, _, _, Tacc = render_autograd(colors_precomp=torch.stack([z, torch.ones_like(z), torch.zeros_like(z)], 1),
                                            bg=torch.zeros(3, dtype=torch.float64), **akw)
        if grad_depth is not None:
            loss = loss + (color[0] * g(grad_depth)).sum()
        if grad_alpha is not None:
            loss = loss + ((1 - Tacc) * g(grad_alpha)).sum()
    loss.backward()
    return {name: (tk[name].grad if tk[name].grad is not None else torch.zeros_like(tk[name])).numpy() for name in NAMES}


def oracle_rows(kw, grad_color, grad_depth=None, grad_alpha=None, dtype=np.float64, order="back_to_front", parallel=False,
                backward_parallel=None):
    """(screen [P,9], dz [P] or None, radii) from the oracle in `dtype`: the colour frame's rows for grad_color, plus (aux) the rows
    of the colors_precomp = (z, 1, 0), bg = 0 frame for dL/dcolor = (grad_depth, grad_alpha, 0), whose channel-0 colour gradient is
    dL/dz.  The aux frame's colour gradients of channels 1, 2 belong to constants and are dropped."""
    import oracle
    bpar = parallel if backward_parallel is None else backward_parallel      # (the forward's pixels do not depend on it)
    screen, dz, radii = None, None, None
    if grad_color is not None:
        fr = oracle.rasterize(dtype=dtype, parallel=parallel, **kw)
        screen, radii = fr.backward_screen(np.asarray(grad_color), parallel=bpar, order=order).astype(np.float64), fr.radii
    if grad_depth is not None or grad_alpha is not None:
        V = np.asarray(kw["viewmatrix"], np.float64)
        z = np.asarray(kw["means3D"], np.float64) @ V[:3, 2] + V[3, 2]
        akw = {k: v for k, v in kw.items() if k != "shs"}
        akw.update(colors_precomp=np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), bg=np.zeros(3))
        fa = oracle.rasterize(dtype=dtype, parallel=parallel, **akw)
        H, W = int(kw["image_height"]), int(kw["image_width"])
        zero = np.zeros((H, W))
        ga = np.stack([zero if grad_depth is None else np.asarray(grad_depth, np.float64).reshape(H, W),
                       zero if grad_alpha is None else np.asarray(grad_alpha, np.float64).reshape(H, W), zero])
        sa = fa.backward_screen(ga, parallel=bpar, order=order).astype(np.float64)
        dz = sa[:, 6].copy()
        sa[:, 6:9] = 0.0
        screen = sa if screen is None else screen + sa
        radii = fa.radii
    return screen, dz, radii


def yard32(kw, grad_color, want64, grad_depth=None, grad_alpha=None, parallel=False):
    """{name: entry-wise |binary32 tier B - want64|}, the larger of the oracle's two binary32 backward orders: what a correct
    binary32 implementation of the same sums reaches (gradcheck.yardstick's idea, for the camera tensors).  Always the oracle's
    serial backward: its parallel one adds in an order that changes from run to run, and in binary32 the yardstick would move
    with it; this way the bound is a fixed function of the frame."""
    out = {n: np.zeros_like(np.asarray(want64[n], np.float64)) for n in NAMES}
    for order in ("back_to_front", "front_to_back"):
        screen, dz, radii = oracle_rows(kw, grad_color, grad_depth, grad_alpha, np.float32, order, parallel, backward_parallel=False)
        got = tier_b(kw, screen, radii, dz, dtype=torch.float32)[0]
        for n in NAMES:
            out[n] = np.maximum(out[n], np.abs(got[n] - np.asarray(want64[n], np.float64)))
    return out


# Pose recovery (tests/test_gpu_camera_grad.py::test_pose_recovery and its CPU rehearsal tools/camera_pose_rehearsal.py)
POSE_START = dict(rot=(0.012, -0.010, 0.008), trans=(0.012, -0.012, 0.010))      # ~1.0 degree, ~0.02 scene units
POSE_LR, POSE_STEPS = 1e-3, 150          # rehearsed on the CPU

F_YARD = 32.0          # twice the measured worst on an MI355X, rounded up to a power of two.  Measured worst e / max(yard32, 1e-7 A)
#                        over every entry of tests/test_gpu_camera_grad.py: 12.5 (the 300-Gaussian frame at pose "b", SH degree 0,
#                        dL/dviewmatrix), with the yardstick from the oracle's serial binary32 backward (yard32 below)


def check_camera_grads(got, want, A, yard, label="", f_yard=None, cap=1e-4, needs=(True, True, True)):
    """Bounds 1 and 2 of the GPU tests, entry-wise with e = |got - want|:   e <= cap A   and   e <= F max(yard32, 1e-7 A).
    Entries with A = 0 must be exact zeros (and are counted and printed).  needs: which of the three tensors required grad; a
    missing (None) gradient of one that did is a failure, and one that did not must have none.  Prints the worst ratios before
    it asserts; returns the worst e / max(yard32, 1e-7 A)."""
    f_yard = F_YARD if f_yard is None else f_yard
    worst, zeros, fails = 0.0, 0, []
    for n, need in zip(NAMES, needs):
        if not need:
            assert got.get(n) is None, f"{label}: {n} did not require grad but got a gradient"
            continue
        assert got.get(n) is not None, f"{label}: {n} requires grad and got None back"
        g, w = np.asarray(got[n], np.float64).reshape(np.shape(want[n])), np.asarray(want[n], np.float64)
        a, y = np.asarray(A[n], np.float64), np.asarray(yard[n], np.float64)
        e = np.abs(g - w)
        z = a == 0
        zeros += int(z.sum())
        if (g[z] != 0).any():
            fails.append(f"{n}: {int((g[z] != 0).sum())} entries with A = 0 are not exact zeros")
        nz = ~z
        r1 = (e[nz] / a[nz]).max(initial=0.0)
        r2 = (e[nz] / np.maximum(y[nz], 1e-7 * a[nz])).max(initial=0.0)
        worst = max(worst, r2)
        print(f"  {label} {n:10s} max e/A {r1:.3e} (cap {cap:g})  max e/max(yard32, 1e-7 A) {r2:.2f} (F {f_yard:g})  "
              f"max A/|want| {(a[nz] / np.maximum(np.abs(w[nz]), 1e-300)).max(initial=0.0):.1f}")
        if r1 > cap:
            fails.append(f"{n}: e/A {r1:.3e} > {cap:g}")
        if r2 > f_yard:
            fails.append(f"{n}: e / max(yard32, 1e-7 A) {r2:.2f} > F = {f_yard:g}")
    print(f"  {label} entries with A = 0 (checked for exact zero): {zeros}")
    assert not fails, f"{label}: " + "; ".join(fails)
    return worst
