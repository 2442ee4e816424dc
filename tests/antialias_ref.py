"""The opacity compensation of the anti-aliasing switch (include/gsrast.h gsr_opacity_compensation_*), restated in torch from its
formulas: binary64 by default, binary32 on request, differentiable through autograd.  It calls nothing of the package: its own
quaternion -> R, R S S^T R^T, view transform, frustum clamp and J.

    det0 = a0 c0 - b^2     det1 = (a0 + h)(c0 + h) - b^2     x = det0 / det1     rho = sqrt(max(2.5e-5, x))     opacity' = opacity rho

a0, b, c0: the 2D covariance T Sigma T^T before the dilation h = 0.3, T = J R_w2c, J at the view-space point whose tx/tz (ty/tz) is
clamped to 1.3 tanfov.  A Gaussian at view z <= 0.2, or with det1 == 0, passes through.  Raw mode: logits, log-scales, unnormalised
quaternions in, logit(sigmoid(o) rho) out.

Two conventions of the rasterizer's own backward are kept, because the compensation's gradients add to its gradients on the same
tensors (tests/torch_ref.py mirrors them with the same detach() tricks):
  * a clamped tx (ty) passes no gradient (csrc/gsr_math.h xmul / ymul);
  * the gradient of the scales omits the factor scale_modifier.

The error rule of the GPU and host tests (check_against_ref): for every compared tensor, the error against binary64 may not exceed
4 x the worst error of THIS restatement evaluated in binary32 on the same inputs, plus 2^-23 x the tensor's largest magnitude.  The
x4 covers operation order and FMA contraction.
"""
import math

import numpy as np
import torch

F64, F32 = torch.float64, torch.float32
NEAR, FOV_CLAMP, DILATE, MIN_RATIO = 0.2, 1.3, 0.3, 0.000025
GRAD_NAMES = ("opacities", "means3D", "scales", "rotations")


def camera_of(kw):
    """The scalars and the view matrix the rule reads, from raster kwargs (tests/util.py raster_kwargs)."""
    return dict(V=np.asarray(kw["viewmatrix"], np.float64), W=int(kw["image_width"]), H=int(kw["image_height"]),
                tanfovx=float(kw["tanfovx"]), tanfovy=float(kw["tanfovy"]), mod=float(kw["scale_modifier"]))


def rule(opacities, means3D, scales, rotations, cam, raw=False, dtype=F64):
    """-> dict: out (compensated opacity, or logit in raw mode; shaped like opacities), x (clamped at 2.5e-5; 1 where passed through:
    rho^2), rho, through, clamped (bool masks), xmul0 / ymul0 (the frustum clamp acted), z (view depth).  The inputs may require
    grad (they are used as given when already of `dtype`)."""
    t = lambda a: a if isinstance(a, torch.Tensor) and a.dtype == dtype else torch.as_tensor(np.asarray(a), dtype=dtype)
    o_in, p, sc, q = t(opacities), t(means3D), t(scales), t(rotations)
    o = o_in.reshape(-1)
    V = torch.as_tensor(cam["V"], dtype=dtype)
    if raw:
        sc = torch.exp(sc)
        q = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
        op = 1.0 / (1.0 + torch.exp(-o))
    else:
        op = o
    s = (sc * cam["mod"]).detach() + (sc - sc.detach())          # value mod * s, gradient without the factor (A.10)
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = [[1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y)],
         [2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x)],
         [2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)]]
    v = [s[:, k] * s[:, k] for k in range(3)]
    Sig = [[sum(R[i][k] * R[j][k] * v[k] for k in range(3)) for j in range(3)] for i in range(3)]
    pv = [p[:, 0] * V[0, j] + p[:, 1] * V[1, j] + p[:, 2] * V[2, j] + V[3, j] for j in range(3)]
    culled = ~(pv[2] > NEAR)
    tz = torch.where(culled, torch.ones_like(pv[2]), pv[2])
    fx, fy = cam["W"] / (2.0 * cam["tanfovx"]), cam["H"] / (2.0 * cam["tanfovy"])
    limx, limy = FOV_CLAMP * cam["tanfovx"], FOV_CLAMP * cam["tanfovy"]
    rx, ry = pv[0] / tz, pv[1] / tz
    cx, cy = (rx < -limx) | (rx > limx), (ry < -limy) | (ry > limy)
    tx = torch.where(cx, (rx.clamp(-limx, limx) * tz).detach(), pv[0])
    ty = torch.where(cy, (ry.clamp(-limy, limy) * tz).detach(), pv[1])
    J00, J02, J11, J12 = fx / tz, -(fx * tx) / (tz * tz), fy / tz, -(fy * ty) / (tz * tz)
    # T = J R_w2c, R_w2c[i][j] = V[j][i]
    T0 = [J00 * V[k, 0] + J02 * V[k, 2] for k in range(3)]
    T1 = [J11 * V[k, 1] + J12 * V[k, 2] for k in range(3)]
    S0 = [sum(Sig[k][l] * T0[l] for l in range(3)) for k in range(3)]
    S1 = [sum(Sig[k][l] * T1[l] for l in range(3)) for k in range(3)]
    a0 = sum(T0[k] * S0[k] for k in range(3))
    b = sum(T0[k] * S1[k] for k in range(3))
    c0 = sum(T1[k] * S1[k] for k in range(3))
    det0 = a0 * c0 - b * b
    det1 = (a0 + DILATE) * (c0 + DILATE) - b * b
    through = culled | (det1 == 0)
    ratio = det0 / torch.where(through, torch.ones_like(det1), det1)
    clamped = ~through & ~(ratio > MIN_RATIO)
    xc = torch.where(clamped, torch.full_like(ratio, MIN_RATIO), ratio)
    xc = torch.where(through, torch.ones_like(xc), xc)
    rho = torch.sqrt(xc)
    pp = op * rho
    out = torch.where(through, o, torch.log(pp) - torch.log1p(-pp) if raw else pp)
    return dict(out=out.reshape(o_in.shape), x=xc, rho=rho, through=through, clamped=clamped, xmul0=cx & ~culled, ymul0=cy & ~culled,
                z=pv[2])


def evaluate(inputs, cam, g, raw=False, dtype=F64):
    """inputs: (opacities, means3D, scales, rotations) arrays / tensors; g: dL/dout.  -> (rule dict, {name: gradient}) in `dtype`."""
    leaves = [torch.as_tensor(np.asarray(a), dtype=dtype).clone().requires_grad_(True) for a in inputs]
    res = rule(*leaves, cam, raw=raw, dtype=dtype)
    gt = torch.as_tensor(np.asarray(g), dtype=dtype).reshape(res["out"].shape)
    grads = torch.autograd.grad(res["out"], leaves, gt)
    return res, dict(zip(GRAD_NAMES, grads))


def bound(ref64, ref32):
    """The error allowed against ref64 for a tensor whose binary32 restatement is ref32."""
    ref64 = ref64.detach().to(F64)
    worst32 = float((ref32.detach().to(F64) - ref64).abs().max()) if ref64.numel() else 0.0
    return 4.0 * worst32 + 2.0 ** -23 * (float(ref64.abs().max()) if ref64.numel() else 0.0), worst32


def check_against_ref(inputs, cam, g, got_out, got_grads, raw=False, what="", report=None):
    """got_out / got_grads: the compensated opacities and {name: gradient} of the implementation under test (binary32) on `inputs`.
    Holds out, x = rho^2 (derived from got_out and the input opacity) and the four gradients to the rule in the module docstring;
    prints both worst errors of each.  Returns the binary64 rule dict."""
    r64, g64 = evaluate(inputs, cam, g, raw, F64)
    r32, g32 = evaluate(inputs, cam, g, raw, F32)
    assert torch.equal(r64["through"], r32["through"]) and torch.equal(r64["clamped"], r32["clamped"]), \
        f"{what}: a Gaussian sits within binary32 rounding of a threshold of the rule: move it"
    assert torch.equal(r64["xmul0"], r32["xmul0"]) and torch.equal(r64["ymul0"], r32["ymul0"]), f"{what}: ... of the frustum clamp"
    o64 = torch.as_tensor(np.asarray(inputs[0]), dtype=F64).reshape(-1)
    got = torch.as_tensor(np.asarray(got_out)).to(F64).reshape(-1)
    if raw:
        sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
        x_got = (sig(got) / sig(o64)) ** 2
    else:
        x_got = (got / o64) ** 2
    rows = [("x", r64["x"], r32["x"], x_got), ("out", r64["out"].reshape(-1), r32["out"].reshape(-1), got)]
    rows += [("d " + n, g64[n], g32[n], torch.as_tensor(np.asarray(got_grads[n])).to(F64).reshape(g64[n].shape)) for n in GRAD_NAMES]
    for name, w64, w32, have in rows:
        w64, w32 = w64.detach(), w32.detach()
        tol, worst32 = bound(w64, w32)
        err = float((have - w64).abs().max()) if have.numel() else 0.0
        line = f"{what} {name:12s} err {err:.3e}  binary32 restatement {worst32:.3e}  bound {tol:.3e}  max|ref| {float(w64.abs().max()) if have.numel() else 0.0:.3e}"
        print(line)
        if report is not None:
            report.append((what, name, err, worst32, tol))
        assert err <= tol, line
    return r64


# ---- scenes of the GPU and host tests -----------------------------------------------------------------------------------------------
def scene_cases():
    """name -> (scene in world coordinates, camera, scale_modifier): the shapes of the issue's item 1.  scene_synth scenes are generated
    in view space; `posed` places one in front of a camera whose view matrix has no zero entry; `xclamp` moves 24 Gaussians of the
    2048-Gaussian scene to |x/z| in (1.3, 1.5) tanfovx with large scales, so that the clamp's xmul = 0 branch runs."""
    import posed as PO
    import scene_synth as S
    cases = {}
    base = lambda **k: S.make_scene(2048, 128, 128, 3, 105, **k)
    cam = S.make_camera(128, 128)
    cases["p2048"] = (base(), cam, 1.0)
    cases["p2048_small"] = (base(scale_lo=0.0003), cam, 1.0)
    cases["p64"] = (S.make_scene(64, 48, 80, 2, 103), S.make_camera(48, 80), 1.0)
    pcam = PO.posed_camera(128, 128, "a")
    cases["posed"] = (PO.to_world(base(), pcam), pcam, 1.0)
    cases["mod0.5"] = (base(), cam, 0.5)
    sc = base()
    g = torch.Generator().manual_seed(7)
    tanx = math.tan(cam.FoVx * 0.5)
    z = sc.means3D[:, 2]
    idx = torch.nonzero((z > 1.0) & (z < 4.0)).reshape(-1)[:24]
    ratio = (1.32 + 0.16 * torch.rand(24, generator=g)) * torch.where(torch.rand(24, generator=g) < 0.5, -1.0, 1.0)
    sc.means3D[idx, 0] = ratio * tanx * sc.means3D[idx, 2]
    # sigma of 0.2 .. 0.35 of the image width: alpha >= 1/255 reaches well inside the frame from 0.3 .. 0.5 widths outside it
    sc.log_scales[idx] = torch.log((0.4 + 0.3 * torch.rand(24, 1, generator=g)) * tanx * sc.means3D[idx, 2:3]) + 0.1 * torch.randn(24, 3, generator=g)
    cases["xclamp"] = (sc, cam, 1.0)
    return cases


def case_inputs(scene, raw):
    """(opacities, means3D, scales, rotations) float32 tensors of a scene: the raw leaves, or their activations."""
    if raw:
        return scene.opacity_logits, scene.means3D, scene.log_scales, scene.raw_rotations
    a = scene.activated()
    return a["opacities"], a["means3D"], a["scales"], a["rotations"]


def upstream(P, seed):
    """dL/dout [P], exactly zero on about a third of the rows (the backward kernel writes those without running the chain)."""
    g = torch.Generator().manual_seed(1000 + seed)
    v = torch.randn(P, generator=g, dtype=F64)
    return torch.where(torch.rand(P, generator=g) < 0.3, torch.zeros_like(v), v)
