"""Camera gradients (dL/dviewmatrix, dL/dprojmatrix, dL/dcampos) on the GPU, against the binary64 references of tests/camera_ref.py.

The camera gradient is a sum over Gaussians that cancels (A / |sum| of several hundred per entry on deep frames, A = sum_i |t_i| of
the per-Gaussian terms), so a flat bound relative to the tensor's largest entry fails a correct binary32 implementation.  Entry-wise,
with e = |got - want| (camera_ref.check_camera_grads):
  1. e <= 1e-4 A: the project's promise (every Gaussian's gradient within 1e-4 of its own scale) carried through the sum; entries
     with A = 0 are exact zeros (4 + 4 structural ones, + 3 with colors_precomp; the count is printed);
  2. e <= F max(yard32, 1e-7 A): yard32 = the same tier-B sum evaluated in binary32 from the binary32 oracle (both backward orders,
     the larger error); F = camera_ref.F_YARD = 32, twice the measured worst ratio (12.5) rounded up to a power of two.
Measured on an MI355X over every case below: worst e / A 4.8e-6, worst e / max(yard32, 1e-7 A) 12.5.
A gradient that comes back None for a tensor that requires grad fails the check (camera_ref.check_camera_grads).
dL/dcolor is zero on the oracle's fragile pixels for both sides, so no term rides on a decision binary32 may take the other way.
"""
import numpy as np
import pytest
import torch

import camera_ref as CR
import oracle
import posed as PO
import scene_synth as S
from test_gpu_parity import DEV, _inputs, _settings
from util import cov3d_from, raster_kwargs

pytestmark = pytest.mark.gpu
W, H = 64, 48


def _t(a, grad=False):
    return torch.as_tensor(np.asarray(a), dtype=torch.float32).to(DEV).requires_grad_(grad)


def _cam_settings(kw, needs=(True, True, True), debug=False):
    rs = _settings(kw, debug)
    cams = [getattr(rs, n).detach().clone().requires_grad_(bool(k)) for n, k in zip(CR.NAMES, needs)]
    return rs._replace(viewmatrix=cams[0], projmatrix=cams[1], campos=cams[2]), cams


def _render(kw, needs=(True, True, True), depth_alpha=False, debug=False, scene_grad=True):
    from diff_gaussian_rasterization import GaussianRasterizer
    rs, cams = _cam_settings(kw, needs, debug)
    inp = _inputs(kw, scene_grad)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=scene_grad)
    out = GaussianRasterizer(rs, depth_alpha=depth_alpha)(means2D=means2D, **inp)
    return out, cams, inp, means2D


def _cam_grads(cams):
    return {n: (None if c.grad is None else c.grad.detach().cpu().numpy()) for n, c in zip(CR.NAMES, cams)}


def _strict(kw, parallel=False):
    return oracle.rasterize(dtype=np.float64, parallel=parallel, **kw).fragile_px == 0


def _reference(kw, gc, gz=None, ga=None, parallel=False, tier_a=False):
    """(want, A, yard32): binary64 sums (tier B; tier A when asked, after checking that the two agree), A = sum |t_i|, and the
    binary32 yardstick."""
    screen, dz, radii = CR.oracle_rows(kw, gc, gz, ga, parallel=parallel)
    want, A, _, sel = CR.tier_b(kw, screen, radii, dz)
    if tier_a:
        a = CR.tier_a(kw, gc, gz, ga)
        for n in CR.NAMES:
            assert np.abs(a[n] - want[n]).max() <= 1e-12 * max(np.abs(a[n]).max(), 1e-300) + 1e-300, n
        want = a
    return want, A, CR.yard32(kw, gc, want, gz, ga, parallel=parallel), sel


def _small_kwargs(pose, D, seed, P=300, mode="sh", scale_modifier=1.0):
    cam = PO.posed_camera(W, H, pose)
    scene = PO.to_world(S.make_scene(P, W, H, D, seed, scale_lo=0.02, scale_hi=0.2), cam)
    a = scene.activated()
    extra = {}
    if mode == "color":
        extra["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    if mode == "cov":
        extra["cov3D_precomp"] = cov3d_from(a["scales"], a["rotations"], scale_modifier)
    return raster_kwargs(scene, cam, bg=(0.1, 0.2, 0.3), scale_modifier=scale_modifier, **extra)


def _edge_kwargs():
    cam = PO.posed_camera(W, H, "b")
    return raster_kwargs(PO.edge_scene(W, H, cam, 7, 100, dict(clamp_x=12, clamp_y=12, clamp_xy=10, near=16, culled=12,
                                                               needle_disc=32, opaque=32, sh_clamp=32))[0], cam)


# the CPU list of tests/test_camera_grad_ref.py: three poses x SH degree 0..3, then the input modes and the edge populations
SMALL = {f"pose {pose} D{D}": (lambda pose=pose, D=D: _small_kwargs(pose, D, 40 + D)) for pose in "abc" for D in range(4)}
SMALL.update({"colors_precomp": lambda: _small_kwargs("a", 2, 51, mode="color"), "cov3D_precomp": lambda: _small_kwargs("a", 2, 51, mode="cov"),
              "scale_modifier 0.7": lambda: _small_kwargs("a", 2, 51, scale_modifier=0.7), "edge scene": _edge_kwargs})


@pytest.mark.parametrize("case", list(SMALL))
def test_small_frames_against_tier_a(case):
    kw = SMALL[case]()
    gc = S.make_grad_image(W, H, 3).numpy().astype(np.float64) * _strict(kw)[None]
    want, A, yard, sel = _reference(kw, gc, tier_a=True)
    (color, radii), cams, inp, _ = _render(kw)
    color.backward(_t(gc))
    got = _cam_grads(cams)
    CR.check_camera_grads(got, want, A, yard, label=case)
    assert (got["viewmatrix"][:, 3] == 0).all() and (got["projmatrix"][:, 2] == 0).all()
    if case == "colors_precomp":
        assert (got["campos"] == 0).all()
    assert np.abs(got["viewmatrix"]).max() > 0 and np.abs(got["projmatrix"]).max() > 0


def _deep_small():
    import gradcheck as GC
    c = GC.DEEP_SMALL
    cam = PO.posed_camera(c["W"], c["H"], "a")
    scene = PO.to_world(S.make_scene(c["P"], c["W"], c["H"], c["D"], c["seed"], scale_lo=c["scale_lo"], scale_hi=c["scale_hi"],
                                     zmin=c["zmin"]), cam)
    return scene, cam


def _uncovered_half_posed():
    from test_gpu_parity import _uncovered_half_posed as f
    return f()


def _plan_of(kw):
    """The plan of the frame through the standard API (plain settings, activated inputs).  The sparse / dense assertion made from it
    is the mirror of the library's host-side decision (effective_binned_ranks * 4 < P, gsr_backward_camera's and gsr_backward_geom's
    own expression) for this scene, not an observation of which kernel ran; the render() and FUSE_GETTERS routes render the same
    scene and plan the same chunks."""
    import diff_gaussian_rasterization as dgr
    inp = _inputs(kw, False)
    _, _, fr = dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, _settings(kw))
    torch.cuda.synchronize()
    return fr.plan


_BIG = {}


def _big(name):
    """(scene, cam, kw, masked dL/dcolor, want, A, yard32) of a full-size frame, computed once per session."""
    if name not in _BIG:
        if name.startswith("cfg"):
            c = S.CONFIGS[name.split()[0]]
            cam = PO.posed_camera(c["W"], c["H"], "a")
            scene = PO.to_world(S.make_config(name.split()[0])[0], cam)
        else:
            scene, cam = _deep_small() if name == "deep small" else _uncovered_half_posed()
        kw = raster_kwargs(scene, cam)
        Wb, Hb = kw["image_width"], kw["image_height"]
        gc = S.make_grad_image(Wb, Hb, 1).numpy().astype(np.float64) * _strict(kw, parallel=True)[None]
        want, A, yard, sel = _reference(kw, gc, parallel=True)
        assert sel.size > 1000 and all(np.abs(want[n]).max() > 0 for n in CR.NAMES)
        _BIG[name] = (scene, cam, kw, gc, want, A, yard)
    return _BIG[name]


@pytest.mark.parametrize("name,sparse", [("deep small", False), ("uncovered half posed", True), ("cfg3n posed", False),
                                         ("cfg3 posed", True)])
@pytest.mark.parametrize("route", ["forward", "render", "fuse_getters"])
def test_full_size_frames_against_tier_b(name, sparse, route):
    """The deep small frame at pose "a" (dense geometry backward; 103 022 live Gaussians), the posed frame with an uncovered half
    (every chunk runs, the late ones live-filtered: the sparse path through order / cnt_open), and cfg3n (dense) and cfg3 (sparse: a
    few thousand live Gaussians) placed in front of the posed camera "a"; each through forward (activated inputs), render() with
    scene.GaussianModel (forward_raw, raw mode 2) and FUSE_GETTERS (raw mode 1).  Which path runs is the plan's (see _plan_of)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    scene, cam, kw, gc, want, A, yard = _big(name)
    plan = _plan_of(kw)
    assert (N.effective_binned_ranks(plan) * 4 < scene.P) == sparse, (N.effective_binned_ranks(plan), scene.P)
    if route == "forward":
        (color, radii), cams, _, _ = _render(kw)
    elif route == "render":
        from gaussian_params import Pipe
        from gaussian_renderer import render
        from scene import GaussianModel
        gm = GaussianModel(scene.sh_degree)
        gm.adopt_scene(scene, device=DEV)
        c = cam.to(DEV)
        cams = [c.world_view_transform.requires_grad_(True), c.full_proj_transform.requires_grad_(True), c.camera_center.requires_grad_(True)]
        color = render(c, gm, Pipe(), torch.zeros(3, device=DEV))["render"]
    else:
        rs, cams = _cam_settings(kw)
        s = scene.to(DEV)
        leaves = [t.detach().clone().requires_grad_(True) for t in (s.means3D, s.shs[:, :1].contiguous(), s.shs[:, 1:].contiguous(),
                                                                    s.opacity_logits, s.log_scales, s.raw_rotations)]
        xyz, dc, rest, op, sc, rot = leaves
        old = dgr.FUSE_GETTERS
        dgr.FUSE_GETTERS = True
        try:
            color, _ = dgr.GaussianRasterizer(rs)(means3D=xyz, means2D=torch.zeros_like(xyz, requires_grad=True), opacities=torch.sigmoid(op),
                                                  shs=torch.cat((dc, rest), 1), scales=torch.exp(sc),
                                                  rotations=torch.nn.functional.normalize(rot))
            assert type(color.grad_fn).__name__.startswith("_RasterizeGaussiansRaw"), type(color.grad_fn).__name__
        finally:
            dgr.FUSE_GETTERS = old
    color.backward(_t(gc))
    for n, c in zip(CR.NAMES, cams):
        assert isinstance(c.grad, torch.Tensor) and c.grad.shape == c.shape, f"{route}: no gradient for {n}"
    CR.check_camera_grads(_cam_grads(cams), want, A, yard, label=f"{name} / {route}")


def test_aux_frame():
    """Loss on colour + depth + alpha: dL/dviewmatrix includes the z chain (tier B with dz); the same frame with only a colour loss
    gives the plain frame's camera gradient bit for bit.  Dense (small frame) and sparse (the uncovered half)."""
    for name in ("small", "uncovered half posed"):
        big = name != "small"
        kw = _big(name)[2] if big else _small_kwargs("c", 3, 61, P=400)
        Wb, Hb = kw["image_width"], kw["image_height"]
        strict = _strict(kw, parallel=big)
        V = np.asarray(kw["viewmatrix"], np.float64)
        z = np.asarray(kw["means3D"], np.float64) @ V[:3, 2] + V[3, 2]
        akw = {k: v for k, v in kw.items() if k != "shs"}
        akw.update(colors_precomp=np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), bg=np.zeros(3))
        strict = strict & _strict(akw, parallel=big)
        g = torch.Generator().manual_seed(9)
        gz = (torch.rand(Hb, Wb, generator=g, dtype=torch.float64) - 0.5).numpy() / float(np.abs(z).max()) * strict
        ga = (torch.rand(Hb, Wb, generator=g, dtype=torch.float64) - 0.5).numpy() * strict
        gc = S.make_grad_image(Wb, Hb, 6).numpy().astype(np.float64) * strict[None]
        want, A, yard, _ = _reference(kw, gc, gz, ga, parallel=big, tier_a=not big)
        (color, radii, depth, alpha), cams, _, _ = _render(kw, depth_alpha=True)
        torch.autograd.backward([color, depth, alpha], [_t(gc), _t(gz)[None], _t(ga)[None]])
        assert all(isinstance(c.grad, torch.Tensor) for c in cams)
        got = _cam_grads(cams)
        CR.check_camera_grads(got, want, A, yard, label=f"aux {name}")
        (color, radii, depth, alpha), cams1, _, _ = _render(kw, depth_alpha=True)
        color.backward(_t(gc))
        (color0, _), cams0, _, _ = _render(kw)
        color0.backward(_t(gc))
        for a, b in zip(cams1, cams0):
            assert torch.equal(a.grad, b.grad)
        assert not np.array_equal(_cam_grads(cams1)["viewmatrix"], got["viewmatrix"])


def test_structure_and_partial_needs():
    kw = _small_kwargs("a", 3, 43)
    gc = _t(S.make_grad_image(W, H, 3))
    (color, _), cams, _, _ = _render(kw)
    color.backward(gc)
    assert (cams[0].grad[:, 3] == 0).all() and (cams[1].grad[:, 2] == 0).all() and cams[2].grad.abs().max() > 0
    (c1, _), only_v, _, _ = _render(kw, needs=(True, False, False))
    c1.backward(gc)
    assert only_v[1].grad is None and only_v[2].grad is None and torch.equal(only_v[0].grad, cams[0].grad)
    (c2, _), only_c, _, _ = _render(kw, needs=(False, False, True), scene_grad=False)          # tracking: the scene is fixed
    c2.backward(gc)
    assert only_c[0].grad is None and torch.equal(only_c[2].grad, cams[2].grad)
    (c3, _), cpre, _, _ = _render(_small_kwargs("a", 2, 51, mode="color"))
    c3.backward(gc)
    assert (cpre[2].grad == 0).all() and cpre[0].grad.abs().max() > 0


def test_nothing_else_moves_and_the_sums_are_reproducible():
    for kw in (_small_kwargs("b", 3, 45, P=2000), _big("uncovered half posed")[2]):
        gc = _t(S.make_grad_image(kw["image_width"], kw["image_height"], 2))
        (c0, r0), _, inp0, m0 = _render(kw, needs=(False, False, False))
        c0.backward(gc)
        (c1, r1), cams, inp1, m1 = _render(kw)
        c1.backward(gc, retain_graph=True)
        assert torch.equal(c0, c1) and torch.equal(r0, r1) and torch.equal(m0.grad, m1.grad)
        for k in inp0:
            assert torch.equal(inp0[k].grad, inp1[k].grad), k
        first = [c.grad.clone() for c in cams]
        for c in cams:
            c.grad = None
        c1.backward(gc)
        (c2, _), cams2, _, _ = _render(kw)
        c2.backward(gc)
        for a, b, c in zip(first, cams, cams2):
            assert torch.equal(a, b.grad) and torch.equal(a, c.grad)
        assert first[0].abs().max() > 0


def test_translation_identity_on_the_device():
    """Camera gradients chained to the centre c (V[3, :3] = -c V[:3, :3], PV = V P, campos = c) against minus the binary64 host sum
    of the device's own dL/dmeans3D rows.  Both sides are within bound 1 of the same per-Gaussian terms: 2e-4 sum_i |dL/dmeans3D_i|."""
    for kw in (_small_kwargs("a", 3, 43, P=2000), _big("deep small")[2]):
        gc = _t(S.make_grad_image(kw["image_width"], kw["image_height"], 2))
        (color, _), cams, inp, _ = _render(kw)
        color.backward(gc)
        g = _cam_grads(cams)
        V, PV = np.asarray(kw["viewmatrix"], np.float64), np.asarray(kw["projmatrix"], np.float64)
        R, Pm = V[:3, :3], np.linalg.inv(V) @ PV
        dc = g["campos"].astype(np.float64) - (g["viewmatrix"].astype(np.float64)[3, :3] +
                                               g["projmatrix"].astype(np.float64)[3, :] @ Pm[:3, :].T) @ R.T
        dm = inp["means3D"].grad.detach().cpu().numpy().astype(np.float64)
        bound = 2e-4 * np.abs(dm).sum(0)
        print("  translation identity: |dc + sum dmeans| / sum |dmeans| =", np.abs(dc + dm.sum(0)) / np.abs(dm).sum(0))
        assert (bound > 0).all() and (np.abs(dc + dm.sum(0)) <= bound).all()


def test_shapes_layouts_and_the_off_path():
    from diff_gaussian_rasterization import GaussianRasterizer, _native as N
    kw = _small_kwargs("a", 3, 43)
    gc = _t(S.make_grad_image(W, H, 3))
    (color, _), cams, _, _ = _render(kw)
    color.backward(gc)
    # cameras are usually stored as .transpose(0, 1) of a column-vector matrix, campos as a row of a matrix
    rs = _settings(kw)
    col = rs.viewmatrix.t().contiguous().requires_grad_(True)
    cp = rs.campos.view(1, 3).clone().requires_grad_(True)
    inp = _inputs(kw, False)
    out, _ = GaussianRasterizer(rs._replace(viewmatrix=col.t(), campos=cp))(means2D=torch.zeros(inp["means3D"].shape[0], 3, device=DEV), **inp)
    out.backward(gc)
    assert col.grad.shape == (4, 4) and torch.equal(col.grad.t(), cams[0].grad) and cp.grad.shape == (1, 3)
    assert torch.equal(cp.grad[0], cams[2].grad)

    def launches(fn):
        N.profile_enable(True)
        try:
            fn()
            torch.cuda.synchronize()
            return {k: v[1] for k, v in N.profile_read().items()}
        finally:
            N.profile_enable(False)

    def run(needs, no_grad=False):
        def f():
            if no_grad:
                with torch.no_grad():
                    (c, _), cams_, _, _ = _render(kw, needs=needs)
                assert not c.requires_grad
            else:
                (c, _), cams_, _, _ = _render(kw, needs=needs)
                c.backward(gc)
        return f
    off, on = launches(run((False, False, False))), launches(run((True, True, True)))
    assert "camera_bwd" not in off and "camera_reduce" not in off
    assert on.get("camera_bwd") == 1 and on.get("camera_reduce") == 1
    assert {k: v for k, v in on.items() if not k.startswith("camera_")} == off
    assert launches(run((True, True, True), no_grad=True)) == launches(run((False, False, False), no_grad=True))
    # debug=True and an empty scene
    (c, _), cams_d, _, _ = _render(kw, debug=True)
    c.backward(gc)
    assert torch.equal(cams_d[0].grad, cams[0].grad)
    empty = {k: (v[:0] if k in ("means3D", "opacities", "shs", "scales", "rotations") else v) for k, v in kw.items()}
    (c, _), cams_e, _, _ = _render(empty)
    c.backward(gc)
    assert all(float(x.grad.abs().max()) == 0.0 for x in cams_e)


def test_tile_rows_with_camera_gradients_raises():
    import diff_gaussian_rasterization as dgr
    kw = _small_kwargs("a", 1, 41)
    rs, _ = _cam_settings(kw)
    inp = _inputs(kw, False)
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(inp["means3D"], inp["shs"], None, inp["opacities"], inp["scales"], inp["rotations"], None, rs, tile_rows=(0, 2))


POSE_START, POSE_LR, POSE_STEPS = CR.POSE_START, CR.POSE_LR, CR.POSE_STEPS      # shared with tools/camera_pose_rehearsal.py


def test_pose_recovery():
    """A fixed scene, target = the render at the true pose; the six numbers of camera_with_pose_delta start off by about 1 degree and
    0.02 scene units and are optimised with Adam on the training loss.  Conditions: the final loss is below the initial one and the
    rotation and translation errors both end below half of their start values."""
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    from scene import GaussianModel
    from scene.cameras import camera_with_pose_delta
    Wp, Hp, P = 256, 192, 30_000
    cam = PO.posed_camera(Wp, Hp, "a").to(DEV)
    scene = PO.to_world(S.make_scene(P, Wp, Hp, 3, 11, scale_lo=0.01, scale_hi=0.06, zmin=1.0), PO.posed_camera(Wp, Hp, "a"))
    gm = GaussianModel(3)
    gm.adopt_scene(scene, device=DEV)
    for p in gm._t.values():
        p.requires_grad_(False)
    pipe, bg = Pipe(), torch.zeros(3, device=DEV)
    zero = torch.zeros(3, device=DEV)
    with torch.no_grad():
        target = render(camera_with_pose_delta(cam, zero, zero), gm, pipe, bg)["render"].clone()
    rot = torch.tensor(POSE_START["rot"], device=DEV, requires_grad=True)
    trans = torch.tensor(POSE_START["trans"], device=DEV, requires_grad=True)
    opt = torch.optim.Adam([rot, trans], lr=POSE_LR)
    r0, t0 = float(rot.detach().norm()), float(trans.detach().norm())
    losses = []
    for _ in range(POSE_STEPS):
        opt.zero_grad()
        loss = training_loss(render(camera_with_pose_delta(cam, rot, trans), gm, pipe, bg)["render"], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    r1, t1 = float(rot.detach().norm()), float(trans.detach().norm())
    print(f"  pose recovery: loss {losses[0]:.5f} -> {losses[-1]:.5f}; rotation error {math_deg(r0):.3f} -> {math_deg(r1):.3f} deg; "
          f"translation error {t0:.4f} -> {t1:.4f}")
    assert losses[-1] < losses[0] and r1 < 0.5 * r0 and t1 < 0.5 * t0


def math_deg(r):
    return r * 180.0 / np.pi
