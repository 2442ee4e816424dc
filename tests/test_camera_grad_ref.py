"""CPU checks of the camera gradients: the C ABI is additive (new symbols declared and exported, the struct mirrored, version and
settings unchanged), the two binary64 references of tests/camera_ref.py agree (tier A: autograd through the whole blend; tier B: the
oracle's screen-space rows contracted with the projection's derivative, Gaussian by Gaussian), moving the camera is moving the scene
the other way, the kernel's own per-Gaussian function (csrc/gsr_math.h camera_backward_one, compiled with g++: tests/camera_host.cpp)
gives tier B's per-Gaussian terms, scene.cameras.camera_with_pose_delta is the camera at zero and differentiable, and the "does this call want camera
gradients" decision is what autograd users expect."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import camera_ref as CR
import oracle
import posed as PO
import scene_synth as S
from util import cov3d_from, raster_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_camera_grad_workspace_size", "gsr_backward_camera")
W, H = 64, 48


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_camera_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert "gsr_camera_grads" in hdr
    assert lib.gsr_version() == 12 and "#define GSR_VERSION 12" in hdr


def test_settings_fields_are_unchanged():
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")


def test_camera_grad_workspace_size_without_gpu(native):
    """One 27-float partial sum per block of 256 Gaussians (at least one), padded to 256 bytes."""
    sizes = []
    for P in (0, 1, 256, 257, 1000, 1_000_000, 5_000_000):
        desc = native.make_desc(P, 3, 16, 1920, 1080, 0.5, 0.5, 1.0, False, False)
        want = max((P + 255) // 256, 1) * 27 * 4
        got = native.camera_grad_workspace_size(desc)
        assert want <= got < want + 256 and got % 256 == 0, (P, got)
        sizes.append(got)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
    lib = native.load()
    bad = native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)
    b = C.c_size_t(0)
    assert lib.gsr_camera_grad_workspace_size(C.byref(bad), C.byref(b)) == -1
    assert b"sh_degree" in lib.gsr_last_error()


def test_backward_camera_refuses_a_slab_without_gpu(native):
    lib = native.load()
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(0, 2))
    one = C.c_void_p(1)
    cam = native.Camera(1, 1, 1, 1)
    g = native.Gaussians(1, 1, None, 1, 1, 1, None)
    out = native.CameraGrads(1, 1, 1)
    rc = lib.gsr_backward_camera(C.byref(slab), C.byref(cam), C.byref(g), one, one, one, C.c_int32(-1), None, C.c_int32(0), one,
                                 C.byref(out), None)
    assert rc == -1 and b"whole images" in lib.gsr_last_error()


# ---- tier A == tier B ---------------------------------------------------------------------------------------------------------
def _small(pose, D, seed, P=100, mode="sh", scale_modifier=1.0):
    cam = PO.posed_camera(W, H, pose)
    scene = PO.to_world(S.make_scene(P, W, H, D, seed, scale_lo=0.02, scale_hi=0.2), cam)
    a = scene.activated()
    extra = {}
    if mode == "color":
        extra["colors_precomp"] = torch.rand(P, 3, generator=torch.Generator().manual_seed(seed))
    if mode == "cov":
        extra["cov3D_precomp"] = cov3d_from(a["scales"], a["rotations"], scale_modifier)
    return raster_kwargs(scene, cam, bg=(0.1, 0.2, 0.3), scale_modifier=scale_modifier, **extra)


def _agree(kw, grad_color, grad_depth=None, grad_alpha=None, tol=1e-12):
    screen, dz, radii = CR.oracle_rows(kw, grad_color, grad_depth, grad_alpha)
    b_sum, b_abs, _, sel = CR.tier_b(kw, screen, radii, dz)
    a = CR.tier_a(kw, grad_color, grad_depth, grad_alpha)
    assert sel.size > 10
    for n in CR.NAMES:
        scale = np.abs(a[n]).max()
        assert np.abs(a[n] - b_sum[n]).max() <= tol * max(scale, np.abs(b_sum[n]).max()) + 1e-300, \
            (n, np.abs(a[n] - b_sum[n]).max(), scale)
        assert (b_abs[n] >= np.abs(b_sum[n]) * (1 - 1e-12)).all()
    for m in (a, b_sum, b_abs):
        assert (m["viewmatrix"][:, 3] == 0).all() and (m["projmatrix"][:, 2] == 0).all()
    return a, b_sum, b_abs


@pytest.mark.parametrize("pose", ["a", "b", "c"])
@pytest.mark.parametrize("D", [0, 1, 2, 3])
def test_tier_a_equals_tier_b_sh(pose, D):
    kw = _small(pose, D, 40 + D)
    a, _, _ = _agree(kw, S.make_grad_image(W, H, 3).numpy().astype(np.float64))
    assert np.abs(a["viewmatrix"]).max() > 0 and np.abs(a["projmatrix"]).max() > 0
    assert (np.abs(a["campos"]).max() > 0) == (D > 0)            # degree 0 has no view dependence


@pytest.mark.parametrize("mode,scale_modifier", [("color", 1.0), ("cov", 1.0), ("sh", 0.7)])
def test_tier_a_equals_tier_b_modes(mode, scale_modifier):
    kw = _small("a", 2, 51, mode=mode, scale_modifier=scale_modifier)
    a, b_sum, b_abs = _agree(kw, S.make_grad_image(W, H, 4).numpy().astype(np.float64))
    if mode == "color":
        assert (a["campos"] == 0).all() and (b_sum["campos"] == 0).all() and (b_abs["campos"] == 0).all()


def test_tier_a_equals_tier_b_edge_scene():
    cam = PO.posed_camera(W, H, "b")
    counts = dict(clamp_x=12, clamp_y=12, clamp_xy=10, near=16, culled=12, needle_disc=24, opaque=24, sh_clamp=24)
    scene, labels = PO.edge_scene(W, H, cam, 7, 60, counts)
    kw = raster_kwargs(scene, cam)
    _agree(kw, S.make_grad_image(W, H, 5).numpy().astype(np.float64))


def test_tier_a_equals_tier_b_aux():
    """A loss on colour, depth and alpha: autograd carries the depth's chain (z from the viewmatrix leaf) into dL/dviewmatrix."""
    kw = _small("c", 1, 61)
    g = torch.Generator().manual_seed(9)
    gz = (torch.rand(H, W, generator=g, dtype=torch.float64) - 0.5).numpy() / 6.0
    ga = (torch.rand(H, W, generator=g, dtype=torch.float64) - 0.5).numpy()
    gc = S.make_grad_image(W, H, 6).numpy().astype(np.float64)
    with_z = _agree(kw, gc, gz, ga)[0]
    colour_only = _agree(kw, gc)[0]
    assert np.abs(with_z["viewmatrix"][:, 2] - colour_only["viewmatrix"][:, 2]).max() > 0


def test_moving_the_camera_is_moving_the_scene_the_other_way():
    """With V[3, :3] = -c V[:3, :3], PV = V P and campos = c, the camera gradients chained to c equal minus dL/dmeans3D, per
    Gaussian and in total."""
    kw = _small("a", 3, 71, P=150)
    gimg = S.make_grad_image(W, H, 8).numpy().astype(np.float64)
    fr = oracle.rasterize(dtype=np.float64, **kw)
    screen = fr.backward_screen(gimg)
    dmeans = fr.backward_geom(screen)["means3D"]
    _, _, t, sel = CR.tier_b(kw, screen, fr.radii)
    V, PV = np.asarray(kw["viewmatrix"], np.float64), np.asarray(kw["projmatrix"], np.float64)
    R, Pm = V[:3, :3], np.linalg.inv(V) @ PV
    dc = t["campos"] - (t["viewmatrix"][:, 3, :3] + t["projmatrix"][:, 3, :] @ Pm[:3, :].T) @ R.T
    scale = np.abs(dmeans[sel]).max()
    assert scale > 0
    assert np.abs(dc + dmeans[sel]).max() <= 1e-12 * scale
    assert np.abs(dc.sum(0) + dmeans[sel].sum(0)).max() <= 1e-12 * np.abs(dmeans[sel]).sum(0).max()
    assert not dmeans[fr.radii == 0].any()


# ---- scene.cameras ------------------------------------------------------------------------------------------------------------
def test_camera_with_pose_delta():
    from scene.cameras import camera_with_pose_delta
    cam = PO.posed_camera(W, H, "b")
    z = torch.zeros(3, dtype=torch.float64)
    c0 = camera_with_pose_delta(cam, z, z)
    assert (c0.image_width, c0.image_height, c0.FoVx, c0.FoVy) == (cam.image_width, cam.image_height, cam.FoVx, cam.FoVy)
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert np.abs(getattr(c0, name).numpy() - getattr(cam, name).double().numpy()).max() <= 1e-6, name
    # a rigid correction composed by hand (Rodrigues), through scene_synth.make_camera
    rv, tv = np.array([0.02, -0.015, 0.01]), np.array([0.02, 0.01, -0.015])
    th = np.linalg.norm(rv)
    k = rv / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rd = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * K @ K
    V = cam.world_view_transform.double().numpy()
    Rc, tc = V[:3, :3] @ Rd.T, V[3, :3] @ Rd.T + tv              # p_view' = Rd p_view + tv, row vectors
    want = S.make_camera(W, H, Rc, tc, math.tan(cam.FoVy * 0.5), math.tan(cam.FoVx * 0.5))
    got = camera_with_pose_delta(cam, torch.tensor(rv), torch.tensor(tv))
    for name in ("world_view_transform", "full_proj_transform", "camera_center"):
        assert np.abs(getattr(got, name).numpy() - getattr(want, name).double().numpy()).max() <= 1e-6, name
    f = lambda r, t: tuple(getattr(camera_with_pose_delta(cam, r, t), n)
                           for n in ("world_view_transform", "full_proj_transform", "camera_center"))
    for r0, t0 in ((z, z), (torch.tensor(rv), torch.tensor(tv))):
        assert torch.autograd.gradcheck(f, (r0.clone().requires_grad_(True), t0.clone().requires_grad_(True)))


# ---- the auto-detect decision ---------------------------------------------------------------------------------------------------
def _rs(vm, pm, cp):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(32, 32, .5, .5, torch.zeros(3), 1.0, vm, pm, 0, cp, False, False)


def test_camera_grads_wanted_decision():
    import diff_gaussian_rasterization as dgr
    plain = lambda: (torch.eye(4), torch.eye(4), torch.zeros(3))
    assert not dgr.camera_grads_wanted(_rs(*plain()))
    for k in range(3):
        t = list(plain())
        t[k] = t[k].requires_grad_(True)
        assert dgr.camera_grads_wanted(_rs(*t))
        assert dgr.camera_grads_wanted(_rs(*t), True) and not dgr.camera_grads_wanted(_rs(*t), False)
        with torch.no_grad():
            assert not dgr.camera_grads_wanted(_rs(*t))
            assert dgr._camera_args(_rs(*t)) == ()
        assert not dgr.camera_grads_wanted(_rs(*(x.detach() for x in t)))
        args = dgr._camera_args(_rs(*t))
        assert len(args) == 3 and all(a is b for a, b in zip(args, t))
        with pytest.raises(ValueError, match="tile_rows"):
            dgr.camera_grads_wanted(_rs(*t), tile_rows=(0, 1))
    assert not dgr.camera_grads_wanted(_rs(*plain()), tile_rows=(0, 1))
    assert dgr._camera_args(_rs(*plain())) == ()


def test_binned_prefix_of_hand_built_plans():
    """_native.binned_prefix, the binned_ranks both backward entry points pass for a frame's own gradients: the depth ranks of the
    chunks that ran.  effective_binned_ranks (the dense / sparse decision) on the same plans stays what it was: it alone skips a
    live-filtered chunk."""
    from diff_gaussian_rasterization import _native as N

    def plan(num_rendered, chunks_run, chunks_filtered=0):
        p = N.FramePlan()
        p.num_rendered, p.num_visible, p.num_chunks, p.chunks_run, p.chunks_filtered = num_rendered, 60, 3, chunks_run, chunks_filtered
        for c, r in enumerate((0, 10, 30, 60)):
            p.chunk_rank_begin[c] = r
        return p
    for p, prefix, effective in ((plan(0, 2), 0, 0),               # nothing rendered
                                 (plan(500, 0), 0, 0),             # no chunk ran
                                 (plan(500, 2), 30, 30),           # two chunks run of three planned: chunk_rank_begin[2]
                                 (plan(500, 2, 0b10), 30, 10),     # ... the second through the live filter
                                 (plan(500, 3), 60, 60)):
        assert N.binned_prefix(p) == prefix
        assert N.effective_binned_ranks(p) == effective


def test_camera_grads_with_tile_rows_raises():
    import diff_gaussian_rasterization as dgr
    rs = _rs(torch.eye(4).requires_grad_(True), torch.eye(4), torch.zeros(3))
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs, tile_rows=(0, 1))


# ---- the kernel's own per-Gaussian function on the host --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def camera_host(tmp_path_factory):
    import subprocess
    so = str(tmp_path_factory.mktemp("ch") / "libcamera_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", "-std=c++17", "-o", so, os.path.join(ROOT, "tests", "camera_host.cpp")])
    return C.CDLL(so)


@pytest.mark.parametrize("case", ["sh3 pose a", "sh1 pose c", "colors_precomp", "cov3D_precomp", "scale_modifier 0.7", "edge scene"])
def test_camera_backward_one_on_the_host_against_tier_b(camera_host, case):
    """csrc/gsr_math.h camera_backward_one (the function k_camera_bwd calls, compiled with g++) against tier B's per-Gaussian terms
    t_i, from the binary64 oracle's screen rows rounded to binary32.  It repeats geom_backward_one's chain (its twin, which
    tests/test_host_math.py holds to the oracle): this is what ties the second copy to a reference without a GPU.  Bound per
    Gaussian and tensor: 1e-4 of the Gaussian's own largest |t_i| entry of that tensor (the project's per-Gaussian promise), plus
    1e-6 of the frame's largest for entries that cancel inside one Gaussian."""
    if case == "edge scene":
        cam = PO.posed_camera(W, H, "b")
        kw = raster_kwargs(PO.edge_scene(W, H, cam, 7, 60, dict(clamp_x=12, clamp_y=12, clamp_xy=10, near=16, culled=12, needle_disc=24,
                                                                opaque=24, sh_clamp=24))[0], cam)
    else:
        kw = {"sh3 pose a": lambda: _small("a", 3, 43), "sh1 pose c": lambda: _small("c", 1, 41),
              "colors_precomp": lambda: _small("a", 2, 51, mode="color"), "cov3D_precomp": lambda: _small("a", 2, 51, mode="cov"),
              "scale_modifier 0.7": lambda: _small("a", 2, 51, scale_modifier=0.7)}[case]()
    fr = oracle.rasterize(dtype=np.float64, **kw)
    screen = fr.backward_screen(S.make_grad_image(W, H, 3).numpy().astype(np.float64)).astype(np.float32)
    _, _, t, sel = CR.tier_b(kw, screen.astype(np.float64), fr.radii)
    f32 = lambda k: None if kw.get(k) is None else np.ascontiguousarray(np.asarray(kw[k], np.float32))
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    n = fr.P
    arrs = {k: f32(k) for k in ("viewmatrix", "projmatrix", "campos", "means3D", "scales", "rotations", "cov3D_precomp", "shs")}
    M = 0 if arrs["shs"] is None else arrs["shs"].shape[1]
    radii = np.ascontiguousarray(fr.radii, np.int32)
    scr = np.ascontiguousarray(screen[:, :9])
    out = np.zeros((n, 27), np.float32)
    camera_host.camera_terms_host(C.c_int(n), C.c_int(int(kw["sh_degree"])), C.c_int(M), C.c_int(W), C.c_int(H),
                                  C.c_float(kw["tanfovx"]), C.c_float(kw["tanfovy"]), C.c_float(kw["scale_modifier"]),
                                  ptr(arrs["viewmatrix"]), ptr(arrs["projmatrix"]), ptr(arrs["campos"]), ptr(arrs["means3D"]),
                                  ptr(arrs["scales"]), ptr(arrs["rotations"]), ptr(arrs["cov3D_precomp"]), ptr(arrs["shs"]),
                                  C.c_int(int(kw.get("colors_precomp") is not None)), ptr(radii), ptr(scr), ptr(out))
    got = out[sel].astype(np.float64)
    gv = np.zeros((sel.size, 4, 4)); gv[:, :, :3] = got[:, :12].reshape(-1, 4, 3)
    gp = np.zeros((sel.size, 4, 4)); gp[:, :, [0, 1, 3]] = got[:, 12:24].reshape(-1, 4, 3)
    assert not out[fr.radii == 0].any() and sel.size > 10
    for name, g in (("viewmatrix", gv), ("projmatrix", gp), ("campos", got[:, 24:27])):
        w = t[name].reshape(sel.size, -1)
        e = np.abs(g.reshape(sel.size, -1) - w)
        own = np.abs(w).max(1, keepdims=True)
        bound = 1e-4 * own + 1e-6 * np.abs(w).max()
        assert (e <= bound).all(), (case, name, float((e / np.maximum(bound, 1e-300)).max()))
        if name != "campos" or case != "colors_precomp":
            assert np.abs(w).max() > 0
