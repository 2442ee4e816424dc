"""CPU checks of the depth / alpha extension: the C ABI is additive (new symbols declared and exported, new struct mirrored,
version and settings unchanged), and the fp64 reference the GPU tests use for the two maps is pinned against torch autograd.

The reference: the oracle renders depth and alpha as an ordinary colour frame with colors_precomp = (z, 1, 0) and bg = 0.
Channel 0 is then depth = sum w_i z_i, channel 1 is sum w_i = 1 - T_final, and the gradient of a loss on the maps is that
frame's gradient for dL/dcolor = (g_z, g_a, 0) plus the colour gradient of channel 0 (= dL/dz) chained to means3D through
z = (means3D . viewmatrix)_z.  tests/torch_ref.py states the same maps directly: depth from a z that autograd differentiates,
alpha as 1 - Tacc."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle
import scene_synth as S
from torch_ref import render_autograd
from util import raster_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_aux_workspace_size", "gsr_forward_aux", "gsr_forward_render_aux", "gsr_backward_render_aux",
                 "gsr_backward_geom_aux")


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_aux_functions_are_declared_and_exported(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert "gsr_aux_outputs" in hdr
    assert lib.gsr_version() == 12


def test_settings_fields_are_unchanged():
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix",
        "sh_degree", "campos", "prefiltered", "debug")


def test_aux_workspace_size_without_gpu(native):
    """1 KB of depth checkpoint per 128 binned instances (+ 2), plus (GSR_MAX_CHUNKS - 1) KB per tile for the chunk starts."""
    desc = native.make_desc(1000, 3, 16, 1920, 1080, 0.5, 0.5, 1.0, False, False)
    tiles = 120 * 68
    seg = native.bwd_segment_entries()
    for n in (0, 1, 1000, 5_000_000):
        want = (max(n, 1) // seg + 2) * 1024 + 7 * tiles * 1024
        assert want <= native.aux_workspace_size(desc, n) < want + 512, n
    with pytest.raises(native.GsrError):
        native.aux_workspace_size(desc, -1)
    lib = native.load()
    bad = native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)
    b = C.c_size_t(0)
    assert lib.gsr_aux_workspace_size(C.byref(bad), C.c_int64(10), C.byref(b)) == -1
    assert b"sh_degree" in lib.gsr_last_error()


def test_null_aux_is_the_plain_call_without_gpu(native):
    """aux = NULL takes the plain calls' path: on arguments they reject, the aux entry points return the same status and the same
    message (every case here is refused before any device work)."""
    lib = native.load()
    ok = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    bad = native.make_desc(10, 5, 16, 64, 64, 0.5, 0.5, 1.0, False, False)
    cam = native.Camera(1, 1, 1, 1)
    no_colour = native.Gaussians(1, None, None, 1, 1, 1, None)          # neither SHs nor colours
    one = C.c_void_p(1)

    def both(plain, aux):
        rc0 = plain()
        msg0 = lib.gsr_last_error()
        rc1 = aux()
        msg1 = lib.gsr_last_error()
        assert rc0 < 0 and (rc0, msg0) == (rc1, msg1), (rc0, msg0, rc1, msg1)
    for d in (ok, bad):
        plan = native.FramePlan()
        plan.num_rendered, plan.num_chunks = 10, 1
        both(lambda: lib.gsr_forward_render(C.byref(d), C.byref(cam), C.byref(no_colour), one, one, one, C.byref(plan), one, None),
             lambda: lib.gsr_forward_render_aux(C.byref(d), C.byref(cam), C.byref(no_colour), one, one, one, C.byref(plan), one, None,
                                                None))
        # no colour gradient: the plain backward's NULL-argument refusal
        both(lambda: lib.gsr_backward_render(C.byref(d), C.byref(cam), one, one, one, one, C.byref(plan), one, None, one, None),
             lambda: lib.gsr_backward_render_aux(C.byref(d), C.byref(cam), one, one, one, one, C.byref(plan), one, None, None, one, one,
                                                 one, None))


def test_aux_with_tile_rows_raises():
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(32, 32, .5, .5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                           torch.zeros(3), False, False)
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs,
                              tile_rows=(0, 1), aux=True)


def _view_z_column(kw):
    return np.asarray(kw["viewmatrix"], np.float64)[:3, 2]


@pytest.mark.parametrize("P,W,H,seed", [(40, 48, 32, 31), (32, 40, 56, 32)])
def test_oracle_depth_alpha_frame_matches_torch_autograd(P, W, H, seed):
    _depth_alpha_vs_autograd(P, W, H, seed)


def test_oracle_depth_alpha_frame_matches_torch_autograd_at_a_posed_camera():
    """The z chain dz (view[2], view[6], view[10]) with every view-matrix entry non-zero (tests/posed.py)."""
    _depth_alpha_vs_autograd(40, 48, 40, 33, pose="b")


def _depth_alpha_vs_autograd(P, W, H, seed, pose=None):
    scene = S.make_scene(P, W, H, 1, seed, scale_lo=0.02, scale_hi=0.25)
    if pose is None:
        cam = S.make_camera(W, H)
    else:
        import posed as PO
        cam = PO.posed_camera(W, H, pose)
        scene = PO.to_world(scene, cam)
    kw = raster_kwargs(scene, cam)
    V = np.asarray(kw["viewmatrix"], np.float64)
    m3 = np.asarray(kw["means3D"], np.float64)
    z = m3 @ V[:3, 2] + V[3, 2]
    cols = np.stack([z, np.ones_like(z), np.zeros_like(z)], 1)
    aux_kw = {k: v for k, v in kw.items() if k != "shs"}
    aux_kw.update(colors_precomp=cols.astype(np.float32), bg=np.zeros(3, np.float32))
    fr = oracle.rasterize(dtype=np.float64, **{**aux_kw, "colors_precomp": cols})

    # torch: explicit depth (z differentiated through means3D) and alpha = 1 - T_final
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    means3D = t(m3).requires_grad_(True)
    leaves = {"means3D": means3D, "opacities": t(kw["opacities"]).requires_grad_(True),
              "scales": t(kw["scales"]).requires_grad_(True), "rotations": t(kw["rotations"]).requires_grad_(True)}
    zt = means3D @ t(V[:3, 2]) + float(V[3, 2])
    ct = torch.stack([zt, torch.ones_like(zt), torch.zeros_like(zt)], 1)
    settings = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in aux_kw.items()
                if k not in ("means3D", "opacities", "scales", "rotations", "colors_precomp")}
    color, radii, proxy, Tacc = render_autograd(colors_precomp=ct, **leaves, **settings)
    depth, alpha = color[0], 1 - Tacc
    np.testing.assert_array_equal(radii.numpy(), fr.radii)
    assert np.abs(depth.detach().numpy() - fr.color[0]).max() <= 1e-12 * max(z.max(), 1.0)
    assert np.abs(alpha.detach().numpy() - fr.color[1]).max() <= 1e-12            # sum w = 1 - T_final
    assert np.all(fr.color[2] == 0)

    g = torch.Generator().manual_seed(seed)
    gz = (torch.rand(H, W, generator=g, dtype=torch.float64) - 0.5) / float(z.max())
    ga = torch.rand(H, W, generator=g, dtype=torch.float64) - 0.5
    ((depth * gz).sum() + (alpha * ga).sum()).backward()
    got = fr.backward(np.stack([gz.numpy(), ga.numpy(), np.zeros((H, W))]))
    got["means3D"] = got["means3D"] + got["colors_precomp"][:, :1] * _view_z_column(kw)[None]      # the z chain
    for name, leaf in leaves.items():
        want = leaf.grad.numpy().reshape(got[name].shape)
        scale = max(np.abs(want).max(), 1e-12)
        err = np.abs(got[name] - want).max()
        assert err <= 1e-9 * scale + 1e-12, f"{name}: {err:.3e} vs scale {scale:.3e}"
    want2d = proxy.grad.numpy()
    assert np.abs(got["means2D"][:, :2] - want2d).max() <= 1e-9 * max(np.abs(want2d).max(), 1e-12)
