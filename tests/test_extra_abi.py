"""CPU-only checks of the extra-colour channels (GaussianRasterizer(depth_alpha=True)(..., extra_colors=t)): the C ABI is additive (five
new symbols in include/gsrast_extra.h, which gsrast.h includes; the version unchanged) and its ctypes table agrees with that header's
prototypes; everything the feature refuses before a launch is a ValueError (or a status with a message); and the float64 reference
construction the GPU tests use - the sum of three oracle backwards, the third a frame with colors_precomp = extra over a zero
background - agrees with torch autograd on tests/torch_ref.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import oracle
import scene_synth as S
from test_abi import header_prototypes, signature_mismatches
from torch_ref import render_autograd
from util import raster_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_extra_workspace_size", "gsr_extra_rows_size", "gsr_forward_render_extra", "gsr_forward_extra",
                 "gsr_backward_render_extra")


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def _extra_header():
    with open(os.path.join(ROOT, "include", "gsrast_extra.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_functions_are_declared_and_exported_and_the_version_stays(native):
    main = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert '#include "gsrast_extra.h"' in main and "#define GSR_VERSION 12" in main
    protos = header_prototypes(_extra_header())
    assert tuple(protos) == NEW_FUNCTIONS == tuple(native.EXTRA_SIGNATURES)
    bad = signature_mismatches(protos, native.EXTRA_SIGNATURES, native.MIRRORS)
    assert not bad, "\n".join(bad)
    lib = native.load()
    for name, (restype, argtypes) in native.EXTRA_SIGNATURES.items():
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert getattr(lib, name).restype is restype and tuple(getattr(lib, name).argtypes) == tuple(argtypes), name
        assert name not in native.SIGNATURES and name not in native.NORMALS_SIGNATURES
    assert lib.gsr_version() == 12
    assert "typedef" not in _extra_header()                          # no struct of its own: gsrast.h's mirrors stay the whole set
    mk = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "gsrast_extra.h" in mk


def test_workspace_sizes_without_gpu(native):
    """Four 1 KB checkpoint planes where the aux frame has one: 4 KB per 128 binned instances (+ 2) plus 4 (GSR_MAX_CHUNKS - 1) KB per
    tile; one float4 per instance of the backward's row bound."""
    desc = native.make_desc(1000, 3, 16, 1920, 1080, 0.5, 0.5, 1.0, False, False)
    tiles = 120 * 68
    seg = native.bwd_segment_entries()
    for n in (0, 1, 1000, 5_000_000):
        want = (max(n, 1) // seg + 2) * 4096 + 7 * tiles * 4096
        assert want <= native.extra_workspace_size(desc, n) < want + 512, n
        aux = (max(n, 1) // seg + 2) * 1024 + 7 * tiles * 1024
        assert aux <= native.aux_workspace_size(desc, n) < aux + 512, n       # the aux frame's own size is what it was
    with pytest.raises(native.GsrError):
        native.extra_workspace_size(desc, -1)
    plan = native.FramePlan()
    plan.num_rendered, plan.num_chunks, plan.chunks_run = 1000, 1, 1
    plan.chunk_instances_max[0] = 1000
    rows, ext = native.backward_rows_size(desc, plan), native.extra_rows_size(desc, plan)
    assert rows % 48 == 0 or rows >= 48
    assert 0 < ext <= rows and abs(ext * 3 - rows) <= 3 * 256                 # a third of the 48-byte rows, to the 256-byte padding


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    desc = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(0, 2))
    cam = native.Camera(256, 256, 256, 256)
    g = native.Gaussians(256, 256, None, 256, 256, 256, None)
    aux = native.AuxOutputs(256, 256, 256)
    p, odd = C.c_void_p(256), C.c_void_p(260)
    plan = native.FramePlan()
    plan.num_rendered, plan.num_chunks = 10, 1

    def fwd(d=desc, a=aux, table=p, out=p):
        rc = lib.gsr_forward_render_extra(C.byref(d), C.byref(cam), C.byref(g), p, p, p, C.byref(plan), p, a, table, out, None)
        return rc, lib.gsr_last_error()

    def both(d=desc, a=aux, table=p, out=p):
        rc = lib.gsr_forward_extra(C.byref(d), C.byref(cam), C.byref(g), p, p, p, C.byref(plan), p, 100, p, None, a, table, out, None)
        return rc, lib.gsr_last_error()

    def bwd(d=desc, a=aux, table=p, out=p, rows=p, grad=p):
        rc = lib.gsr_backward_render_extra(C.byref(d), C.byref(cam), p, p, p, p, C.byref(plan), p, a, table, out, p, None, None, None, p,
                                           rows, grad, None)
        return rc, lib.gsr_last_error()

    for call in (fwd, both, bwd):
        for kw, word in ((dict(table=None), b"extra table is NULL"), (dict(table=odd), b"16-byte aligned"), (dict(out=None), b"extra_map is NULL"),
                         (dict(a=None), b"aux is required"), (dict(d=slab), b"whole images only")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, rc, msg)
    rc, msg = bwd(grad=None)
    assert rc == -1 and b"dL_dextra is NULL" in msg
    rc, msg = bwd(rows=None)
    assert rc == -1 and b"extra_rows_ws is NULL" in msg
    b = C.c_size_t(0)
    assert lib.gsr_extra_rows_size(C.byref(desc), None, C.byref(b)) == -1 and b"NULL" in lib.gsr_last_error()
    with pytest.raises(ValueError, match="aux required"):
        native._variant("forward_render", None, None, None, extra=(None, None))


def _rasterizer(depth_alpha=True, **kw):
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(32, 32, .5, .5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    rs = rs._replace(**{k: kw.pop(k) for k in list(kw) if k in rs._fields})
    return dgr.GaussianRasterizer(rs, depth_alpha=depth_alpha, **kw)


def _call(rast, extra, raw=False, P=4):
    z = torch.zeros(P, 3)
    if raw:
        return rast.forward_raw(z, z.clone(), torch.zeros(P, 1, 3), torch.zeros(P, 0, 3), torch.zeros(P, 1), z, torch.zeros(P, 4), extra_colors=extra)
    return rast(means3D=z, means2D=z.clone(), opacities=torch.zeros(P, 1), shs=torch.zeros(P, 1, 3), scales=z, rotations=torch.zeros(P, 4),
                extra_colors=extra)


@pytest.mark.parametrize("raw", [False, True], ids=["forward", "forward_raw"])
def test_refusals_before_any_launch_are_value_errors(raw):
    """Host tensors throughout: a call that got past these checks would raise the RuntimeError of the missing HIP device instead."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization.contrib import ContributionStats
    ok = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="depth_alpha=True"):
        _call(_rasterizer(depth_alpha=False), ok, raw)
    for bad, word in ((torch.zeros(5, 3), "shape"), (torch.zeros(4, 4), "shape"), (torch.zeros(4, 3, dtype=torch.float64), "dtype"),
                      (torch.zeros(4, 3, device="meta"), "the frame's inputs live on"), (np.zeros((4, 3), np.float32), "tensor")):
        with pytest.raises(ValueError, match=word):
            _call(_rasterizer(), bad, raw)
    with pytest.raises(ValueError, match="absgrad"):
        _call(_rasterizer(depth_alpha=False, absgrad=True), ok, raw)
    with pytest.raises(ValueError, match="contributions"):
        _call(_rasterizer(depth_alpha=False, contributions=ContributionStats(4, device="cpu")), ok, raw)
    for field in ("viewmatrix", "projmatrix", "campos"):
        t = (torch.zeros(3) if field == "campos" else torch.eye(4)).requires_grad_(True)
        with pytest.raises(ValueError, match="camera gradients"):
            _call(_rasterizer(**{field: t}), ok, raw)
    # past every check: the call reaches the native forward, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call(_rasterizer(), ok, raw)
    z = torch.zeros(4, 3)
    rs = _rasterizer().raster_settings
    with pytest.raises(ValueError, match="tile_rows"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs, tile_rows=(0, 1), aux=True, extra=ok)
    with pytest.raises(ValueError, match="depth_alpha=True"):
        dgr.rasterize_forward(z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs, extra=ok)


def test_sharded_renderer_and_training_flags_refuse():
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    r = ShardedRenderer.__new__(ShardedRenderer)                    # (the refusals come before anything of the instance is read)
    with pytest.raises(ValueError, match="extra_colors is not supported by ShardedRenderer"):
        r.render(None, None, None, None, extra_colors=torch.zeros(4, 3))
    with pytest.raises(ValueError):
        r.render_with_normals(None, None, None, None)
    from scene.gaussian_model import OptimizationDefaults
    assert OptimizationDefaults().normal_in_frame is False
    import train_loop

    class Opt(OptimizationDefaults):
        pass
    opt = OptimizationDefaults()
    opt.lambda_normal, opt.normal_in_frame, opt.densify_absgrad = 0.05, True, True
    with pytest.raises(ValueError, match="normal_in_frame with densify_absgrad"):
        train_loop.train(None, [], [], opt, None, None, 0)


def test_reference_construction_matches_torch_autograd():
    """L = <g_c, C> + <g_z, depth> + <g_a, alpha> + <g_e, extra> on one tiny scene: the sum of three oracle backwards - the SH frame's
    for g_c, the (z, 1, 0) frame's for (g_z, g_a, 0) with its z chain, and the frame with colors_precomp = extra over a zero background
    for g_e, whose colors_precomp gradient is dL/dextra_colors - against torch autograd through tests/torch_ref.py, in binary64."""
    P, W, H, seed = 64, 48, 80, 41
    scene = S.make_scene(P, W, H, 1, seed, scale_lo=0.02, scale_hi=0.25)
    kw = raster_kwargs(scene, S.make_camera(W, H))
    V = np.asarray(kw["viewmatrix"], np.float64)
    m3 = np.asarray(kw["means3D"], np.float64)
    z = m3 @ V[:3, 2] + V[3, 2]
    gen = torch.Generator().manual_seed(seed)
    extra = torch.rand(P, 3, generator=gen, dtype=torch.float64).numpy() * 2 - 1          # signed, uniform in [-1, 1]
    base = {k: v for k, v in kw.items() if k != "shs"}
    fr_sh = oracle.rasterize(dtype=np.float64, **kw)
    fr_aux = oracle.rasterize(dtype=np.float64, **{**base, "colors_precomp": np.stack([z, np.ones_like(z), np.zeros_like(z)], 1), "bg": np.zeros(3)})
    fr_ext = oracle.rasterize(dtype=np.float64, **{**base, "colors_precomp": extra, "bg": np.zeros(3)})

    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    leaves = {"means3D": t(m3).requires_grad_(True), "opacities": t(kw["opacities"]).requires_grad_(True),
              "scales": t(kw["scales"]).requires_grad_(True), "rotations": t(kw["rotations"]).requires_grad_(True)}
    shs, ext = t(kw["shs"]).requires_grad_(True), t(extra).requires_grad_(True)
    settings = {k: (t(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()
                if k not in ("means3D", "opacities", "scales", "rotations", "shs", "colors_precomp")}
    zero_bg = {**settings, "bg": torch.zeros(3, dtype=torch.float64)}
    zt = leaves["means3D"] @ t(V[:3, 2]) + float(V[3, 2])
    # three renders that share every leaf: the blend weights are the same function of the same leaves in each
    color, radii, proxy_c, _ = render_autograd(shs=shs, **leaves, **settings)
    aux, _, proxy_a, Tacc = render_autograd(colors_precomp=torch.stack([zt, torch.ones_like(zt), torch.zeros_like(zt)], 1), **leaves, **zero_bg)
    emap, _, proxy_e, _ = render_autograd(colors_precomp=ext, **leaves, **zero_bg)
    np.testing.assert_array_equal(radii.numpy(), fr_sh.radii)
    assert np.abs(emap.detach().numpy() - fr_ext.color).max() <= 1e-12
    gc = torch.rand(3, H, W, generator=gen, dtype=torch.float64) - 0.5
    gz = (torch.rand(H, W, generator=gen, dtype=torch.float64) - 0.5) / float(z.max())
    ga = torch.rand(H, W, generator=gen, dtype=torch.float64) - 0.5
    ge = torch.rand(3, H, W, generator=gen, dtype=torch.float64) - 0.5
    ((color * gc).sum() + (aux[0] * gz).sum() + ((1 - Tacc) * ga).sum() + (emap * ge).sum()).backward()

    w_sh = fr_sh.backward(gc.numpy())
    w_aux = fr_aux.backward(np.stack([gz.numpy(), ga.numpy(), np.zeros((H, W))]))
    w_ext = fr_ext.backward(ge.numpy())
    got = {n: w_sh[n] + w_aux[n] + w_ext[n] for n in ("means3D", "means2D", "opacities", "scales", "rotations")}
    got["means3D"] = got["means3D"] + w_aux["colors_precomp"][:, :1] * V[:3, 2][None]
    got["shs"], got["extra_colors"] = w_sh["shs"], w_ext["colors_precomp"]
    want = {**{n: leaf.grad.numpy() for n, leaf in leaves.items()}, "shs": shs.grad.numpy(), "extra_colors": ext.grad.numpy()}
    for name, w in want.items():
        w = w.reshape(got[name].shape)
        scale = max(np.abs(w).max(), 1e-12)
        err = np.abs(got[name] - w).max()
        print(f"{name}: err {err:.3e} scale {scale:.3e}")
        assert scale > 1e-6 and err <= 1e-9 * scale + 1e-12, f"{name}: {err:.3e} vs scale {scale:.3e}"
    want2d = (proxy_c.grad + proxy_a.grad + proxy_e.grad).numpy()
    assert np.abs(got["means2D"][:, :2] - want2d).max() <= 1e-9 * max(np.abs(want2d).max(), 1e-12)
