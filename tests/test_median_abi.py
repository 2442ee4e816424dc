"""CPU-only checks of the median depth map (GaussianRasterizer(depth_alpha=True, median_depth=True)): the C ABI is
additive (three new symbols in include/gsrast_median.h, which gsrast.h includes; the version unchanged) and its ctypes table agrees
with that header's prototypes; everything the feature refuses before a launch is a ValueError (or a status with a message); and
normals.surface_depth has its identities on host tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from test_abi import header_prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_forward_render_median", "gsr_forward_median", "gsr_backward_render_median")


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def _median_header():
    with open(os.path.join(ROOT, "include", "gsrast_median.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_functions_are_declared_and_exported_and_the_version_stays(native):
    main = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert '#include "gsrast_median.h"' in main and "#define GSR_VERSION 12" in main
    protos = header_prototypes(_median_header())
    assert tuple(protos) == NEW_FUNCTIONS == tuple(native.MEDIAN_SIGNATURES)
    bad = signature_mismatches(protos, native.MEDIAN_SIGNATURES, native.MIRRORS)
    assert not bad, "\n".join(bad)
    lib = native.load()
    for name, (restype, argtypes) in native.MEDIAN_SIGNATURES.items():
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert getattr(lib, name).restype is restype and tuple(getattr(lib, name).argtypes) == tuple(argtypes), name
        assert name not in native.SIGNATURES and name not in native.EXTRA_SIGNATURES
    assert lib.gsr_version() == 12
    assert "typedef" not in _median_header()                         # no struct of its own: gsrast.h's mirrors stay the whole set
    mk = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "gsrast_median.h" in mk


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    desc = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False)
    slab = native.make_desc(1000, 3, 16, 100, 60, 0.5, 0.5, 1.0, False, False, tile_rows=(0, 2))
    cam = native.Camera(256, 256, 256, 256)
    g = native.Gaussians(256, 256, None, 256, 256, 256, None)
    aux = native.AuxOutputs(256, 256, 256)
    p, odd = C.c_void_p(256), C.c_void_p(258)
    plan = native.FramePlan()
    plan.num_rendered, plan.num_chunks = 10, 1

    def fwd(d=desc, a=aux, median=p, enc=p):
        rc = lib.gsr_forward_render_median(C.byref(d), C.byref(cam), C.byref(g), p, p, p, C.byref(plan), p, a, median, enc, None)
        return rc, lib.gsr_last_error()

    def both(d=desc, a=aux, median=p, enc=p):
        rc = lib.gsr_forward_median(C.byref(d), C.byref(cam), C.byref(g), p, p, p, C.byref(plan), p, 100, p, None, a, median, enc, None)
        return rc, lib.gsr_last_error()

    def bwd(d=desc, a=aux, median=None, enc=p):
        rc = lib.gsr_backward_render_median(C.byref(d), C.byref(cam), p, p, p, p, C.byref(plan), p, a, p, None, None, enc, None, p, None)
        return rc, lib.gsr_last_error()

    for call in (fwd, both, bwd):
        cases = [(dict(enc=None), b"median_enc is NULL"), (dict(enc=odd), b"4-byte aligned"), (dict(a=None), b"aux is required"),
                 (dict(d=slab), b"whole images only")]
        if call is not bwd:
            cases += [(dict(median=None), b"median is NULL"), (dict(median=odd), b"4-byte aligned")]
        for kw, word in cases:
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, rc, msg)
    for who in ("forward_render", "forward_both"):
        with pytest.raises(ValueError, match="aux required"):
            native._variant(who, None, None, None, median=(None, None))
        with pytest.raises(ValueError, match="no extra"):
            native._variant(who, aux, None, None, extra=(None, None), median=(None, None))


def _rasterizer(depth_alpha=True, median_depth=True, **kw):
    import diff_gaussian_rasterization as dgr
    rs = dgr.GaussianRasterizationSettings(32, 32, .5, .5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0, torch.zeros(3), False, False)
    return dgr.GaussianRasterizer(rs, depth_alpha=depth_alpha, median_depth=median_depth, **kw)


def _call(rast, raw=False, P=4, **kw):
    z = torch.zeros(P, 3)
    if raw:
        return rast.forward_raw(z, z.clone(), torch.zeros(P, 1, 3), torch.zeros(P, 0, 3), torch.zeros(P, 1), z, torch.zeros(P, 4), **kw)
    return rast(means3D=z, means2D=z.clone(), opacities=torch.zeros(P, 1), shs=torch.zeros(P, 1, 3), scales=z, rotations=torch.zeros(P, 4), **kw)


def test_constructor_refusals():
    from diff_gaussian_rasterization.contrib import ContributionStats
    with pytest.raises(ValueError, match="median_depth.*depth_alpha=True"):
        _rasterizer(depth_alpha=False)
    with pytest.raises(ValueError, match="median_depth.*absgrad"):
        _rasterizer(depth_alpha=False, absgrad=True)
    with pytest.raises(ValueError, match="absgrad"):
        _rasterizer(absgrad=True)
    with pytest.raises(ValueError, match="median_depth.*contributions"):
        _rasterizer(contributions=ContributionStats(4, device="cpu"))
    assert _rasterizer().median_depth is True and _rasterizer(median_depth=False).median_depth is False


@pytest.mark.parametrize("raw", [False, True], ids=["forward", "forward_raw"])
def test_refusals_before_any_launch_are_value_errors(raw):
    """Host tensors throughout: a call that got past these checks would raise the RuntimeError of the missing HIP device instead."""
    import diff_gaussian_rasterization as dgr
    with pytest.raises(ValueError, match="median_depth: not with extra_colors"):
        _call(_rasterizer(), raw, extra_colors=torch.zeros(4, 3))
    # past every check: the call reaches the native forward, which has no CPU path
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call(_rasterizer(), raw)
    z = torch.zeros(4, 3)
    rs = _rasterizer().raster_settings
    args = (z, torch.zeros(4, 1, 3), None, torch.zeros(4, 1), z, torch.zeros(4, 4), None, rs)
    with pytest.raises(ValueError, match="median_depth.*tile_rows"):
        dgr.rasterize_forward(*args, tile_rows=(0, 1), aux=True, median=True)
    with pytest.raises(ValueError, match="median_depth.*depth_alpha=True"):
        dgr.rasterize_forward(*args, median=True)
    with pytest.raises(ValueError, match="median_depth.*extra_colors"):
        dgr.rasterize_forward(*args, aux=True, median=True, extra=torch.zeros(4, 3))
    with pytest.raises(ValueError, match="median_depth.*depth_alpha=True"):
        dgr.rasterize_gaussians(z, z.clone(), torch.zeros(4, 1, 3), torch.zeros(0), torch.zeros(4, 1), z, torch.zeros(4, 4), torch.zeros(0), rs,
                                median_depth=True)


def test_renderer_sharded_renderer_and_training_flags_refuse():
    import gaussian_renderer as GR
    import train_loop
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    from gaussian_params import Pipe
    from scene import mesh
    from scene.gaussian_model import OptimizationDefaults
    r = ShardedRenderer.__new__(ShardedRenderer)                    # (the refusals come before anything of the instance is read)
    with pytest.raises(ValueError, match="median_depth is not supported by ShardedRenderer"):
        r.render(None, None, None, None, median_depth=True)
    pipe = Pipe()
    with pytest.raises(ValueError, match="median_depth.*depth_alpha=True"):
        GR.render(None, None, pipe, None, median_depth=True)
    with pytest.raises(ValueError, match="median_depth.*extra_colors"):
        GR.render(None, None, pipe, None, depth_alpha=True, median_depth=True, extra_colors=torch.zeros(4, 3))
    pipe.absgrad = True
    with pytest.raises(ValueError, match="median_depth.*absgrad"):
        GR.render(None, None, pipe, None, depth_alpha=True, median_depth=True)
    pipe.absgrad = False
    with pytest.raises(ValueError, match="render_with_normals: depth_ratio must be 0"):
        GR.render_with_normals(None, None, pipe, None, depth_ratio=1.0)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="depth_ratio"):
            GR.render_normals(None, None, pipe, depth_ratio=bad)
        with pytest.raises(ValueError, match="depth_ratio"):
            mesh.fuse_depth_maps(None, [], pipe, None, None, depth_ratio=bad)
    assert OptimizationDefaults().depth_ratio == 0.0
    opt = OptimizationDefaults()
    opt.lambda_normal, opt.normal_in_frame, opt.depth_ratio = 0.05, True, 1.0
    with pytest.raises(ValueError, match="normal_in_frame with depth_ratio"):
        train_loop.train(None, [], [], opt, None, None, 0)
    opt.normal_in_frame, opt.depth_ratio = False, 2.0
    with pytest.raises(ValueError, match="depth_ratio = 2.0"):
        train_loop.train(None, [], [], opt, None, None, 0)


def test_surface_depth_identities():
    from diff_gaussian_rasterization.normals import surface_depth
    g = torch.Generator().manual_seed(3)
    alpha = torch.rand(1, 24, 40, generator=g) * 0.98 + 0.01
    median = torch.rand(1, 24, 40, generator=g) * 9 + 0.3
    depth = alpha * (torch.rand(1, 24, 40, generator=g) * 9 + 0.3)
    assert surface_depth(depth, alpha, median, 0.0) is depth                     # r = 0: the same tensor
    one = surface_depth(depth, alpha, median, 1.0)
    z = (one / alpha).double()
    ulp = np.spacing(median.numpy().astype(np.float32)).astype(np.float64)       # r = 1: z = D / alpha is the median within 1 ulp
    assert (np.abs(z.numpy() - median.double().numpy()) <= ulp).all()
    half = surface_depth(depth, alpha, median, 0.25)
    want = 0.75 * depth.double() + 0.25 * alpha.double() * median.double()
    assert (half.double() - want).abs().max() <= 4 * 2.0 ** -24 * float(want.abs().max())
    for bad in (-1e-3, 1.0001, float("nan")):
        with pytest.raises(ValueError, match="depth_ratio"):
            surface_depth(depth, alpha, median, bad)
    with pytest.raises(ValueError, match="one shape"):
        surface_depth(depth, alpha, median[:, :3], 0.5)


@pytest.mark.parametrize("r", [0.0, 0.3, 1.0])
def test_surface_depth_gradient_against_autograd_in_float64(r):
    from diff_gaussian_rasterization.normals import surface_depth
    g = torch.Generator().manual_seed(5)
    depth, alpha, median = (torch.rand(1, 8, 12, generator=g, dtype=torch.float64).requires_grad_(True) for _ in range(3))
    up = torch.rand(1, 8, 12, generator=g, dtype=torch.float64) - 0.5
    (surface_depth(depth, alpha, median, r) * up).sum().backward()
    want = {"depth": (1 - r) * up, "alpha": r * median.detach() * up, "median": r * alpha.detach() * up}
    for name, t in (("depth", depth), ("alpha", alpha), ("median", median)):
        got = torch.zeros_like(up) if t.grad is None else t.grad
        assert (got - want[name]).abs().max() <= 1e-15, name
    assert torch.autograd.gradcheck(lambda d, a, m: surface_depth(d, a, m, r), (depth, alpha, median), eps=1e-6, atol=1e-8)
