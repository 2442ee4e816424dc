"""CPU checks of the bilateral grid: the C ABI is additive (five new symbols declared and exported, the version and
the settings tuple unchanged) and refuses bad arguments without touching a GPU; the package's torch path in float32 and the kernels'
own per-pixel functions (csrc/gsr_bilagrid_math.h compiled by g++ under AddressSanitizer and UBSan: tests/bilagrid_host.cpp) agree
with the float64 reference (tests/bilagrid_ref.py) under its error rule; gradcheck passes on the float64 restatement; the module, the
new OptimizationDefaults and the learning-rate schedule are what DESIGN states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bilagrid_ref as BR
from diff_gaussian_rasterization import bilagrid
from scene import OptimizationDefaults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_bilagrid_workspace_size", "gsr_bilagrid_forward", "gsr_bilagrid_backward", "gsr_bilagrid_tv_forward",
                 "gsr_bilagrid_tv_backward")


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_functions_are_declared_and_exported_and_the_version_stays(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert lib.gsr_version() == 12 and "#define GSR_VERSION 12" in hdr
    import diff_gaussian_rasterization as dgr
    assert dgr.GaussianRasterizationSettings._fields == (
        "image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix", "projmatrix", "sh_degree", "campos",
        "prefiltered", "debug")


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    f = C.c_void_p(256)
    i32 = C.c_int32

    def sizes(H=1080, W=1920, L=8, Gy=16, Gx=16, b=True, t=True):
        bb, tt = C.c_size_t(0), C.c_size_t(0)
        rc = lib.gsr_bilagrid_workspace_size(i32(H), i32(W), i32(L), i32(Gy), i32(Gx), C.byref(bb) if b else None, C.byref(tt) if t else None)
        return rc, bb.value, tt.value
    rc, b, t = sizes()
    # 30 x 68 tiles of 64 x 16 pixels whose footprint is at most 3 x 3 nodes: 9 x 8 x 12 floats each
    assert rc == 0 and 30 * 68 * 9 * 96 * 4 <= b < 30 * 68 * 9 * 96 * 4 + 512 and t >= 512 * 12 + 4
    assert sizes(H=0)[:2] == (0, 0)
    # more nodes than pixels: a tile's footprint is the whole 16 x 9 of the grid it can reach
    assert sizes(H=37, W=53)[1] >= 3 * 16 * 9 * 96 * 4
    for kw in (dict(L=0), dict(Gy=0), dict(Gx=-1), dict(Gx=1025), dict(H=-1), dict(W=40000), dict(b=False, t=False)):
        assert sizes(**kw)[0] == -1, kw
    assert b"gsr_bilagrid_workspace_size" in lib.gsr_last_error()

    def fwd(N=3, L=8, Gy=16, Gx=16, H=10, W=12, idx=1, grids=f, image=f, out=f):
        rc = lib.gsr_bilagrid_forward(i32(N), i32(L), i32(Gy), i32(Gx), i32(H), i32(W), i32(idx), grids, image, out, None)
        return rc, lib.gsr_last_error()
    for kw in (dict(N=0), dict(L=0), dict(Gy=-3), dict(Gx=0), dict(H=-1), dict(W=-1)):
        assert fwd(**kw)[0] == -1, kw
    for idx in (-1, 3, 100):
        rc, msg = fwd(idx=idx)
        assert rc == -1 and b"idx" in msg
    for name in ("grids", "image", "out"):
        rc, msg = fwd(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
    assert fwd(H=0, image=None, out=None)[0] == 0 and fwd(W=0, image=None, out=None)[0] == 0

    def bwd(N=3, L=8, Gy=16, Gx=16, H=10, W=12, idx=1, grids=f, image=f, go=f, dg=f, di=f, ws=f, nbytes=1 << 30):
        rc = lib.gsr_bilagrid_backward(i32(N), i32(L), i32(Gy), i32(Gx), i32(H), i32(W), i32(idx), grids, image, go, dg, di, ws,
                                       C.c_size_t(nbytes), None)
        return rc, lib.gsr_last_error()
    for kw in (dict(N=0), dict(L=2000), dict(H=-1), dict(idx=3), dict(idx=-1)):
        assert bwd(**kw)[0] == -1, kw
    for name in ("grids", "image", "go"):
        rc, msg = bwd(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
    rc, msg = bwd(ws=None)
    assert rc == -1 and b"workspace" in msg
    rc, msg = bwd(nbytes=16)
    assert rc == native.ERR_WORKSPACE and b"needed" in msg
    assert bwd(dg=None, di=None, grids=None)[0] == 0 and bwd(H=0, image=None, go=None)[0] == 0

    def tvf(N=3, L=8, Gy=16, Gx=16, grids=f, ws=f, out=f):
        return lib.gsr_bilagrid_tv_forward(i32(N), i32(L), i32(Gy), i32(Gx), grids, ws, out, None), lib.gsr_last_error()

    def tvb(N=3, L=8, Gy=16, Gx=16, grids=f, go=f, dg=f):
        return lib.gsr_bilagrid_tv_backward(i32(N), i32(L), i32(Gy), i32(Gx), grids, go, dg, None), lib.gsr_last_error()
    for fn, names in ((tvf, ("grids", "ws", "out")), (tvb, ("grids", "go", "dg"))):
        for kw in (dict(N=0), dict(L=0), dict(Gy=0), dict(Gx=0), dict(N=1 << 20, L=1024, Gy=1024, Gx=1024)):
            assert fn(**kw)[0] == -1, kw
        for name in names:
            rc, msg = fn(**{name: None})
            assert rc == -1 and b"NULL" in msg, name


# ---- the package's torch path against the reference ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_path_float32_against_the_reference(shape):
    """The sanity check of K: a float32 evaluation by another implementation (torch's grid_sample) sits under the same bound."""
    ref = BR.reference(shape)
    grids, image = ref.grids.clone().requires_grad_(True), ref.image.clone().requires_grad_(True)
    out = bilagrid.slice_apply(grids, image, BR.IDX)
    out.backward(ref.go)
    assert out.dtype == torch.float32 and grids.grad.shape == grids.shape
    assert not grids.grad[0].any() and not grids.grad[2].any()
    BR.check_slice(ref, out.detach().numpy(), grids.grad[BR.IDX].numpy(), image.grad.numpy(), f"torch float32 {shape}")


def test_fragile_share_of_the_reference_inputs():
    for shape in BR.SHAPES:
        ref = BR.reference(shape)
        assert ref.fragile.mean() <= 0.01, shape
    ref = BR.reference(BR.SHAPES[0])
    assert 0.01 < ref.untouched[0].mean() < 0.15          # some nodes of the 37 x 53 case are reached by no pixel
    gray = (np.asarray(BR.GRAY)[:, None, None] * BR.reference(BR.SHAPES[5]).image.numpy()).sum(0)
    # the luma of three independent uniforms clamps less often than one uniform would: both sides are there all the same
    print(f"lumas clamped at 270 x 480: {(gray <= 0).mean():.2%} below 0, {(gray >= 1).mean():.2%} above 1")
    assert 0.001 < (gray <= 0).mean() < 0.06 and 0.001 < (gray >= 1).mean() < 0.06


@pytest.mark.parametrize("shape", BR.TV_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_torch_tv_float32_against_the_reference(shape):
    ref = BR.tv_reference(shape)
    grids = ref.grids.clone().requires_grad_(True)
    tv = bilagrid.total_variation_loss(grids)
    (tv * ref.upstream).backward()
    assert torch.isfinite(tv) and torch.isfinite(grids.grad).all()
    if shape[1:] == (1, 1, 1):
        assert float(tv.detach()) == 0.0 and not grids.grad.any()
    BR.check_tv(ref, float(tv.detach()), grids.grad.numpy(), f"torch float32 tv {shape}")


def test_gradcheck_on_the_float64_restatement():
    g = torch.Generator().manual_seed(5)
    for L, Gy, Gx, H, W in ((3, 4, 5, 6, 7), (1, 1, 1, 3, 2), (2, 1, 3, 4, 4)):
        grids = (torch.eye(4, dtype=torch.float64)[:3].reshape(1, 12, 1, 1, 1)
                 + 0.3 * torch.randn(2, 12, L, Gy, Gx, generator=g, dtype=torch.float64)).requires_grad_(True)
        # lumas inside (0.07, 0.93) and off the levels: gradcheck's finite differences must not straddle a kink
        image = (0.1 + 0.8 * torch.rand(3, H, W, generator=g, dtype=torch.float64))
        fz = (torch.tensor(BR.GRAY, dtype=torch.float64)[:, None, None] * image).sum(0) * (L - 1)
        image = (image + 0.02 * ((fz - fz.round()).abs() < 0.01)).requires_grad_(True)
        assert torch.autograd.gradcheck(lambda a, b: BR.slice_apply64(a, b, 1), (grids, image), eps=1e-6, atol=1e-7, rtol=1e-5)
        assert torch.autograd.gradcheck(BR.tv64, (grids,), eps=1e-6, atol=1e-7, rtol=1e-5)
        # the package's torch path is the same function of float64 tensors
        assert torch.allclose(bilagrid.slice_apply_torch(grids, image, 1), BR.slice_apply64(grids, image, 1), rtol=1e-12, atol=1e-13)
        assert torch.allclose(bilagrid.total_variation_loss_torch(grids), BR.tv64(grids), rtol=1e-13, atol=0)


# ---- the kernels' per-pixel functions on the host, under sanitizers ------------------------------------------------------------------
@pytest.fixture(scope="module")
def bilagrid_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("bilagrid")
    exe = str(d / "bilagrid_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "bilagrid_host.cpp")])

    def run(grid, image, go):
        _, L, Gy, Gx = grid.shape
        _, H, W = image.shape
        with open(d / "in.bin", "wb") as fh:
            fh.write(np.array([L, Gy, Gx, H, W], np.int32).tobytes())
            for a in (grid, image, go):
                fh.write(np.ascontiguousarray(a, np.float32).tobytes())
        subprocess.check_call([exe, str(d / "in.bin"), str(d / "out.bin")])
        flat = np.fromfile(d / "out.bin", np.float32)
        n, ng = 3 * H * W, grid.size
        assert flat.size == 2 * n + 2 * ng
        return (flat[:n].reshape(3, H, W), flat[n:2 * n].reshape(3, H, W), flat[2 * n:2 * n + ng].reshape(grid.shape),
                flat[2 * n + ng:].reshape(grid.shape))
    return run


@pytest.mark.parametrize("shape", BR.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_functions_against_the_reference(bilagrid_host, shape):
    ref = BR.reference(shape)
    out, dimage, dgrid, _ = bilagrid_host(ref.grids[BR.IDX].numpy(), ref.image.numpy(), ref.go.numpy())
    BR.check_slice(ref, out, dgrid, dimage, f"host {shape}")


def test_host_functions_at_the_edges_of_the_luma_axis(bilagrid_host):
    """Lumas far outside [0, 1], exactly 0 and 1, on every level, and a NaN: every index stays inside the grid (the sanitizers
    watch) and the finite ones meet the reference."""
    L, Gy, Gx = 8, 16, 16
    ref = BR.reference(BR.SHAPES[0])
    grid = ref.grids[BR.IDX].numpy()
    levels = np.concatenate(([-5.0, -0.0, 0.0, 1.0, 1.0 + 2.0 ** -23, 7.0, 1e30, -1e30], np.arange(L) / (L - 1)))
    image = np.broadcast_to(levels[None, None, :], (3, 2, levels.size)).astype(np.float32).copy()
    go = np.ones_like(image)
    out, dimage, dgrid, _ = bilagrid_host(grid, image, go)
    want = BR.slice_apply64(ref.grids.double(), torch.from_numpy(image).double(), BR.IDX).numpy()
    scale = np.abs(want) + 1.0
    assert np.isfinite(out).all() and (np.abs(out - want) <= 1e-4 * scale).all()
    image[:, 0, 0] = np.nan
    out, dimage, dgrid, _ = bilagrid_host(grid, image, go)
    assert np.isnan(out[:, 0, 0]).all() and np.isfinite(out[:, 1, :]).all()


@pytest.mark.parametrize("shape", BR.TV_SHAPES[1:] + ((1, 8, 16, 16),), ids=lambda s: "x".join(map(str, s)))
def test_host_tv_gradient_against_the_reference(bilagrid_host, shape):
    """The host program takes one grid: the gradient of tv over that grid alone, unit upstream."""
    N, L, Gy, Gx = shape
    grids = BR.make_tv_grids(N, L, Gy, Gx)[:1]
    g64 = grids.double().requires_grad_(True)
    BR.tv64(g64).backward()
    _, _, _, tvgrad = bilagrid_host(grids[0].numpy(), np.zeros((3, 1, 1), np.float32), np.zeros((3, 1, 1), np.float32))
    S = np.zeros(grids.shape)
    g = grids.double().numpy()
    for dim in (4, 3, 2):
        if g.shape[dim] > 1:
            d = np.abs(np.diff(g, axis=dim)) * (2.0 / (g.size // g.shape[dim] * (g.shape[dim] - 1)))
            lo, hi = [slice(None)] * 5, [slice(None)] * 5
            lo[dim], hi[dim] = slice(0, -1), slice(1, None)
            S[tuple(lo)] += d
            S[tuple(hi)] += d
    w = BR.worst(tvgrad[None], g64.grad.numpy(), S, 10)
    print(f"host tv gradient {shape}: worst error {w:.3f} x the bound")
    assert w <= 1.0 and np.isfinite(tvgrad).all()


# ---- the Python surface --------------------------------------------------------------------------------------------------------------
def test_module_surface_and_refusals():
    m = bilagrid.BilateralGrid(5)
    assert tuple(m.grids.shape) == (5, 12, 8, 16, 16) and m.grids.dtype == torch.float32 and m.grids.is_contiguous()
    assert list(m.state_dict()) == ["grids"]
    eye = torch.eye(4)[:3].reshape(12)
    assert torch.equal(m.grids, eye.view(1, 12, 1, 1, 1).expand_as(m.grids))
    m2 = bilagrid.BilateralGrid(2, grid_x=4, grid_y=3, grid_w=2)
    assert tuple(m2.grids.shape) == (2, 12, 2, 3, 4)
    image = torch.rand(3, 9, 11) * 1.3 - 0.1
    assert torch.allclose(m(image, 3), image, atol=1e-6)                 # the identity transform, wherever the luma falls
    assert float(m.tv_loss().detach()) == 0.0
    with pytest.raises(RuntimeError, match="native=True needs device tensors"):
        bilagrid.slice_apply(m.grids, image, 0, native=True)
    with pytest.raises(RuntimeError, match="native=True needs device tensors"):
        bilagrid.total_variation_loss(m.grids, native=True)
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.slice_apply(m.grids, image.double(), 0)
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.slice_apply(m.grids, image.transpose(1, 2), 0)
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.slice_apply(m.grids.double(), image, 0)
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.total_variation_loss(m.grids.transpose(3, 4))
    with pytest.raises(IndexError):
        bilagrid.slice_apply(m.grids, image, 5)
    with pytest.raises(ValueError, match=r"\[N, 12, L, Gy, Gx\]"):
        bilagrid.slice_apply(torch.zeros(2, 9, 2, 2, 2), image, 0)
    with pytest.raises(ValueError, match=r"\[3, H, W\]"):
        bilagrid.slice_apply(m.grids, torch.zeros(4, 5, 5), 0)
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    with pytest.raises(ValueError, match="bilateral_grid"):
        ShardedRenderer(None, 1, 0, bilateral_grid=True)


def test_optimization_defaults():
    d = OptimizationDefaults()
    assert d.bilateral_grid is False and d.bilateral_grid_shape == (16, 16, 8)
    assert d.bilateral_grid_lr == 2e-3 and d.bilateral_grid_tv == 10.0


def test_learning_rate_schedule_against_its_closed_form():
    """gsplat chains LinearLR(start_factor=0.01, total_iters=1000) with ExponentialLR(gamma = 0.01 ** (1 / iterations))."""
    lr, iterations = 2e-3, 30_000
    f = lambda it: bilagrid.bilateral_grid_lr(lr, it, iterations)
    assert f(0) == pytest.approx(lr * 0.01, rel=1e-12)
    assert f(500) == pytest.approx(lr * (0.01 + 0.99 * 0.5) * 0.01 ** (500 / iterations), rel=1e-12)
    assert f(1000) == pytest.approx(lr * 0.01 ** (1000 / iterations), rel=1e-12)
    assert f(iterations) == pytest.approx(lr * 0.01, rel=1e-12)
    # against torch's own chained schedulers, stepped
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=lr)
    n = 3000
    sched = torch.optim.lr_scheduler.ChainedScheduler([
        torch.optim.lr_scheduler.LinearLR(opt, start_factor=0.01, total_iters=1000),
        torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.01 ** (1.0 / n))])
    for it in range(n + 1):
        if it in (0, 1, 500, 999, 1000, 1001, n):
            assert opt.param_groups[0]["lr"] == pytest.approx(bilagrid.bilateral_grid_lr(lr, it, n), rel=1e-9), it
        opt.step()
        sched.step()
