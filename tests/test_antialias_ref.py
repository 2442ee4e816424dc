"""CPU checks of the anti-aliasing switch (the opacity compensation in front of the rasterizer): the C ABI is additive (two new
symbols declared and exported, no new struct, the version and the settings tuple unchanged) and refuses what it does not support
without touching a GPU; the kernels' own per-Gaussian functions (csrc/gsr_math.h opacity_compensation_one / _backward_one, compiled
with g++: tests/antialias_host.cpp) and the package's torch path agree with the binary64 restatement (tests/antialias_ref.py) under
its error rule, for activated and raw inputs; the restatement's gradient is autograd's, checked by gradcheck; the exactly
representable rows (culled, clamped) come out bit for bit; the three refusals of the Python surface raise before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import antialias_ref as AR
from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
from diff_gaussian_rasterization.antialias import compensate_opacity, compensate_opacity_torch
from util import raster_kwargs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_opacity_compensation_forward", "gsr_opacity_compensation_backward")
F64, F32 = torch.float64, torch.float32
CASES = ("p2048", "p2048_small", "p64", "posed", "mod0.5", "xclamp")


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


@pytest.fixture(scope="module")
def cases():
    return AR.scene_cases()


def _settings(scene, cam, mod=1.0, **over):
    kw = raster_kwargs(scene, cam, scale_modifier=mod, as_numpy=False)
    fields = dict(image_height=kw["image_height"], image_width=kw["image_width"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"],
                  bg=kw["bg"], scale_modifier=mod, viewmatrix=kw["viewmatrix"], projmatrix=kw["projmatrix"], sh_degree=scene.sh_degree,
                  campos=kw["campos"], prefiltered=False, debug=False)
    fields.update(over)
    return GaussianRasterizationSettings(**fields), AR.camera_of(kw)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_functions_are_declared_and_exported_and_nothing_else_moved(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert lib.gsr_version() == 12 and "#define GSR_VERSION 12" in hdr
    assert GaussianRasterizationSettings._fields == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier",
                                                     "viewmatrix", "projmatrix", "sh_degree", "campos", "prefiltered", "debug")
    consts = open(os.path.join(ROOT, "include", "gsr_constants.h")).read()
    assert re.search(r"#define\s+GSR_AA_MIN_RATIO\s+0\.000025\b", consts)
    assert (AR.NEAR, AR.FOV_CLAMP, AR.DILATE) == tuple(float(re.search(rf"#define\s+{n}\s+([0-9.]+)", consts).group(1))
                                                       for n in ("GSR_NEAR_CUT", "GSR_FOV_CLAMP", "GSR_COV2D_DILATE"))


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    desc = native.make_desc(8, 0, 0, 64, 64, 0.5, 0.5, 1.0, False, False)
    cam = native.Camera(None, 16, None, None)
    ok = native.Gaussians(16, None, None, 16, 16, 16, None, None, 0)
    grads = native.Grads(16, None, None, None, 16, 16, 16, None, None, 0)
    out = C.c_void_p(16)

    def both(d=desc, c=cam, g=ok):
        f = lib.gsr_opacity_compensation_forward(C.byref(d), C.byref(c), C.byref(g), out, None)
        msg_f = lib.gsr_last_error()
        b = lib.gsr_opacity_compensation_backward(C.byref(d), C.byref(c), C.byref(g), out, C.byref(grads), None)
        return f, b, msg_f, lib.gsr_last_error()

    f, b, mf, mb = both(g=native.Gaussians(16, None, None, 16, None, None, 16, None, 0))
    assert f == -1 and b == -1 and b"cov3D_precomp" in mf and b"cov3D_precomp" in mb
    f, b, mf, mb = both(g=native.Gaussians(16, None, None, 16, 16, None, None, None, 0))
    assert f == -1 and b == -1 and b"rotations" in mf and b"rotations" in mb
    f, b, mf, mb = both(c=native.Camera(16, None, 16, 16))
    assert f == -1 and b == -1 and b"viewmatrix" in mf and b"viewmatrix" in mb
    f, b, mf, mb = both(d=native.make_desc(-1, 0, 0, 64, 64, 0.5, 0.5, 1.0, False, False))
    assert f == -1 and b == -1 and b"P=-1" in mf and b"P=-1" in mb
    f, b, mf, mb = both(g=native.Gaussians(16, None, None, 16, 16, 20, None, None, 0))
    assert f == -1 and b == -1 and b"16-byte aligned" in mf and b"16-byte aligned" in mb
    assert lib.gsr_opacity_compensation_forward(C.byref(desc), C.byref(cam), C.byref(ok), None, None) == -1
    assert both(d=native.make_desc(0, 0, 0, 64, 64, 0.5, 0.5, 1.0, False, False))[:2] == (0, 0)        # P = 0: nothing to do, nothing read
    none_wanted = native.Grads(None, None, None, None, None, None, None, None, None, 0)
    assert lib.gsr_opacity_compensation_backward(C.byref(desc), C.byref(cam), C.byref(ok), out, C.byref(none_wanted), None) == 0


def test_python_surface_refuses_what_the_switch_does_not_support(cases):
    scene, cam, _ = cases["p64"]
    rs, _ = _settings(scene, cam)
    a = scene.activated()
    P = scene.P
    # a precomputed 3D covariance
    with pytest.raises(ValueError, match="precomputed 3D covariance"):
        GaussianRasterizer(rs, antialiasing=True)(means3D=a["means3D"], means2D=torch.zeros(P, 3), opacities=a["opacities"], shs=a["shs"],
                                                  cov3D_precomp=torch.zeros(P, 6))
    # a camera tensor that requires grad
    for name in ("viewmatrix", "projmatrix", "campos"):
        rs_g = rs._replace(**{name: getattr(rs, name).clone().requires_grad_(True)})
        with pytest.raises(ValueError, match="requires grad"):
            GaussianRasterizer(rs_g, antialiasing=True)(means3D=a["means3D"], means2D=torch.zeros(P, 3), opacities=a["opacities"],
                                                        shs=a["shs"], scales=a["scales"], rotations=a["rotations"])
        with pytest.raises(ValueError, match="requires grad"):
            GaussianRasterizer(rs_g, antialiasing=True).forward_raw(scene.means3D, torch.zeros(P, 3), scene.shs, None, scene.opacity_logits,
                                                                    scene.log_scales, scene.raw_rotations)
    # the sharded renderer
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    from gaussian_params import Pipe

    class AaPipe(Pipe):
        antialiasing = True
    sharded = ShardedRenderer.__new__(ShardedRenderer)          # render() refuses before it reads anything of the renderer's
    with pytest.raises(ValueError, match="ShardedRenderer"):
        sharded.render(cam, object(), AaPipe(), torch.zeros(3))
    assert Pipe.antialiasing is False and GaussianRasterizer(rs).antialiasing is False
    with pytest.raises(ValueError, match="expected"):
        compensate_opacity(a["opacities"], a["means3D"], torch.zeros(P, 6), a["rotations"], rs)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compensate_opacity(a["opacities"], a["means3D"], a["scales"], a["rotations"], rs, native=True)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_fixture_scenes_exercise_the_rule(cases):
    """On the binary64 side: the scenes hold what the tests below (and tests/test_gpu_antialias.py) mean to run."""
    def stats(name):
        scene, cam, mod = cases[name]
        _, c = _settings(scene, cam, mod)
        r = AR.rule(*AR.case_inputs(scene, False), c)
        return r, ~r["through"]
    r, live = stats("p2048")
    assert int(r["clamped"].sum()) == 0
    assert float((r["rho"][live] < 0.5).double().mean()) >= 0.10 and float((r["rho"][live] > 0.5).double().mean()) >= 0.10
    r, live = stats("p2048_small")
    assert int(r["clamped"].sum()) >= 50
    r, live = stats("xclamp")
    assert int((r["xmul0"] & live).sum()) >= 16
    r, live = stats("posed")
    assert int(r["through"].sum()) > 0 and int(live.sum()) > 1500


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_gradcheck_of_the_restatement(cases, raw):
    scene, cam, _ = cases["p64"]
    _, c = _settings(scene, cam)
    inputs = [t.to(F64) for t in AR.case_inputs(scene, raw)]
    r = AR.rule(*inputs, c, raw=raw)
    lim = AR.FOV_CLAMP * c["tanfovx"]
    pv = inputs[1] @ torch.as_tensor(c["V"][:3, :3]) + torch.as_tensor(c["V"][3, :3])
    away = (~r["through"] & ~r["clamped"] & (r["x"] > 1e-3) & (r["x"] < 0.99) & (pv[:, 2] > 0.5)
            & ((pv[:, 0] / pv[:, 2]).abs() < 0.9 * lim) & ((pv[:, 1] / pv[:, 2]).abs() < 0.9 * AR.FOV_CLAMP * c["tanfovy"]))
    rows = torch.nonzero(away).reshape(-1)[:4]
    assert rows.numel() == 4
    leaves = [t[rows].clone().requires_grad_(True) for t in inputs]
    assert torch.autograd.gradcheck(lambda o, p, s, q: AR.rule(o, p, s, q, c, raw=raw)["out"], leaves, eps=1e-7, atol=1e-7, rtol=1e-5)


# ---- the kernels' per-Gaussian functions on the host, and the package's torch path -------------------------------------------------
@pytest.fixture(scope="module")
def antialias_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("aa") / "antialias_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "antialias_host.cpp")])

    def run(inputs, cam, g, raw):
        """-> (out [P], {name: gradient}) float32 from opacity_compensation_one / opacity_compensation_backward_one."""
        d = os.path.dirname(exe)
        o, p, s, q = (t.to(F32) for t in inputs)
        rows = torch.cat((p, s, q, o.reshape(-1, 1), torch.as_tensor(g).to(F32).reshape(-1, 1)), 1).numpy()
        with open(os.path.join(d, "in.txt"), "w") as fh:
            fh.write(f"{cam['W']} {cam['H']} {np.float32(cam['tanfovx']):.9g} {np.float32(cam['tanfovy']):.9g} {np.float32(cam['mod']):.9g} {int(raw)}\n")
            fh.write(" ".join(f"{v:.9g}" for v in cam["V"].astype(np.float32).reshape(-1)) + "\n")
            np.savetxt(fh, rows, fmt="%.9g")
        subprocess.check_call([exe, os.path.join(d, "in.txt"), os.path.join(d, "out.txt")])
        out = torch.from_numpy(np.loadtxt(os.path.join(d, "out.txt"), dtype=np.float32, ndmin=2))
        assert out.shape == (p.shape[0], 12)
        return out[:, 0], dict(opacities=out[:, 1:2], means3D=out[:, 2:5], scales=out[:, 5:8], rotations=out[:, 8:12])
    return run


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("case", CASES)
def test_host_functions_against_the_restatement(cases, antialias_host, case, raw):
    scene, cam, mod = cases[case]
    _, c = _settings(scene, cam, mod)
    inputs = AR.case_inputs(scene, raw)
    g = AR.upstream(scene.P, 3)
    out, grads = antialias_host(inputs, c, g, raw)
    AR.check_against_ref(inputs, c, g.to(F32), out, grads, raw=raw, what=f"host {case} {'raw' if raw else 'act'}")
    zero = g == 0
    assert zero.any() and all(not grads[n][zero].any() for n in AR.GRAD_NAMES)


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("case", CASES)
def test_torch_path_against_the_restatement(cases, case, raw):
    scene, cam, mod = cases[case]
    rs, c = _settings(scene, cam, mod)
    inputs = AR.case_inputs(scene, raw)
    g = AR.upstream(scene.P, 4).to(F32)
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    out = compensate_opacity(*leaves, rs, raw=raw, native=False)          # host tensors: native=None takes the same path
    assert out.shape == inputs[0].shape and out.dtype == F32
    assert torch.equal(out, compensate_opacity(*inputs, rs, raw=raw)) and torch.equal(out, compensate_opacity_torch(*inputs, rs, raw=raw))
    grads = dict(zip(AR.GRAD_NAMES, torch.autograd.grad(out, leaves, g.reshape(out.shape))))
    AR.check_against_ref(inputs, c, g, out.detach(), grads, raw=raw, what=f"torch {case} {'raw' if raw else 'act'}")
    # in binary64 the two are the same arithmetic up to its order
    out64 = compensate_opacity_torch(*(t.to(F64) for t in inputs), rs, raw=raw)
    want = AR.rule(*inputs, c, raw=raw)["out"]
    assert float((out64 - want).abs().max()) <= 1e-9 * max(1.0, float(want.abs().max()))


def _edge_rows():
    """means3D (identity camera), scales, rotations, opacities of rows whose result is exact: two culled ones (just behind the near
    cut, behind the camera) and two far under a pixel (x < 2.5e-5: clamped)."""
    means = torch.tensor([[0.01, 0.02, 0.1999], [0.3, -0.2, -1.5], [0.1, 0.1, 3.0], [-0.4, 0.2, 5.0]])
    scales = torch.tensor([[0.02, 0.03, 0.01], [0.02, 0.03, 0.01], [1e-5, 2e-5, 1e-5], [1e-4, 1e-5, 3e-5]])
    rots = torch.nn.functional.normalize(torch.tensor([[1.0, 0.2, -0.1, 0.3], [0.5, 0.5, 0.5, 0.5], [1.0, 0.0, 0.0, 0.0], [0.3, -0.8, 0.1, 0.2]]))
    op = torch.tensor([0.7, 0.3, 0.6, 0.9])
    return op, means, scales, rots


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_edge_rows_bit_for_bit(cases, antialias_host, raw):
    import scene_synth as S
    scene, cam, _ = cases["p64"]
    rs, c = _settings(scene, S.make_camera(48, 80))
    op, means, scales, rots = _edge_rows()
    inputs = (torch.log(op / (1 - op)), means, torch.log(scales), rots * 1.7) if raw else (op, means, scales, rots)
    g = torch.tensor([0.5, -2.0, 1.5, -0.25])
    r = AR.rule(*inputs, c, raw=raw)
    assert r["through"].tolist() == [True, True, False, False] and r["clamped"].tolist() == [False, False, True, True]
    leaves = [t.clone().requires_grad_(True) for t in inputs]
    out_t = compensate_opacity(*leaves, rs, raw=raw)
    grads_t = dict(zip(AR.GRAD_NAMES, torch.autograd.grad(out_t, leaves, g)))
    out_h, grads_h = antialias_host(inputs, c, g, raw)
    for out, grads in ((out_t.detach(), grads_t), (out_h, grads_h)):
        # culled: the opacity (or the logit) passes through, its gradient too, nothing else moves
        assert torch.equal(out[:2], inputs[0][:2]) and torch.equal(grads["opacities"].reshape(-1)[:2], g[:2])
        for n in ("means3D", "scales", "rotations"):
            assert not grads[n].any(), n                      # culled or clamped: zero geometry gradient
        if not raw:                                           # clamped: opacity * 0.005, one binary32 product
            assert torch.equal(out[2:], op[2:] * np.float32(0.005)) and torch.equal(grads["opacities"].reshape(-1)[2:], g[2:] * np.float32(0.005))
    if raw:                                                   # logit(sigmoid(o) 0.005) to rounding, and the closed form of its gradient
        p = torch.sigmoid(inputs[0][2:].double())
        want = torch.log(p * 0.005) - torch.log1p(-p * 0.005)
        for out, grads in ((out_t.detach(), grads_t), (out_h, grads_h)):
            assert float((out[2:].double() - want).abs().max()) <= 4 * 2.0 ** -24 * float(want.abs().max())
            dwant = g[2:].double() * (1 - p) / (1 - p * 0.005)
            assert float((grads["opacities"].reshape(-1)[2:].double() - dwant).abs().max()) <= 8 * 2.0 ** -24 * float(dwant.abs().max())
