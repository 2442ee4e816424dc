"""CPU checks of Mip-Splatting's 3D smoothing filter (diff_gaussian_rasterization/filter3d.py, csrc/gsr_filter3d.hip): the C ABI is
additive (four new symbols declared and exported, the version unchanged) and refuses what it does not support without touching a
GPU; the kernels' own per-Gaussian functions (csrc/gsr_filter3d_math.h, compiled with g++: tests/filter3d_host.cpp) and the package's
torch twins agree with the binary64 restatement (tests/filter3d_ref.py) under its error rules: a bracket for the filter size, bounds
counted in roundings for the application, forward and both gradients, raw and activated; the restatement's gradient is autograd's,
checked by gradcheck; the model's PLY layouts, refusals and opacity reset."""
import ctypes as C
import os
import re
import subprocess
from dataclasses import replace

import numpy as np
import pytest
import torch

import filter3d_ref as FR
import scene_synth as S
from diff_gaussian_rasterization import filter3d as F3
from diff_gaussian_rasterization.filter3d import apply_filter_3d, apply_filter_3d_torch, compute_filter_3d, compute_filter_3d_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_filter3d_workspace_size", "gsr_filter3d_compute", "gsr_filter3d_apply_forward", "gsr_filter3d_apply_backward")
F64, F32 = torch.float64, torch.float32
SIZES = (1, 257, 2000)


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """The g++ build of the kernels' functions: host.compute(xyz, cameras) -> (filter [P,1], seen [P]) or None when nothing is
    seen; host.apply(inputs, g_o, g_s, raw) -> (o', s', dL/do, dL/ds)."""
    d = str(tmp_path_factory.mktemp("f3d"))
    exe = os.path.join(d, "filter3d_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "filter3d_host.cpp")])
    fin, fout = os.path.join(d, "in.txt"), os.path.join(d, "out.txt")

    class Host:
        @staticmethod
        def compute(xyz, cameras):
            table, focal_max = F3.camera_table(cameras, "cpu")
            with open(fin, "w") as fh:
                fh.write(f"{xyz.shape[0]} {len(cameras)} {np.float32(focal_max):.9g}\n")
                np.savetxt(fh, table.numpy(), fmt="%.9g")
                np.savetxt(fh, xyz.numpy(), fmt="%.9g")
            rc = subprocess.call([exe, "compute", fin, fout])
            if rc == 3:
                return None
            assert rc == 0
            out = np.loadtxt(fout, dtype=np.float64, ndmin=2)
            return torch.from_numpy(out[:, 0].astype(np.float32)).reshape(-1, 1), torch.from_numpy(out[:, 1] > 0)

        @staticmethod
        def apply(inputs, g_o, g_s, raw):
            o, s, f = inputs
            rows = torch.cat((s, o.reshape(-1, 1), f.reshape(-1, 1), g_s, g_o.reshape(-1, 1)), 1).to(F32).numpy()
            with open(fin, "w") as fh:
                fh.write(f"{int(raw)}\n")
                np.savetxt(fh, rows, fmt="%.9g")
            subprocess.check_call([exe, "apply", fin, fout])
            out = torch.from_numpy(np.loadtxt(fout, dtype=np.float32, ndmin=2))
            assert out.shape == (s.shape[0], 8)
            return out[:, 3:4], out[:, 0:3], out[:, 7:8], out[:, 4:7]
    return Host


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
    consts = open(os.path.join(ROOT, "include", "gsr_constants.h")).read()
    value = lambda n: float(re.search(rf"#define\s+{n}\s+([0-9.]+)", consts).group(1))
    assert (value("GSR_NEAR_CUT"), value("GSR_F3D_VARIANCE"), value("GSR_F3D_MARGIN")) == (F3.NEAR_CUT, F3.VARIANCE, F3.MARGIN) \
        == (FR.NEAR, FR.VARIANCE, FR.MARGIN) == (0.2, 0.2, 0.15)
    src = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "gsr_filter3d.hip")).read()
    assert int(re.search(r"kF3dCamChunk = (\d+)", src).group(1)) == FR.CAM_CHUNK


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    p, bad, ws = C.c_void_p(64), C.c_void_p(66), C.c_size_t(1 << 20)
    seen = C.c_int32(7)
    i64, i32, f = C.c_int64, C.c_int32, C.c_float

    def compute(P=8, Cn=2, cams=p, focal=f(50.0), xyz=p, out=p, work=p, nbytes=ws):
        rc = lib.gsr_filter3d_compute(i64(P), i32(Cn), cams, focal, xyz, out, work, nbytes, C.byref(seen), None)
        return rc, lib.gsr_last_error()

    def fwd(P=8, o=p, s=p, flt=p, oo=p, so=p):
        rc = lib.gsr_filter3d_apply_forward(i64(P), i32(1), o, s, flt, oo, so, None)
        return rc, lib.gsr_last_error()

    def bwd(P=8, o=p, s=p, flt=p, go=p, gs=p, do=p, ds=p):
        rc = lib.gsr_filter3d_apply_backward(i64(P), i32(0), o, s, flt, go, gs, do, ds, None)
        return rc, lib.gsr_last_error()

    for call in (compute, fwd, bwd):
        rc, msg = call(P=-1)
        assert rc == -1 and b"P=-1" in msg
        assert call(P=0)[0] == 0                                     # P = 0: nothing to do, nothing read
    assert seen.value == 0
    for cn in (0, -3):
        rc, msg = compute(Cn=cn)
        assert rc == -1 and b"C=" in msg
    rc, msg = compute(focal=f(0.0))
    assert rc == -1 and b"focal_max" in msg
    for name in ("cams", "xyz", "out", "work"):
        shown = {"cams": b"cameras", "out": b"filter_out", "work": b"workspace"}.get(name, name.encode())
        rc, msg = compute(**{name: None})
        assert rc == -1 and shown in msg and b"NULL" in msg, name
        rc, msg = compute(**{name: bad})
        assert rc == -1 and shown in msg and b"aligned" in msg, name
    rc, msg = compute(cams=C.c_void_p(68))                           # the camera table is read as 16-byte vectors
    assert rc == -1 and b"cameras" in msg and b"16-byte" in msg
    rc, msg = compute(nbytes=C.c_size_t(4))
    assert rc == -1 and b"workspace_bytes" in msg
    b = C.c_size_t(0)
    assert lib.gsr_filter3d_workspace_size(i64(1000), C.byref(b)) == 0 and b.value >= 4 * (1 + 4)
    assert lib.gsr_filter3d_workspace_size(i64(-1), C.byref(b)) == -1 and lib.gsr_filter3d_workspace_size(i64(8), None) == -1
    names = {"o": b"opacities", "s": b"scales", "flt": b"filter", "oo": b"opacities_out", "so": b"scales_out"}
    for name, shown in names.items():
        rc, msg = fwd(**{name: None})
        assert rc == -1 and shown in msg and b"NULL" in msg, name
        rc, msg = fwd(**{name: bad})
        assert rc == -1 and shown in msg and b"aligned" in msg, name
    for name in ("o", "s", "flt"):
        rc, msg = bwd(**{name: None})
        assert rc == -1 and names[name] in msg and b"NULL" in msg, name
    for name, shown in (("go", b"grad_opacities_out"), ("gs", b"grad_scales_out"), ("do", b"grad_opacities"), ("ds", b"grad_scales")):
        rc, msg = bwd(**{name: bad})
        assert rc == -1 and shown in msg and b"aligned" in msg, name
    assert bwd(do=None, ds=None)[0] == 0                              # nothing wanted: nothing runs


def test_python_surface_refusals():
    xyz, cams = FR.fixture("posed1", 257)
    o, s, f = torch.zeros(257, 1), torch.zeros(257, 3), torch.ones(257, 1)
    with pytest.raises(ValueError, match="xyz"):
        compute_filter_3d(torch.zeros(5, 4), cams)
    with pytest.raises(ValueError, match="cameras"):
        compute_filter_3d(xyz, [])
    with pytest.raises(ValueError, match="scales"):
        apply_filter_3d(o, torch.zeros(257, 4), f)
    with pytest.raises(ValueError, match="opacities"):
        apply_filter_3d(torch.zeros(256, 1), s, f)
    with pytest.raises(ValueError, match="filter_3D"):
        apply_filter_3d(o, s, torch.ones(100, 1))
    with pytest.raises(ValueError, match="filter_3D is torch.float64"):
        apply_filter_3d(o, s, f.double())
    with pytest.raises(ValueError, match="opacities is torch.float16"):
        apply_filter_3d(o.half(), s, f)
    with pytest.raises(RuntimeError, match="no CPU path"):
        compute_filter_3d(xyz, cams, native=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        apply_filter_3d(o, s, f, native=True)


# ---- the filter size --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", SIZES)
@pytest.mark.parametrize("name", FR.FIXTURES)
def test_compute_twin_and_host_function_in_the_bracket(host, name, P):
    xyz, cams = FR.fixture(name, P)
    assert xyz.shape == (P, 3) and xyz.dtype == F32
    br = FR.compute_bracket(xyz, cams)
    assert not br["none"]
    if P >= 257:                                                   # the fixture exercises both rules
        assert bool((~br["seen_maybe"]).any()), "no Gaussian is unseen: the fill rule does not run"
        assert int(br["seen_sure"].sum()) >= P // 2
    twin = compute_filter_3d(xyz, cams)
    assert twin.shape == (P, 1) and twin.dtype == F32 and torch.equal(twin, compute_filter_3d_torch(xyz, cams))
    FR.check_compute(twin, br, f"twin {name} P={P}")
    got, seen = host.compute(xyz, cams)
    FR.check_compute(got, br, f"host {name} P={P}")
    assert bool(seen[br["seen_sure"]].all()) and not bool(seen[~br["seen_maybe"]].any())
    # order independence: a permutation of the cameras gives the same bits
    if len(cams) > 1:
        perm = [cams[i] for i in torch.randperm(len(cams), generator=torch.Generator().manual_seed(3)).tolist()]
        assert torch.equal(compute_filter_3d(xyz, perm), twin)
        assert torch.equal(host.compute(xyz, perm)[0], got)
    # in binary64 the twin is the rule itself
    twin64 = compute_filter_3d_torch(xyz.to(F64), cams).reshape(-1)
    dec = br["decided"]
    want = torch.where(br["seen_sure"], br["d_hi"], br["d_hi"][br["seen_sure"]].max()) * (np.sqrt(0.2) / br["focal_max"])
    assert float((twin64 - want)[dec].abs().max()) <= 1e-12 * float(want.abs().max())


def test_compute_edge_rows_one_step_inside_and_outside_each_bound(host):
    xyz, cams, rows, inside = FR.edge_fixture()
    br = FR.compute_bracket(xyz, cams)
    assert bool((~br["decided"][rows] | ~br["seen_sure"][rows]).all()), "the ten rows are meant to sit inside the undecided band"
    k = np.float32(np.sqrt(np.float32(0.2))) / np.float32(64.0)
    fill = xyz[:247][br["seen_sure"][:247], 2].max().numpy()          # identity camera: z is the depth, exactly
    want = torch.tensor([np.float32(z) * k if ins else fill * k for z, ins in zip(xyz[rows, 2].numpy(), inside.tolist())])
    twin = compute_filter_3d(xyz, cams)
    got, seen = host.compute(xyz, cams)
    FR.check_compute(twin, br, "twin edge")
    FR.check_compute(got, br, "host edge")
    assert torch.equal(seen[rows], inside)
    assert torch.equal(got[rows, 0], want) and torch.equal(twin[rows, 0], want)


def test_compute_nobody_sees_anything(host):
    cams = FR.posed_trio()
    xyz = torch.cat([FR._behind(c, 20, torch.Generator().manual_seed(1)) for c in cams[:1]])
    br = FR.compute_bracket(xyz, cams[:1])
    assert br["none"]
    with pytest.raises(ValueError, match="no Gaussian is seen"):
        compute_filter_3d(xyz, cams[:1])
    assert host.compute(xyz, cams[:1]) is None


# ---- the application ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_gradcheck_of_the_restatement(raw):
    (o, s, f), _, _ = FR.apply_case(6, 1, raw)
    leaves = [o.to(F64).requires_grad_(True), s.to(F64).requires_grad_(True)]
    assert bool((f == 0).any()) and bool((f > 0).any())
    assert torch.autograd.gradcheck(lambda a, b: FR.apply(a, b, f, raw), leaves, eps=1e-7, atol=1e-7, rtol=1e-5)


def _twin(inputs, g_o, g_s, raw):
    o, s, f = inputs
    leaves = [o.clone().requires_grad_(True), s.clone().requires_grad_(True)]
    o_out, s_out = apply_filter_3d(*leaves, f, raw=raw)
    assert o_out.shape == o.shape and s_out.shape == s.shape and o_out.dtype == F32
    d_o, d_s = torch.autograd.grad((o_out, s_out), leaves, (g_o, g_s))
    return o_out.detach(), s_out.detach(), d_o, d_s


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("P", SIZES)
def test_apply_twin_and_host_function_against_the_restatement(host, P, raw):
    inputs, g_o, g_s = FR.apply_case(P, 40 + P, raw)
    FR.check_apply(inputs, g_o, g_s, _twin(inputs, g_o, g_s, raw), raw, f"twin P={P}")
    got = host.apply(inputs, g_o, g_s, raw)
    FR.check_apply(inputs, g_o, g_s, got, raw, f"host P={P}")
    zero = (inputs[2] == 0).reshape(-1)                              # f = 0: the row passes through, and so do its gradients
    if zero.any():
        assert torch.equal(got[0][zero], inputs[0][zero]) and torch.equal(got[1][zero], inputs[1][zero])
        assert torch.equal(got[2][zero], g_o[zero]) and torch.equal(got[3][zero], g_s[zero])
    # either gradient is optional
    o, s, f = inputs
    leaf = s.clone().requires_grad_(True)
    only_s = torch.autograd.grad(apply_filter_3d(o, leaf, f, raw=raw)[1], leaf, g_s)[0]
    FR.check_apply(inputs, torch.zeros_like(g_o), g_s, (None, None, None, only_s), raw, f"twin scales only P={P}")
    # in binary64 the twin is the rule itself
    o64, s64 = apply_filter_3d_torch(o.to(F64), s.to(F64), f.to(F64), raw=raw)
    ro, rs = FR.apply(o, s, f, raw)
    assert float((o64 - ro).abs().max()) <= 1e-12 * max(1.0, float(ro.abs().max())) and float((s64 - rs).abs().max()) <= 1e-12 * max(1.0, float(rs.abs().max()))


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
def test_apply_extremes_stay_finite(host, raw):
    inputs = FR.extreme_case(raw)
    n = inputs[1].shape[0]
    g_o, g_s = torch.ones(n, 1), torch.ones(n, 3)
    for what, got in (("twin", _twin(inputs, g_o, g_s, raw)), ("host", host.apply(inputs, g_o, g_s, raw))):
        assert all(bool(torch.isfinite(t).all()) for t in got), what
        FR.check_apply(inputs, g_o, g_s, got, raw, f"{what} extremes")            # forward and both gradients, finite and in bound
        o, s, f = inputs
        zero = (f == 0).reshape(-1)
        assert torch.equal(got[0][zero], o[zero]) and torch.equal(got[1][zero], s[zero])
        # where f is negligible the scale comes back exactly: f = 1e-6 beside s = 1 or e^50 (activated: under half an ulp of s), beside
        # u = 50 (raw: 0.5 log1p((f/s)^2) is under half an ulp of u; at u = 0 it is not: u' = 5e-13 is the answer)
        small = ((f == 1e-6).reshape(-1)) & (s[:, 0] >= (50.0 if raw else 1.0))
        cols = slice(0, 1) if raw else slice(0, 3)
        assert int(small.sum()) >= 3 and torch.equal(got[1][small, cols], s[small, cols]), what


# ---- the model ------------------------------------------------------------------------------------------------------------------
def _model(P=300, D=3):
    from scene import GaussianModel, OptimizationDefaults
    gm = GaussianModel(D)
    gm.adopt_scene(S.make_scene(P, 64, 64, D, 7, zmin=0.5), device="cpu")
    gm.training_setup(OptimizationDefaults())
    return gm


def test_model_defaults_and_getters():
    from scene import OptimizationDefaults
    assert OptimizationDefaults().filter_3d is False
    gm = _model()
    assert gm.filter_3D is None
    assert torch.equal(gm.get_scaling_with_3D_filter, gm.get_scaling) and torch.equal(gm.get_opacity_with_3D_filter, gm.get_opacity)
    cov0 = gm.get_covariance()
    gm.compute_3D_filter([S.make_camera(64, 64)])
    assert gm.filter_3D.shape == (300, 1) and bool((gm.filter_3D > 0).all())
    lo, ls = apply_filter_3d(gm._opacity, gm._scaling, gm.filter_3D, raw=True)
    assert torch.equal(gm.get_scaling_with_3D_filter, torch.exp(ls)) and torch.equal(gm.get_opacity_with_3D_filter, torch.sigmoid(lo))
    assert bool((gm.get_scaling_with_3D_filter > gm.get_scaling).all()) and bool((gm.get_opacity_with_3D_filter < gm.get_opacity).all())
    assert bool((gm.get_covariance()[:, 0] > cov0[:, 0]).all())
    snap = gm.capture()
    assert len(snap) == 12                                           # capture() does not change: the filter is recomputed


def test_ply_layouts(tmp_path):
    from scene import GaussianModel, ply_io
    gm = _model()
    plain = str(tmp_path / "plain.ply")
    gm.save_ply(plain)
    direct = str(tmp_path / "direct.ply")
    n = lambda t: t.detach().numpy()
    ply_io.write_gaussian_ply(direct, n(gm._xyz), n(gm._features_dc), n(gm._features_rest), n(gm._opacity), n(gm._scaling), n(gm._rotation))
    assert open(plain, "rb").read() == open(direct, "rb").read()
    assert ply_io.property_names(45)[-1] == "rot_3" and len(ply_io.property_names(45)) == 62
    gm.compute_3D_filter([S.make_camera(64, 64)])
    with_filter = str(tmp_path / "filter.ply")
    gm.save_ply(with_filter)
    d = ply_io.read_gaussian_ply(with_filter)
    assert d["names"] == ply_io.property_names(45) + ["filter_3D"]
    gm2 = GaussianModel(3)
    gm2.load_ply(with_filter, device="cpu")
    assert torch.equal(gm2.filter_3D, gm.filter_3D) and torch.equal(gm2._scaling.detach(), gm._scaling.detach())
    gm2.load_ply(plain, device="cpu")
    assert gm2.filter_3D is None
    fused = str(tmp_path / "fused.ply")
    gm.save_ply(fused, fuse_filter=True)
    d = ply_io.read_gaussian_ply(fused)
    assert d["names"] == ply_io.property_names(45)
    lo, ls = apply_filter_3d(gm._opacity.detach(), gm._scaling.detach(), gm.filter_3D, raw=True)
    assert np.array_equal(d["opacity"], lo.numpy()) and np.array_equal(d["scaling"], ls.numpy())
    assert np.array_equal(d["rotation"], n(gm._rotation)) and np.array_equal(d["xyz"], n(gm._xyz))
    with pytest.raises(ValueError, match="fuse_filter"):
        gm.save_compressed(str(tmp_path / "model.npz"))


def test_stale_filter_and_sharded_renderer_are_refused():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    gm = _model()
    cam = S.make_camera(64, 64)
    gm.compute_3D_filter([cam])
    gm.prune_points(torch.arange(300) < 10)                          # a structural edit leaves the filter stale
    assert gm.filter_3D.shape[0] == 300 and gm._xyz.shape[0] == 290
    for pipe_kw in ({}, {"fused_activations": False}):
        pipe = Pipe()
        for k, v in pipe_kw.items():
            setattr(pipe, k, v)
        with pytest.raises(ValueError, match="compute_3D_filter"):
            render(cam, gm, pipe, torch.zeros(3))
    with pytest.raises(ValueError, match="compute_3D_filter"):
        gm.get_opacity_with_3D_filter
    gm.compute_3D_filter([cam])
    assert gm.filter_3D.shape[0] == 290
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    sharded = ShardedRenderer.__new__(ShardedRenderer)               # render() refuses before it reads anything of the renderer's
    with pytest.raises(ValueError, match="3D filter"):
        sharded.render(cam, gm, Pipe(), torch.zeros(3))


def test_reset_opacity_caps_the_filtered_opacity():
    gm = _model()
    gm.compute_3D_filter([S.make_camera(64, 64)])
    before = gm.get_opacity_with_3D_filter.detach().clone()
    assert float(before.max()) > 0.3
    gm.reset_opacity()
    after = gm.get_opacity_with_3D_filter.detach()
    assert float(after.max()) <= 0.01
    low = before.reshape(-1) < 0.009                                  # under the cap: the opacity stays what it was
    assert bool(low.any()) and float((after.reshape(-1)[low] / before.reshape(-1)[low] - 1).abs().max()) <= 1e-4
    assert bool(torch.isfinite(gm._opacity).all()) and gm.filter_3D.shape[0] == gm._xyz.shape[0]


def test_train_loop_calls_compute_only_when_the_switch_is_on(monkeypatch):
    """The schedule, on a stub: before the first render, after every densify_and_prune, every 100 iterations past densify_until_iter
    and not in the last 100; off: never."""
    import train_loop
    from scene import OptimizationDefaults
    calls = []

    class Stub:
        optimizer = None
        filter_3D = None

        def update_learning_rate(self, it): return 0.0
        def oneupSHdegree(self): pass
        def update_densification_stats(self, *a): pass
        def densify_and_prune(self, *a): calls.append(("densify", self.it))
        def reset_opacity(self): pass
        def compute_3D_filter(self, cameras): calls.append(("filter", getattr(self, "it", 0)))

    class Opt:
        def step(self, **kw): pass
        def zero_grad(self, set_to_none=True): pass

    stub = Stub()
    stub.optimizer = Opt()
    loss = torch.zeros((), requires_grad=True)
    monkeypatch.setattr(train_loop, "render", lambda cam, g, pipe, bg: dict(render=None, viewspace_points=None, visibility_filter=None, radii=None))
    monkeypatch.setattr(train_loop, "training_loss", lambda *a: loss * 1.0)

    def tick(it, l, g):
        g.it = it
    for on in (True, False):
        calls.clear()
        stub.it = 0
        opt = replace(OptimizationDefaults(), filter_3d=on, densify_from_iter=50, densification_interval=100, densify_until_iter=250)
        train_loop.train(stub, [None], [None], opt, None, torch.zeros(3), 600, on_iteration=tick)
        densify = [c for c in calls if c[0] == "densify"]
        assert len(densify) == 2
        if on:
            assert [i for i, c in enumerate(calls) if c[0] == "filter"] == [0, 2, 4, 5, 6]
            assert [c[1] for c in calls if c[0] == "filter"][3:] == [299, 399]          # (the stub's `it` is the previous iteration's)
        else:
            assert calls == densify
