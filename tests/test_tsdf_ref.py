"""CPU checks of TSDF fusion and mesh extraction (diff_gaussian_rasterization/tsdf.py, csrc/gsr_tsdf.hip, scene/mesh.py; DESIGN section
26): the C ABI is additive (four new symbols in include/gsrast_tsdf.h, which gsrast.h includes; the version unchanged), its ctypes
table agrees with the header's prototypes, and every refusal comes without touching a GPU; the package's torch twins and the kernels'
own per-element functions (csrc/gsr_tsdf_math.h compiled by g++ under AddressSanitizer and UBSan: tests/tsdf_host.cpp, a stand-alone
program run as a subprocess) agree with the binary64 restatement (tests/tsdf_ref.py) under its error rule, fragile voxels by their
reachable states; on every fixture the fragile (voxel, frame) pairs are at most 1 % of the updates; surface nets on an analytic sphere
is a closed, consistently oriented surface of genus 0 whose vertices lie on the sphere as closely as the reference's own; no face
touches a cell with an unobserved corner; a volume of three rounds of the extraction's block scan holds what the kernel test needs of
it, and its reference tells a scan with a wrong carry between rounds from the right one; the PLY file reads back.  Every test prints
the figures it judged."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tsdf_ref as TR
from test_abi import header_prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_tsdf_integrate", "gsr_tsdf_mesh_workspace_size", "gsr_tsdf_mesh_count", "gsr_tsdf_mesh_emit")
F64, F32 = torch.float64, torch.float32
FUSION_CASES = [(g, W, H) for g in TR.GRIDS for W, H in TR.MAPS]


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


@functools.lru_cache(maxsize=None)
def fusion_reference(grid_name, W, H):
    """(grid, frames, fuse_tracked(...)) of a fusion case: computed once and shared, here and in tests/test_gpu_tsdf.py."""
    grid, frames = TR.GRIDS[grid_name], TR.make_frames(W, H)
    return grid, frames, TR.fuse_tracked(grid, frames)


def make_volume(grid, device="cpu", dtype=F32):
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    return TSDFVolume(grid.origin, float(grid.voxel), grid.dims, float(grid.trunc), device=device, dtype=dtype)


def integrate_frames(vol, frames, native=None):
    t = lambda a: torch.as_tensor(a, dtype=vol.tsdf.dtype, device=vol.tsdf.device).contiguous()
    for fr in frames:
        vol.integrate(t(fr.depth)[None], t(fr.alpha)[None], t(fr.color), t(fr.V), fr.tanfovx, fr.tanfovy, alpha_min=fr.alpha_min,
                      depth_max=fr.depth_max, native=native)
    return vol


def volume_arrays(vol):
    return vol.tsdf.detach().cpu().numpy().reshape(-1), vol.weight.detach().cpu().numpy().reshape(-1), vol.color.detach().cpu().numpy().reshape(3, -1)


def ratio(got, want: TR.Tracked, what):
    got = torch.as_tensor(np.asarray(got), dtype=F64).reshape(want.v.shape)
    err = (got - want.v).abs()
    assert (err[want.e == 0] == 0).all(), f"{what}: a value whose bound is zero is not exact"
    pos = want.e > 0
    r = float((err[pos] / want.e[pos]).max()) if pos.any() else 0.0
    print(f"{what}: worst error / bound = {r:.3f}")
    return r


def check_mesh(got, ref, what):
    """(vertices, faces, colors) of an implementation against surface_nets_ref: the faces integer for integer, the vertex count, the
    vertices and colours within the replayed bound."""
    v, f, c = (np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a) for a in got)
    assert v.shape == tuple(ref["vertices"].v.shape) and c.shape == v.shape, f"{what}: {v.shape[0]} vertices, the reference has {ref['vertices'].v.shape[0]}"
    assert f.shape == ref["faces"].shape and np.array_equal(f.astype(np.int64), ref["faces"]), f"{what}: the faces differ"
    assert ratio(v, ref["vertices"], what + " vertices") <= 1
    assert ratio(c, ref["colors"], what + " colours") <= 1


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def _tsdf_header():
    with open(os.path.join(ROOT, "include", "gsrast_tsdf.h")) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_functions_are_declared_and_exported_and_the_version_stays(native):
    main = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert '#include "gsrast_tsdf.h"' in main and "#define GSR_VERSION 12" in main
    protos = header_prototypes(_tsdf_header())
    assert tuple(protos) == NEW_FUNCTIONS == tuple(native.TSDF_SIGNATURES)
    bad = signature_mismatches(protos, native.TSDF_SIGNATURES, native.MIRRORS)
    assert not bad, "\n".join(bad)
    lib = native.load()
    for name, (restype, argtypes) in native.TSDF_SIGNATURES.items():
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert getattr(lib, name).restype is restype and tuple(getattr(lib, name).argtypes) == tuple(argtypes), name
        assert name not in native.SIGNATURES and name not in native.NORMALS_SIGNATURES and name not in native.EXTRA_SIGNATURES
    assert lib.gsr_version() == 12
    assert "typedef" not in _tsdf_header()                           # no struct of its own: gsrast.h's mirrors stay the whole set
    mk = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "gsr_tsdf.hip" in mk and "gsr_tsdf_math.h" in mk and "gsrast_tsdf.h" in mk


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gsrast.h"\nint main(void) { size_t b; return gsr_tsdf_mesh_workspace_size(0, 0, 0, &b) != 0 ? 0 : 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    p, odd = C.c_void_p(256), C.c_void_p(258)
    inf = float("inf")

    def fuse(nx=8, ny=8, nz=8, vs=0.1, tr=0.3, H=8, W=9, tx=0.5, ty=0.5, am=0.5, dm=inf, V=p, d=p, a=p, c=p, t=p, w=p, vc=p, ox=0.0):
        return lib.gsr_tsdf_integrate(nx, ny, nz, ox, 0.0, 0.0, vs, tr, H, W, tx, ty, am, dm, V, d, a, c, t, w, vc, None), lib.gsr_last_error()

    for kw in (dict(nx=0), dict(nz=-1), dict(nx=2048, ny=2048, nz=512), dict(nx=65536, ny=65536, nz=1), dict(vs=0.0), dict(vs=-1.0), dict(vs=inf),
               dict(tr=0.0), dict(tr=float("nan")), dict(H=-1), dict(W=40000), dict(tx=0.0), dict(ty=inf), dict(am=0.0), dict(am=float("nan")),
               dict(dm=0.0), dict(dm=float("nan")), dict(ox=float("nan"))):
        rc, msg = fuse(**kw)
        assert rc == -1 and b"gsr_tsdf_integrate" in msg, kw
    for name, shown in (("V", b"viewmatrix"), ("d", b"depth"), ("a", b"alpha"), ("c", b"color"), ("t", b"tsdf"), ("w", b"weight"), ("vc", b"vol_color")):
        rc, msg = fuse(**{name: None})
        assert rc == -1 and shown in msg and b"NULL" in msg
        rc, msg = fuse(**{name: odd})
        assert rc == -1 and shown in msg and b"aligned" in msg
    assert fuse(H=0, d=None, a=None, c=None)[0] == 0                 # an image without pixels: nothing is read
    assert fuse(nx=2047, ny=2048, nz=512, H=0)[0] == 0               # 2^31 - 2^20 voxels: inside the limit

    b = C.c_size_t(7)
    assert lib.gsr_tsdf_mesh_workspace_size(1, 9, 9, b) == 0 and b.value == 0            # thinner than 2 voxels: no cell
    assert lib.gsr_tsdf_mesh_workspace_size(512, 512, 512, b) == 0
    blocks = 512 ** 3 // 256
    assert 48 * blocks <= b.value <= 48 * blocks + 4 * 256                                # 4 ballot words, a count and a prefix per block
    assert lib.gsr_tsdf_mesh_workspace_size(2048, 2048, 512, b) == -1 and lib.gsr_tsdf_mesh_workspace_size(4, 4, 4, None) == -1
    nv, nf = C.c_int64(5), C.c_int64(5)

    def count(nx=8, ny=8, nz=8, mw=1.0, t=p, w=p, ws=p, nb=1 << 20, v=nv, f=nf):
        return lib.gsr_tsdf_mesh_count(nx, ny, nz, mw, t, w, ws, nb, v, f, None), lib.gsr_last_error()

    def emit(nx=8, ny=8, nz=8, vs=0.1, mw=1.0, t=p, w=p, c=p, ws=p, nb=1 << 20, v=4, f=2, ov=p, of=p, oc=p):
        return lib.gsr_tsdf_mesh_emit(nx, ny, nz, 0.0, 0.0, 0.0, vs, mw, t, w, c, ws, nb, v, f, ov, of, oc, None), lib.gsr_last_error()

    assert count(nx=1, t=None, w=None, ws=None)[0] == 0 and nv.value == 0 and nf.value == 0
    for call in (count, emit):
        for kw, word in ((dict(nx=-1), b"voxels"), (dict(mw=float("nan")), b"NaN"), (dict(t=None), b"tsdf is NULL"), (dict(w=odd), b"aligned"),
                         (dict(ws=None), b"workspace is NULL"), (dict(ws=C.c_void_p(128)), b"256-byte")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, msg)
        rc, msg = call(nb=8)
        assert rc == native.ERR_WORKSPACE and b"workspace_bytes" in msg
    assert count(v=None)[0] == -1
    for kw in (dict(vs=0.0), dict(v=-1), dict(f=3), dict(c=None), dict(ov=None), dict(of=None), dict(oc=odd)):
        assert emit(**kw)[0] == -1, kw
    assert emit(v=0, f=0, t=None, w=None, c=None, ws=None, ov=None, of=None, oc=None)[0] == 0   # an empty mesh: nothing is read


def test_python_refusals_are_value_errors_and_native_on_host_raises():
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    for kw in (dict(dims=(2048, 2048, 512)), dict(dims=(4, 0, 4)), dict(dims=(4, 4)), dict(voxel_size=0.0), dict(voxel_size=-0.1),
               dict(voxel_size=float("inf")), dict(sdf_trunc=0.0), dict(sdf_trunc=float("nan")), dict(origin=(0.0, float("nan"), 0.0)),
               dict(dtype=torch.float16)):
        args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 4, 4), sdf_trunc=0.3, device="cpu")
        args.update(kw)
        with pytest.raises(ValueError):
            TSDFVolume(**args)
    vol = TSDFVolume((0.0, 0.0, 0.0), 0.1, (4, 5, 6), 0.3, device="cpu")
    assert vol.tsdf.shape == (6, 5, 4) and vol.weight.shape == (6, 5, 4) and vol.color.shape == (3, 6, 5, 4)
    assert all(t.dtype == F32 and t.is_contiguous() and float(t.abs().sum()) == 0 for t in (vol.tsdf, vol.weight, vol.color))
    d, a, c, V = torch.ones(1, 6, 7), torch.ones(1, 6, 7), torch.ones(3, 6, 7), torch.eye(4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.integrate(d, a, c, V, 0.5, 0.5, native=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vol.extract_mesh(native=True)
    ok = dict(depth=d, alpha=a, color=c, viewmatrix=V, tanfovx=0.5, tanfovy=0.5)
    for bad in (dict(depth=torch.ones(2, 6, 7)), dict(alpha=torch.ones(1, 6, 8)), dict(color=torch.ones(4, 6, 7)), dict(viewmatrix=torch.eye(3)),
                dict(depth=d.double()), dict(color=torch.ones(3, 7, 6).transpose(1, 2)), dict(tanfovx=0.0), dict(alpha_min=0.0), dict(depth_max=0.0),
                dict(depth_max=float("nan")), dict(depth=np.ones((1, 6, 7), np.float32)), dict(depth=d.clone().requires_grad_(True)),
                dict(alpha=a.clone().requires_grad_(True)), dict(color=c.clone().requires_grad_(True))):
        with pytest.raises(ValueError):
            vol.integrate(**{**ok, **bad})
    assert float(vol.weight.sum()) == 0                                         # no refused call wrote anything
    with torch.no_grad():                                                       # grad mode off: a map that requires grad is a constant
        vol.integrate(d.clone().requires_grad_(True), a, c, V, 0.5, 0.5)
    import types

    from diff_gaussian_rasterization.sharded import ShardedRenderer
    r = ShardedRenderer.__new__(ShardedRenderer)
    with pytest.raises(ValueError, match="extract_mesh"):
        r.extract_mesh(None, [], None, None)
    with pytest.raises(ValueError, match="ShardedRenderer"):
        r.fuse_depth_maps(None, [], None, None, None)
    from scene import mesh
    with pytest.raises(ValueError, match="no cameras"):
        mesh.extract_mesh(None, [], None, None)
    cam = types.SimpleNamespace(camera_center=torch.zeros(3))
    with pytest.raises(ValueError, match="one centre"):
        mesh.extract_mesh(None, [cam, cam], None, None)


# ---- fusion -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tsdf"))
    exe = os.path.join(d, "tsdf_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "tsdf_host.cpp")])
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")

    class Host:
        @staticmethod
        def fuse(grid, frames):
            with open(fin, "wb") as fh:
                np.array(list(grid.dims) + [len(frames)], np.int32).tofile(fh)
                np.array(list(grid.origin) + [grid.voxel, grid.trunc], np.float32).tofile(fh)
                for fr in frames:
                    np.array([fr.H, fr.W], np.int32).tofile(fh)
                    np.array([fr.tanfovx, fr.tanfovy, fr.alpha_min, fr.depth_max], np.float32).tofile(fh)
                    for arr in (fr.V, fr.depth, fr.alpha, fr.color):
                        np.ascontiguousarray(arr, np.float32).tofile(fh)
            subprocess.check_call([exe, "fuse", fin, fout])
            out = np.fromfile(fout, np.float32)
            n = grid.n
            assert out.size == 5 * n
            return out[:n], out[n:2 * n], out[2 * n:].reshape(3, n)

        @staticmethod
        def mesh(grid, tsdf, weight, color, min_weight=1.0):
            with open(fin, "wb") as fh:
                np.array(grid.dims, np.int32).tofile(fh)
                np.array(list(grid.origin) + [grid.voxel, min_weight], np.float32).tofile(fh)
                for arr in (tsdf, weight, color):
                    np.ascontiguousarray(arr, np.float32).tofile(fh)
            subprocess.check_call([exe, "mesh", fin, fout])
            with open(fout, "rb") as fh:
                nv, nf = np.fromfile(fh, np.int32, 2)
                v = np.fromfile(fh, np.float32, 3 * nv).reshape(nv, 3)
                c = np.fromfile(fh, np.float32, 3 * nv).reshape(nv, 3)
                f = np.fromfile(fh, np.int32, 3 * nf).reshape(nf, 3)
            return v, f, c
    return Host


@pytest.mark.parametrize("grid_name, W, H", FUSION_CASES)
def test_fusion_reference_forms_agree_and_fragile_voxels_stay_under_the_cap(grid_name, W, H):
    grid, frames, ref = fusion_reference(grid_name, W, H)
    TR.assert_cap(ref, f"{grid_name} {W}x{H}")
    tsdf, weight, color, updates = TR.fuse_ref(grid, frames)
    robust = ~ref["fragile"].numpy()
    st = ref["state"]
    assert np.array_equal(weight[robust], st.weight.numpy()[robust])
    assert np.abs(tsdf - st.tsdf.v.numpy())[robust].max() <= 1e-12
    assert max(np.abs(color[c] - st.color[c].v.numpy())[robust].max() for c in range(3)) <= 1e-12
    assert abs(updates - ref["updates"]) <= ref["fragile_events"]
    if grid.n > 1:                                                               # the fixture holds what the issue asks of it
        assert any((TR._view(grid, fr, np.arange(grid.n))[2].v <= 0).any() for fr in frames), "no voxel behind a camera"
        assert 0 < float((st.weight == 0).sum()) and float(st.weight.max()) >= 2, "no skipped voxel, or no running mean"
        assert any(np.isfinite(fr.depth_max) for fr in frames) and any((~fr.valid & (fr.alpha > 0)).any() for fr in frames)


@pytest.mark.parametrize("grid_name, W, H", FUSION_CASES)
def test_fusion_twin_and_host_program_follow_the_reference(host, grid_name, W, H):
    grid, frames, ref = fusion_reference(grid_name, W, H)
    tag = f"{grid_name} {W}x{H}"
    assert TR.check_volume(*host.fuse(grid, frames), ref, "host " + tag) <= 1
    assert TR.check_volume(*volume_arrays(integrate_frames(make_volume(grid), frames)), ref, "twin fp32 " + tag) <= 1
    t64, w64, c64 = volume_arrays(integrate_frames(make_volume(grid, dtype=F64), frames))
    robust = ~ref["fragile"].numpy()
    st = ref["state"]
    assert np.array_equal(w64[robust], st.weight.numpy()[robust]) and np.abs(t64 - st.tsdf.v.numpy())[robust].max() <= 1e-12
    assert max(np.abs(c64[c] - st.color[c].v.numpy())[robust].max() for c in range(3)) <= 1e-12


def test_skipped_voxels_keep_every_bit_in_the_twin_and_on_the_host(host):
    grid, frames, ref = fusion_reference("17x9x21", 33, 17)
    vol = make_volume(grid)
    g = torch.Generator().manual_seed(3)
    for t in (vol.tsdf, vol.weight, vol.color):                                  # random bits, NaNs and infinities among them
        t.view(torch.int32).copy_(torch.randint(-2 ** 31, 2 ** 31 - 1, t.shape, generator=g, dtype=torch.int64).to(torch.int32))
    before = [t.clone() for t in (vol.tsdf, vol.weight, vol.color)]
    integrate_frames(vol, frames)
    untouched = (ref["state"].weight == 0) & ~ref["fragile"]
    assert int(untouched.sum()) > 0
    m = untouched.reshape(vol.tsdf.shape)
    for now, was in zip((vol.tsdf, vol.weight, vol.color), before):
        mm = m if now.dim() == 3 else m[None].expand_as(now)
        assert torch.equal(now.view(torch.int32)[mm], was.view(torch.int32)[mm])


# ---- surface nets -------------------------------------------------------------------------------------------------------------
def sphere_checks(grid, vertices, faces, ref_vertices, what):
    """The four topological checks and the distance from the sphere (at most twice the reference's own)."""
    topo = TR.mesh_topology(faces)
    vol = TR.signed_volume(vertices, faces)
    dev, dev_ref = TR.sphere_deviation(grid, vertices), TR.sphere_deviation(grid, ref_vertices)
    print(f"{what}: V = {len(vertices)}, F = {len(faces)}, Euler = {topo['euler']}, volume = {vol:.4f} "
          f"(the sphere's {4.0 / 3.0 * np.pi * TR.SPHERE_R ** 3:.4f}), largest distance from the sphere {dev:.4f} voxels (reference {dev_ref:.4f})")
    assert topo["undirected_ok"], "an undirected edge is not in exactly two triangles"
    assert topo["directed_ok"], "a directed edge is in more than one triangle: the orientation is not consistent"
    assert topo["euler"] == 2 and np.unique(faces).size == len(vertices)
    assert vol > 0
    assert dev <= 2 * dev_ref


@functools.lru_cache(maxsize=None)
def sphere_reference(half=False):
    grid, tsdf, weight, color = TR.analytic_sphere()
    if half:
        weight = weight.copy()
        weight[:, :, grid.dims[0] // 2:] = 0.0
    return grid, tsdf, weight, color, TR.surface_nets_ref(grid, tsdf, weight, color)


def volume_of(grid, tsdf, weight, color, device="cpu", dtype=F32):
    vol = make_volume(grid, device, dtype)
    for dst, src in ((vol.tsdf, tsdf), (vol.weight, weight), (vol.color, color)):
        src = np.asarray(src)
        dst.copy_(torch.as_tensor(src if src.flags.writeable else src.copy()).reshape(dst.shape))      # (a shared fixture is read-only)
    return vol


@functools.lru_cache(maxsize=None)
def three_round_reference(min_weight=1.0):
    """surface_nets_ref of TR.three_round_volume() at one min_weight plus `vertex_owners`, the voxel index of every vertex's cell:
    computed once and shared, here and in tests/test_gpu_tsdf.py; the arrays are read-only."""
    grid, tsdf, weight, color = TR.three_round_volume()
    ref = TR.surface_nets_ref(grid, tsdf, weight, color, min_weight)
    nx, ny, _ = grid.dims
    ref["vertex_owners"] = (ref["cells"][:, 2] * ny + ref["cells"][:, 1]) * nx + ref["cells"][:, 0]
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


def three_round_conditions(min_weight, what):
    """What the issue asks of the fixture, asserted wherever it is used: three rounds of the voxel scan, voxels of every round own at
    least 1 000 vertices and 1 000 quads, the first blocks of rounds 1 and 2 have non-zero prefixes.  -> (grid, ref)"""
    grid, ref = TR.three_round_volume()[0], three_round_reference(min_weight)
    assert grid.n > 2 * TR.SCAN_ROUND and grid.dims[0] % 64 != 0
    assert np.array_equal(np.sort(ref["vertex_owners"]), ref["vertex_owners"]) and np.array_equal(np.sort(ref["quad_owners"]), ref["quad_owners"])
    assert 2 * len(ref["quad_owners"]) == len(ref["faces"]) and len(ref["vertex_owners"]) == ref["vertices"].v.shape[0]
    TR.assert_rounds(ref["vertex_owners"], grid.n, f"{what} min_weight {min_weight}: vertices")
    TR.assert_rounds(ref["quad_owners"], grid.n, f"{what} min_weight {min_weight}: quads")
    return grid, ref


def test_surface_nets_on_an_analytic_sphere(host):
    grid, tsdf, weight, color, ref = sphere_reference()
    assert np.abs(ref["replay"]["vertices"].numpy() - ref["vertices"].v.numpy()).max() <= 1e-12          # the two forms of the reference
    assert np.abs(ref["replay"]["colors"].numpy() - ref["colors"].v.numpy()).max() <= 1e-12
    sphere_checks(grid, ref["vertices"].v.numpy(), ref["faces"], ref["vertices"].v.numpy(), "reference")
    for name, got in (("host", host.mesh(grid, tsdf, weight, color)), ("twin fp32", volume_of(grid, tsdf, weight, color).extract_mesh()),
                      ("twin fp64", volume_of(grid, tsdf, weight, color, dtype=F64).extract_mesh())):
        check_mesh(got, ref, name + " sphere")
        v, f, c = (np.asarray(a) for a in got)
        sphere_checks(grid, v, f, ref["vertices"].v.numpy(), name)
        assert got[1].dtype in (torch.int32, np.int32)
        assert float(c.min()) >= 0 and float(c.max()) <= 1


def test_a_volume_with_an_unobserved_half_gives_no_face_on_an_unobserved_corner(host):
    grid, tsdf, weight, color, ref = sphere_reference(half=True)
    full = sphere_reference()[4]
    assert 0 < ref["faces"].shape[0] < full["faces"].shape[0]
    obs = weight >= 1
    for name, got in (("host", host.mesh(grid, tsdf, weight, color)), ("twin", volume_of(grid, tsdf, weight, color).extract_mesh())):
        check_mesh(got, ref, name + " half")
        used = ref["cells"][np.unique(np.asarray(got[1]))]                       # the cells the faces reference, by their lowest corners
        for dx, dy, dz in TR.CORNER:
            assert obs[used[:, 2] + dz, used[:, 1] + dy, used[:, 0] + dx].all(), f"{name}: a face references a cell with an unobserved corner"
    assert not TR.mesh_topology(ref["faces"])["undirected_ok"]                   # an open surface: the check can tell


@pytest.mark.parametrize("grid_name", ["17x9x21", "64x64x64"])
def test_surface_nets_twin_and_host_on_a_fused_volume(host, grid_name):
    grid, frames, _ = fusion_reference(grid_name, 96, 96)
    vol = integrate_frames(make_volume(grid), frames)
    tsdf, weight, color = (t.numpy() for t in (vol.tsdf, vol.weight, vol.color))
    ref = TR.surface_nets_ref(grid, tsdf, weight, color)
    assert ref["faces"].shape[0] > 0 and (weight < 1).any()
    check_mesh(host.mesh(grid, tsdf, weight, color), ref, f"host {grid_name}")
    check_mesh(vol.extract_mesh(), ref, f"twin {grid_name}")
    ref2 = TR.surface_nets_ref(grid, tsdf, weight, color, min_weight=2.0)        # another cut of the same volume
    assert 0 < ref2["vertices"].v.shape[0] < ref["vertices"].v.shape[0]
    check_mesh(host.mesh(grid, tsdf, weight, color, 2.0), ref2, f"host {grid_name} min_weight 2")
    check_mesh(vol.extract_mesh(min_weight=2.0), ref2, f"twin {grid_name} min_weight 2")


def test_degenerate_volumes_give_an_empty_mesh(host):
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)):
        grid = TR.Grid(dims, (0, 0, 0), 0.1, 0.3)
        tsdf = np.linspace(-1, 1, grid.n, dtype=np.float32)
        for got in (host.mesh(grid, tsdf, np.ones(grid.n, np.float32), np.zeros(3 * grid.n, np.float32)),
                    volume_of(grid, tsdf, np.ones(grid.n, np.float32), np.zeros(3 * grid.n, np.float32)).extract_mesh()):
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0, 3)
    grid = TR.Grid((6, 5, 4), (0, 0, 0), 0.1, 0.3)                               # no active cell: one sign, and unobserved voxels
    for tsdf, weight in ((np.full(grid.n, 0.5, np.float32), np.ones(grid.n, np.float32)), (np.linspace(-1, 1, grid.n, dtype=np.float32), np.zeros(grid.n, np.float32))):
        assert TR.surface_nets_ref(grid, tsdf, weight, np.zeros(3 * grid.n))["faces"].shape == (0, 3)
        for got in (host.mesh(grid, tsdf, weight, np.zeros(3 * grid.n, np.float32)), volume_of(grid, tsdf, weight, np.zeros(3 * grid.n, np.float32)).extract_mesh()):
            assert got[0].shape == (0, 3) and got[1].shape == (0, 3)
    grid = TR.Grid((2, 2, 2), (0.5, -0.5, 1.0), 0.25, 0.5)                       # one cell: one vertex, no face
    tsdf = np.array([-0.5, 0.25, 0.5, 0.75, 0.5, 1.0, 1.0, 1.0], np.float32)
    color = np.linspace(0, 1, 24, dtype=np.float32)
    ref = TR.surface_nets_ref(grid, tsdf, np.ones(8, np.float32), color)
    assert ref["vertices"].v.shape == (1, 3) and ref["faces"].shape == (0, 3)
    check_mesh(host.mesh(grid, tsdf, np.ones(8, np.float32), color), ref, "host 2x2x2")
    check_mesh(volume_of(grid, tsdf, np.ones(8, np.float32), color).extract_mesh(), ref, "twin 2x2x2")


# ---- past the first round of k_sn_scan ----------------------------------------------------------------------------------------
def test_the_three_round_fixture_holds_what_it_is_for():
    import mesh_ref as MR
    grid, tsdf, weight, color = TR.three_round_volume()
    refs = {mw: three_round_conditions(mw, "reference")[1] for mw in (1.0, 2.0)}
    assert 4_194_304 < grid.n < 5_500_000
    assert sorted(np.unique(weight).tolist()) == [0.0, 1.0, 2.0]
    v1, v2 = refs[1.0]["vertices"].v.shape[0], refs[2.0]["vertices"].v.shape[0]
    assert 0 < v2 < v1 and 0 < len(refs[2.0]["faces"]) < len(refs[1.0]["faces"])              # the two cuts give different meshes
    # the hole cuts the surface: a volume observed everywhere has more faces, and no face names a cell with an unobserved corner
    full = TR.surface_nets_ref(grid, tsdf, np.ones_like(weight), color)
    assert len(full["faces"]) > len(refs[1.0]["faces"])
    used = refs[1.0]["cells"][np.unique(refs[1.0]["faces"])]
    for dx, dy, dz in TR.CORNER:
        assert (weight[used[:, 2] + dz, used[:, 1] + dy, used[:, 0] + dx] >= 1).all()
    # two disjoint surfaces, the plane in one piece around its hole and the larger; without the small one only the plane is left
    faces = refs[1.0]["faces"]
    labels, sizes = MR.components_ref(faces, v1)
    pieces = sorted(sizes[sizes > 0].tolist())
    alone = TR.surface_nets_ref(*TR.three_round_volume(small=False))
    print(f"min_weight 1: V = {v1}, F = {len(faces)} in components of {pieces} faces; min_weight 2: V = {v2}, F = {len(refs[2.0]['faces'])}; "
          f"observed everywhere F = {len(full['faces'])}; the plane alone F = {len(alone['faces'])}")
    assert len(pieces) == 2 and pieces[0] < pieces[1] == len(alone["faces"])
    assert TR.mesh_topology(faces[labels == np.argmax(sizes == pieces[0])])["undirected_ok"], "the small surface is not closed"


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
def test_the_three_round_fixture_tells_the_carry_rules_apart(min_weight):
    """numpy on the reference's owners, no kernel: a scan that drops the carry between rounds, or keeps only the last round's total,
    gives other prefixes than the right one in rounds 1 and 2, or in round 2, for the vertices and for the quads."""
    grid, ref = three_round_conditions(min_weight, "reference")
    for name in ("vertex_owners", "quad_owners"):
        TR.assert_rules_differ(TR.block_counts(ref[name], grid.n), f"min_weight {min_weight} {name}")


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
def test_the_twin_on_the_three_round_fixture(min_weight):
    """The float32 torch twin takes a fraction of the reference's time on this volume (measured: 0.1 s against 2.5 s), so it is held to
    the reference here too."""
    grid, tsdf, weight, color = TR.three_round_volume()
    check_mesh(volume_of(grid, tsdf, weight, color).extract_mesh(min_weight=min_weight, native=False), three_round_reference(min_weight),
               f"twin three rounds min_weight {min_weight}")


# ---- PLY ----------------------------------------------------------------------------------------------------------------------
def test_ply_round_trip(tmp_path):
    from scene.mesh import load_mesh_ply, save_mesh_ply
    grid, tsdf, weight, color, ref = sphere_reference()
    v, f = ref["vertices"].v.numpy().astype(np.float32), ref["faces"].astype(np.int32)
    c = ref["colors"].v.numpy().astype(np.float32)
    c[0], c[1] = (-0.5, 1.5, 0.5), (0.0, 1.0, 0.25)                              # outside [0,1]: clamped
    path = str(tmp_path / "out" / "mesh.ply")
    save_mesh_ply(path, torch.as_tensor(v), torch.as_tensor(f), torch.as_tensor(c))
    v2, f2, c2 = load_mesh_ply(path)
    assert v2.dtype == np.float32 and np.array_equal(v2.view(np.int32), v.view(np.int32))
    assert f2.dtype == np.int32 and np.array_equal(f2, f)
    assert c2.dtype == np.uint8 and np.array_equal(c2, np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    assert c2[0].tolist() == [0, 255, 128] and c2[1].tolist() == [0, 255, 64]
    head = open(path, "rb").read(400).split(b"end_header\n")[0].decode()
    assert head.startswith("ply\nformat binary_little_endian 1.0\n") and f"element vertex {len(v)}" in head and f"element face {len(f)}" in head
    assert os.path.getsize(path) == len(head) + len("end_header\n") + 15 * len(v) + 13 * len(f)
    save_mesh_ply(path, np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)))    # an empty mesh is a file too
    assert all(a.shape == (0, 3) for a in load_mesh_ply(path))
    with pytest.raises(ValueError, match="does not exist"):
        save_mesh_ply(path, v, f + len(v), c)
