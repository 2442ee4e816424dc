"""CPU checks of the sparse TSDF volume (diff_gaussian_rasterization/tsdf.py SparseTSDFVolume, csrc/gsr_tsdf.hip, csrc/gsr_tsdf_sparse_math.h,
scene/mesh.py): the C ABI is additive (eight new symbols in include/gsrast_tsdf_sparse.h, which gsrast.h includes;
the version unchanged, gsrast_tsdf.h's four prototypes untouched), its ctypes table agrees with the header's prototypes, and every
refusal comes without touching a GPU; the marking rule - the kernels' own text (tests/tsdf_sparse_host.cpp, compiled by g++ under
AddressSanitizer and UBSan and run as a subprocess) and the torch twins in binary32 and binary64 - lies between the binary64
restatement's marks at pad - 0.25 and pad + 0.25 and covers every brick the dense rule needs, on every fixture, and leaves bricks
unmarked; the two-pass twin holds the dense twin's bits in every allocated brick and gives its mesh; the streaming twin holds, per
brick, exactly the frames from its allocation on; the degenerate cases.  Every test prints the figures it judged."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import tsdf_ref as TR
import tsdf_sparse_ref as SR
from test_abi import header_prototypes, signature_mismatches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_tsdf_sparse_allocate", "gsr_tsdf_sparse_commit_workspace_size", "gsr_tsdf_sparse_commit_count", "gsr_tsdf_sparse_commit_assign",
                 "gsr_tsdf_sparse_integrate", "gsr_tsdf_sparse_mesh_workspace_size", "gsr_tsdf_sparse_mesh_count", "gsr_tsdf_sparse_mesh_emit")
F64, F32 = torch.float64, torch.float32
FIXTURES = sorted(SR.fixtures())


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def sparse_volume(grid, device="cpu", dtype=F32, **kw):
    from diff_gaussian_rasterization.tsdf import SparseTSDFVolume
    return SparseTSDFVolume(grid.origin, float(grid.voxel), grid.dims, float(grid.trunc), device=device, dtype=dtype, **kw)


def dense_volume(grid, device="cpu", dtype=F32):
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    return TSDFVolume(grid.origin, float(grid.voxel), grid.dims, float(grid.trunc), device=device, dtype=dtype)


def frame_args(vol, fr, color=True):
    t = lambda a: torch.as_tensor(a, dtype=vol.tsdf.dtype, device=vol.tsdf.device).contiguous()
    maps = (t(fr.depth)[None], t(fr.alpha)[None]) + ((t(fr.color),) if color else ())
    return maps + (t(fr.V), fr.tanfovx, fr.tanfovy), dict(alpha_min=fr.alpha_min, depth_max=fr.depth_max)


def allocate(vol, fr, **kw):
    a, k = frame_args(vol, fr, color=False)
    vol.allocate(*a, **k, **kw)


def integrate(vol, fr, **kw):
    a, k = frame_args(vol, fr)
    vol.integrate(*a, **k, **kw)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int64)


def allocated_voxels(vol):
    """bool [nz,ny,nx]: the voxels of the grid that lie in an allocated brick."""
    nx, ny, nz = vol.dims
    return (vol.brick_table >= 0).repeat_interleave(8, 0).repeat_interleave(8, 1).repeat_interleave(8, 2)[:nz, :ny, :nx]


def canonical(mesh, dims):
    """(vertices, faces, colors, cells) -> the same mesh with its vertices in ascending dense cell index and its faces as a sorted
    array of rows: what does not depend on the order of emission."""
    v, f, c, cells = (a.detach().cpu() for a in mesh)
    nx, ny, _ = dims
    key = (cells[:, 2].long() * ny + cells[:, 1].long()) * nx + cells[:, 0].long()
    order = torch.argsort(key)
    assert key.unique().numel() == key.numel(), "two vertices share a cell"
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel())
    faces = inv[f.long()] if f.numel() else f.long()
    faces = faces[np.lexsort(faces.numpy().T[::-1])] if faces.numel() else faces
    return v[order], faces, c[order], cells[order]


def assert_same_mesh(got, want, dims, what):
    g, w = canonical(got, dims), canonical(want, dims)
    print(f"{what}: {g[0].shape[0]} vertices, {g[1].shape[0]} faces (the dense volume's: {w[0].shape[0]}, {w[1].shape[0]})")
    assert torch.equal(g[3], w[3]), f"{what}: the cells differ"
    assert torch.equal(bits(g[0]), bits(w[0])) and torch.equal(bits(g[2]), bits(w[2])), f"{what}: a vertex or a colour differs in a bit"
    assert torch.equal(g[1], w[1]), f"{what}: the faces differ as a set of rows"


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def _header(name):
    with open(os.path.join(ROOT, "include", name)) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def test_functions_are_declared_and_exported_and_the_version_stays(native):
    main = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert main.count('#include "gsrast_tsdf_sparse.h"') == 1 and "#define GSR_VERSION 12" in main
    protos = header_prototypes(_header("gsrast_tsdf_sparse.h"))
    assert tuple(protos) == NEW_FUNCTIONS == tuple(native.TSDF_SPARSE_SIGNATURES)
    bad = signature_mismatches(protos, native.TSDF_SPARSE_SIGNATURES, native.MIRRORS)
    assert not bad, "\n".join(bad)
    assert len(header_prototypes(_header("gsrast_tsdf.h"))) == 4 == len(native.TSDF_SIGNATURES)
    lib = native.load()
    for name, (restype, argtypes) in native.TSDF_SPARSE_SIGNATURES.items():
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert getattr(lib, name).restype is restype and tuple(getattr(lib, name).argtypes) == tuple(argtypes), name
        assert native._ALL_SIGNATURES[name] == (restype, argtypes)
        assert not any(name in t for t in (native.SIGNATURES, native.TSDF_SIGNATURES, native.MESH_SIGNATURES))
    assert lib.gsr_version() == 12
    assert "typedef" not in _header("gsrast_tsdf_sparse.h")
    mk = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "Makefile")).read()
    assert "gsr_tsdf_sparse_math.h" in mk and "gsrast_tsdf_sparse.h" in mk


def test_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "gsrast.h"\nint main(void) { size_t b; return gsr_tsdf_sparse_mesh_workspace_size(0, &b) != 0 ? 0 : 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "t.o")])
    alone = tmp_path / "a.c"
    alone.write_text('#include "gsrast_tsdf_sparse.h"\nint main(void) { return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(alone), "-o", str(tmp_path / "a.o")])


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    p, odd = C.c_void_p(256), C.c_void_p(258)
    inf, nan = float("inf"), float("nan")

    def alloc(nx=40, ny=33, nz=37, vs=0.1, tr=0.3, pad=1.5, H=8, W=9, tx=0.5, ty=0.5, am=0.5, dm=inf, Vi=p, d=p, a=p, m=p, ox=0.0):
        return lib.gsr_tsdf_sparse_allocate(nx, ny, nz, ox, 0.0, 0.0, vs, tr, pad, H, W, tx, ty, am, dm, Vi, d, a, m, None), lib.gsr_last_error()

    def fuse(nx=40, ny=33, nz=37, vs=0.1, tr=0.3, H=8, W=9, tx=0.5, ty=0.5, am=0.5, dm=inf, B=3, V=p, d=p, a=p, c=p, bc=p, t=p, w=p, vc=p, ox=0.0):
        return lib.gsr_tsdf_sparse_integrate(nx, ny, nz, ox, 0.0, 0.0, vs, tr, H, W, tx, ty, am, dm, B, V, d, a, c, bc, t, w, vc, None), lib.gsr_last_error()

    common = (dict(nx=0), dict(nz=-1), dict(nx=32769), dict(vs=0.0), dict(vs=inf), dict(tr=0.0), dict(tr=nan), dict(H=-1), dict(W=40000), dict(tx=0.0),
              dict(ty=inf), dict(am=0.0), dict(am=nan), dict(dm=0.0), dict(dm=nan), dict(ox=nan))
    for call, extra in ((alloc, (dict(pad=1.0), dict(pad=1.2), dict(pad=nan), dict(pad=inf))), (fuse, (dict(B=-1), dict(B=2 ** 22)))):
        for kw in common + extra:
            rc, msg = call(**kw)
            assert rc == -1 and b"gsr_tsdf_sparse_" in msg, (call.__name__, kw)
    for call, names in ((alloc, (("Vi", b"viewmatrix_inverse"), ("d", b"depth"), ("a", b"alpha"), ("m", b"marks"))),
                        (fuse, (("V", b"viewmatrix"), ("d", b"depth"), ("a", b"alpha"), ("c", b"color"), ("bc", b"brick_coords"), ("t", b"tsdf"),
                                ("w", b"weight"), ("vc", b"vol_color")))):
        for name, shown in names:
            rc, msg = call(**{name: None})
            assert rc == -1 and shown in msg and b"NULL" in msg
            rc, msg = call(**{name: odd})
            assert rc == -1 and shown in msg and b"aligned" in msg
    assert alloc(H=0, d=None, a=None)[0] == 0 and fuse(W=0, d=None, a=None, c=None)[0] == 0     # an image without pixels: nothing is read
    assert fuse(B=0, t=None, w=None, vc=None, bc=None)[0] == 0                                   # no brick: nothing is read
    assert alloc(nx=32768, ny=32768, nz=8, H=0)[0] == 0                                          # 2^24 bricks, 2^33 voxels: inside the limits
    assert alloc(nx=32768, ny=32768, nz=32768, H=0)[0] == -1                                     # a brick table of 2^36 entries

    b = C.c_size_t(7)
    assert lib.gsr_tsdf_sparse_commit_workspace_size(1024, 1024, 1024, b) == 0
    blocks = 128 ** 3 // 256
    assert 16 * blocks <= b.value <= 16 * blocks + 3 * 256                                       # a count and a prefix per 256 table entries
    assert lib.gsr_tsdf_sparse_commit_workspace_size(0, 8, 8, b) == -1 and lib.gsr_tsdf_sparse_commit_workspace_size(8, 8, 8, None) == -1
    assert lib.gsr_tsdf_sparse_mesh_workspace_size(0, b) == 0 and b.value == 0
    assert lib.gsr_tsdf_sparse_mesh_workspace_size(1000, b) == 0 and 48 * 2000 <= b.value <= 48 * 2000 + 4 * 256    # two blocks of 256 voxels per brick
    assert lib.gsr_tsdf_sparse_mesh_workspace_size(-1, b) == -1 and lib.gsr_tsdf_sparse_mesh_workspace_size(2 ** 22, b) == -1
    assert lib.gsr_tsdf_sparse_mesh_workspace_size(2 ** 22 - 1, b) == 0 and lib.gsr_tsdf_sparse_mesh_workspace_size(4, None) == -1

    new = C.c_int64(5)

    def count(nx=40, ny=33, nz=37, m=p, t=p, ws=p, nb=1 << 20, out=new):
        return lib.gsr_tsdf_sparse_commit_count(nx, ny, nz, m, t, ws, nb, out, None), lib.gsr_last_error()

    def assign(nx=40, ny=33, nz=37, B=2, cap=8, m=p, t=p, ws=p, nb=1 << 20, bc=p, bo=p, br=p):
        return lib.gsr_tsdf_sparse_commit_assign(nx, ny, nz, B, cap, m, t, ws, nb, bc, bo, br, None), lib.gsr_last_error()

    for call in (count, assign):
        for kw, word in ((dict(nx=-1), b"voxels"), (dict(m=None), b"marks is NULL"), (dict(t=odd), b"aligned"), (dict(ws=None), b"workspace is NULL"),
                         (dict(ws=C.c_void_p(128)), b"256-byte")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, msg)
        rc, msg = call(nb=8)
        assert rc == native.ERR_WORKSPACE and b"workspace_bytes" in msg
    assert count(out=None)[0] == -1
    for kw in (dict(B=-1), dict(B=9), dict(cap=2 ** 22), dict(bc=None), dict(bo=odd), dict(br=None)):
        assert assign(**kw)[0] == -1, kw

    nv, nf = C.c_int64(5), C.c_int64(5)
    bricks = dict(bt=p, bc=p, bo=p, br=p)

    def mcount(nx=40, ny=33, nz=37, B=3, mw=1.0, t=p, w=p, ws=p, nb=1 << 20, v=nv, f=nf, **k):
        k = {**bricks, **k}
        return lib.gsr_tsdf_sparse_mesh_count(nx, ny, nz, B, mw, t, w, k["bt"], k["bc"], k["bo"], k["br"], ws, nb, v, f, None), lib.gsr_last_error()

    def memit(nx=40, ny=33, nz=37, vs=0.1, B=3, mw=1.0, t=p, w=p, c=p, ws=p, nb=1 << 20, v=4, f=2, ov=p, of=p, oc=p, cells=None, **k):
        k = {**bricks, **k}
        return lib.gsr_tsdf_sparse_mesh_emit(nx, ny, nz, 0.0, 0.0, 0.0, vs, B, mw, t, w, c, k["bt"], k["bc"], k["bo"], k["br"], ws, nb, v, f, ov, of, oc,
                                             cells, None), lib.gsr_last_error()

    assert mcount(nx=1, t=None, w=None, ws=None)[0] == 0 and nv.value == 0 and nf.value == 0    # thinner than 2 voxels: nothing is read
    nv.value = nf.value = 5
    assert mcount(B=0, t=None, w=None, ws=None)[0] == 0 and nv.value == 0 and nf.value == 0     # no allocated brick: nothing is read
    for call in (mcount, memit):
        for kw, word in ((dict(nx=-1), b"voxels"), (dict(B=-2), b"num_bricks"), (dict(mw=nan), b"NaN"), (dict(t=None), b"tsdf is NULL"), (dict(w=odd), b"aligned"),
                         (dict(bt=None), b"brick_table is NULL"), (dict(bc=odd), b"brick_coords"), (dict(bo=None), b"brick_order"), (dict(br=None), b"brick_rank"),
                         (dict(ws=None), b"workspace is NULL"), (dict(ws=C.c_void_p(128)), b"256-byte")):
            rc, msg = call(**kw)
            assert rc == -1 and word in msg, (call.__name__, kw, msg)
        rc, msg = call(nb=8)
        assert rc == native.ERR_WORKSPACE and b"workspace_bytes" in msg
    assert mcount(v=None)[0] == -1
    for kw in (dict(vs=0.0), dict(v=-1), dict(f=3), dict(c=None), dict(ov=None), dict(of=None), dict(oc=odd), dict(cells=odd)):
        assert memit(**kw)[0] == -1, kw
    assert memit(v=0, f=0, t=None, w=None, c=None, ws=None, ov=None, of=None, oc=None, bt=None, bc=None, bo=None, br=None)[0] == 0


def test_python_refusals_are_value_errors_and_native_on_host_raises():
    from diff_gaussian_rasterization.tsdf import MAX_BRICKS, SparseTSDFVolume
    ok = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(12, 9, 20), sdf_trunc=0.3, device="cpu")
    for kw in (dict(dims=(32769, 8, 8)), dict(dims=(4, 0, 4)), dict(dims=(4, 4)), dict(voxel_size=0.0), dict(voxel_size=-0.1), dict(voxel_size=float("inf")),
               dict(sdf_trunc=0.0), dict(sdf_trunc=float("nan")), dict(origin=(0.0, float("nan"), 0.0)), dict(dtype=torch.float16), dict(pad=1.0),
               dict(pad=1.2), dict(pad=float("nan")), dict(pad=float("inf")), dict(capacity=MAX_BRICKS + 1), dict(capacity=-1)):
        with pytest.raises(ValueError):
            SparseTSDFVolume(**{**ok, **kw})
    with pytest.raises(ValueError, match="brick table"):                        # 4096^3 = 2^36 entries; refused before anything is allocated
        SparseTSDFVolume(**{**ok, "dims": (32768, 32768, 32768)})
    vol = SparseTSDFVolume(**ok)
    assert vol.brick_table.shape == (3, 2, 2) and vol.brick_table.dtype == torch.int32 and bool((vol.brick_table == -1).all())
    assert vol.num_bricks == 0 and vol.tsdf.shape == (0, 8, 8, 8) and vol.weight.shape == (0, 8, 8, 8) and vol.color.shape == (0, 3, 8, 8, 8)
    assert vol.brick_coords.shape == (0, 3) and vol.brick_coords.dtype == torch.int32 and vol.pad == 1.5
    d, a, c, V = torch.ones(1, 6, 7), torch.ones(1, 6, 7), torch.ones(3, 6, 7), torch.eye(4)
    for call in (lambda: vol.allocate(d, a, V, 0.5, 0.5, native=True), lambda: vol.integrate(d, a, c, V, 0.5, 0.5, native=True),
                 lambda: vol.extract_mesh(native=True)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    good = dict(depth=d, alpha=a, color=c, viewmatrix=V, tanfovx=0.5, tanfovy=0.5)
    for bad in (dict(depth=torch.ones(2, 6, 7)), dict(alpha=torch.ones(1, 6, 8)), dict(color=torch.ones(4, 6, 7)), dict(viewmatrix=torch.eye(3)),
                dict(depth=d.double()), dict(tanfovx=0.0), dict(alpha_min=0.0), dict(depth_max=0.0), dict(depth_max=float("nan")),
                dict(depth=np.ones((1, 6, 7), np.float32)), dict(depth=d.clone().requires_grad_(True)), dict(alpha=a.clone().requires_grad_(True)),
                dict(color=c.clone().requires_grad_(True)), dict(viewmatrix=V.clone().requires_grad_(True))):
        with pytest.raises(ValueError):
            vol.integrate(**{**good, **bad})
        if "color" not in bad:
            kw = {**good, **bad}
            kw.pop("color")
            with pytest.raises(ValueError):
                vol.allocate(**kw)
    assert vol.num_bricks == 0 and not bool(vol._marks.any())                   # no refused call marked or wrote anything
    with torch.no_grad():                                                       # grad mode off: a map that requires grad is a constant
        vol.allocate(d.clone().requires_grad_(True), a, V, 0.5, 0.5)
    big = SparseTSDFVolume((0.0, 0.0, 0.0), 0.01, (2048, 2048, 1024), 0.05, device="cpu")      # 2^32 voxels: a table of 2^23 entries
    assert big.brick_table.numel() == 2 ** 23
    with pytest.raises(ValueError, match="2\\^31 - 1"):
        big.to_dense()
    with pytest.raises(ValueError, match="more than 2\\^31 - 1"):
        big._make_room(MAX_BRICKS + 1)
    from scene import mesh
    cams = [types.SimpleNamespace(camera_center=torch.tensor([float(k), 0.0, 0.0])) for k in range(2)]
    with pytest.raises(ValueError, match="resolution"):
        mesh.extract_mesh(None, cams, None, None, resolution=64, voxel_size=0.1)
    with pytest.raises(ValueError, match="resolution"):
        mesh.extract_mesh(None, cams, None, None, sparse=True, resolution=0)
    from diff_gaussian_rasterization.sharded import ShardedRenderer
    with pytest.raises(ValueError, match="extract_mesh"):
        ShardedRenderer.__new__(ShardedRenderer).extract_mesh(None, [], None, None, sparse=True, resolution=64)


# ---- marking ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tsdf_sparse"))
    exe = os.path.join(d, "tsdf_sparse_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "tsdf_sparse_host.cpp")])
    fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")

    class Host:
        @staticmethod
        def marks(grid, frames, pad):
            from diff_gaussian_rasterization.tsdf import affine_inverse
            with open(fin, "wb") as fh:
                np.array(list(grid.dims) + [len(frames)], np.int32).tofile(fh)
                np.array(list(grid.origin) + [grid.voxel, grid.trunc, pad], np.float32).tofile(fh)
                for fr in frames:
                    np.array([fr.H, fr.W], np.int32).tofile(fh)
                    np.array([fr.tanfovx, fr.tanfovy, fr.alpha_min, fr.depth_max], np.float32).tofile(fh)
                    affine_inverse(torch.as_tensor(fr.V)).numpy().astype(np.float32).tofile(fh)
                    for arr in (fr.depth, fr.alpha):
                        np.ascontiguousarray(arr, np.float32).tofile(fh)
            subprocess.check_call([exe, "marks", fin, fout])
            nbx, nby, nbz = SR.brick_dims(grid.dims)
            return np.fromfile(fout, np.uint8).reshape(len(frames), nbz, nby, nbx).astype(bool)

        @staticmethod
        def index(dims):
            return subprocess.run([exe, "index"] + [str(n) for n in dims]).returncode
    return Host


def test_the_inverse_of_the_view_matrix_is_the_inverse():
    from diff_gaussian_rasterization.tsdf import affine_inverse
    for fr in TR.make_frames(8, 8):
        V = torch.as_tensor(fr.V)
        M = affine_inverse(V)
        assert M.dtype == F32 and M.is_contiguous()
        want = np.linalg.inv(fr.V.astype(np.float64))
        assert np.abs(M.numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max()
    S = torch.tensor([[2.0, 0.3, 0.0, 0.0], [0.1, 1.5, -0.2, 0.0], [0.0, 0.4, 0.7, 0.0], [0.5, -1.0, 2.0, 1.0]], dtype=F64)   # not a rotation
    assert np.abs(affine_inverse(S).numpy() - np.linalg.inv(S.numpy())).max() <= 1e-14


def test_brick_index_arithmetic_on_the_host(host):
    for dims in ((40, 33, 37), (8, 8, 8), (1, 1, 1), (9, 17, 7), (64, 1, 65)):
        assert host.index(dims) == 0, dims


@pytest.mark.parametrize("name", FIXTURES)
def test_marks_sandwich_and_superset_of_the_host_program_and_the_twins(host, name):
    grid, frames = SR.fixtures()[name]
    assert any(n % 8 for n in grid.dims)
    got = host.marks(grid, frames, SR.PAD)
    for k, fr in enumerate(frames):
        assert fr.valid.any()
        SR.check_marks(got[k], grid, fr, f"host {name} frame {k}")
        for dtype in (F32, F64):
            vol = sparse_volume(grid, dtype=dtype)
            allocate(vol, fr)
            marked = vol._marks.numpy() != 0
            SR.check_marks(marked, grid, fr, f"twin {dtype} {name} frame {k}")
            assert vol.num_bricks == int(marked.sum()) and not bool(vol._marks.any())          # the commit: a slot per mark, the marks cleared
            assert np.array_equal(vol.brick_table.numpy() >= 0, marked)


def test_the_fixtures_hold_what_they_are_for():
    fx = SR.fixtures()
    grid, (fr,) = fx["near_zero"]
    d = fr.depth[fr.valid] / fr.alpha[fr.valid]
    assert (d - grid.trunc < 0).any(), "no pixel with d - sdf_trunc < 0"
    grid, (fr,) = fx["wide_pixels"]
    d = float(np.median(fr.depth[fr.valid] / fr.alpha[fr.valid]))
    assert 2 * fr.tanfovx * d / fr.W > 8 * float(grid.voxel) and 2 * fr.tanfovy * d / fr.H > 8 * float(grid.voxel), "a pixel is no wider than a brick"
    grid, (fr,) = fx["silhouette"]
    d = np.where(fr.valid, fr.depth / np.where(fr.valid, fr.alpha, 1), np.nan)
    assert np.nanmax(np.abs(np.diff(d, axis=1))) > 2.0, "no neighbouring pixels metres apart"
    grid, (fr,) = fx["camera_inside"]
    c = -fr.V[3, :3].astype(np.float64) @ fr.V[:3, :3].astype(np.float64).T
    vox = (c - grid.origin) / float(grid.voxel)
    assert (vox > 0).all() and (vox < np.array(grid.dims) - 1).all(), "the camera is not inside the volume"
    grid, (fr,) = fx["plane_grazing"]
    d = fr.depth[fr.valid] / fr.alpha[fr.valid]
    assert d.max() > 5 * d.min() and fr.valid.mean() > 0.3                      # the plane runs away from the camera under its rays
    grid, (fr,) = fx["depth_max_cut"]
    assert np.isfinite(fr.depth_max) and (fr.depth[fr.valid] / fr.alpha[fr.valid] > fr.depth_max).any()


# ---- the twins ----------------------------------------------------------------------------------------------------------------
TWIN_GRID = TR.Grid((40, 33, 37), (-1.0, -0.8, -0.9), 0.05, 0.1)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_the_two_pass_twin_holds_the_dense_twins_bits_and_gives_its_mesh(dtype):
    from diff_gaussian_rasterization.tsdf import extract_mesh_torch
    frames = TR.make_frames(48, 40)
    dense, vol = dense_volume(TWIN_GRID, dtype=dtype), sparse_volume(TWIN_GRID, dtype=dtype)
    for fr in frames:
        allocate(vol, fr)
    for fr in frames:
        integrate(dense, fr)
        integrate(vol, fr)
    nb = int(np.prod(vol.brick_dims))
    print(f"{dtype}: {vol.num_bricks} of {nb} bricks allocated")
    assert 0 < vol.num_bricks < nb and vol.tsdf.shape == (vol.num_bricks, 8, 8, 8) and vol.color.shape == (vol.num_bricks, 3, 8, 8, 8)
    c = vol.brick_coords.long()
    assert torch.equal(vol.brick_table[c[:, 2], c[:, 1], c[:, 0]], torch.arange(vol.num_bricks, dtype=torch.int32))
    assert int((vol.brick_table >= 0).sum()) == vol.num_bricks
    m, back = allocated_voxels(vol), vol.to_dense()
    assert 0 < int(m.sum()) < m.numel()
    for name in ("tsdf", "weight"):
        assert torch.equal(bits(getattr(dense, name)[m]), bits(getattr(back, name)[m])), name
        assert not bool(getattr(back, name)[~m].any())
    assert torch.equal(bits(dense.color[:, m]), bits(back.color[:, m]))
    beyond = torch.ones(5 * 8, 5 * 8, 5 * 8, dtype=torch.bool)                  # the voxels of allocated bricks beyond dims stay zero
    beyond[:37, :33, :40] = False
    pool = torch.zeros(5, 8, 5, 8, 5, 8, dtype=dtype)
    pool[c[:, 2], :, c[:, 1], :, c[:, 0], :] = vol.weight + vol.tsdf.abs() + vol.color.abs().sum(1)
    assert not bool(pool.view(40, 40, 40)[beyond].any())
    want = extract_mesh_torch(dense, return_cells=True)
    got = vol.extract_mesh(return_cells=True)
    assert want[0].shape[0] > 100 and want[1].shape[0] > 100 and got[3].dtype == torch.int32 and got[1].dtype == torch.int32
    assert_same_mesh(got, want, TWIN_GRID.dims, f"two-pass twin {dtype}")
    from diff_gaussian_rasterization.tsdf import brick_order_key
    key = brick_order_key(got[3], TWIN_GRID.dims)
    assert bool((key[1:] > key[:-1]).all()), "the vertices are not in ascending (brick, local voxel) order"
    assert len(vol.extract_mesh()) == 3 and torch.equal(vol.extract_mesh()[1], got[1])
    got2 = vol.extract_mesh(min_weight=2.0, return_cells=True)                  # another cut of the same volume
    dense2 = extract_mesh_torch(dense, 2.0, return_cells=True)
    assert 0 < got2[0].shape[0] < got[0].shape[0] and torch.equal(canonical(got2, TWIN_GRID.dims)[3], canonical(dense2, TWIN_GRID.dims)[3])


def test_the_streaming_twin_holds_the_frames_from_a_bricks_allocation_on():
    frames = SR.streaming_frames()
    vol = sparse_volume(TWIN_GRID)
    first = []                                                                  # per frame: the slots it allocated
    for fr in frames:
        before = vol.num_bricks
        allocate(vol, fr)
        integrate(vol, fr)
        first.append((before, vol.num_bricks))
    print("slots allocated per frame:", first)
    assert all(b > a for a, b in first), "a frame allocated nothing: the rule is not exercised"
    for k, (a, b) in enumerate(first):
        dense = dense_volume(TWIN_GRID)
        for fr in frames[k:]:
            integrate(dense, fr)
        c = vol.brick_coords[a:b].long()
        for name in ("tsdf", "weight"):
            padded = torch.zeros(5, 8, 5, 8, 5, 8)
            padded.view(40, 40, 40)[:37, :33, :40] = getattr(dense, name)
            assert torch.equal(bits(padded[c[:, 2], :, c[:, 1], :, c[:, 0], :]), bits(getattr(vol, name)[a:b])), (k, name)
    full = dense_volume(TWIN_GRID)
    for fr in frames:
        integrate(full, fr)
    a, b = first[1]                                                             # and the first frame's carving is lost in the second's bricks
    c = vol.brick_coords[a:b].long()
    padded = torch.zeros(5, 8, 5, 8, 5, 8)
    padded.view(40, 40, 40)[:37, :33, :40] = full.weight
    assert not torch.equal(padded[c[:, 2], :, c[:, 1], :, c[:, 0], :], vol.weight[a:b])


def test_allocation_order_changes_the_slots_and_nothing_else():
    frames = TR.make_frames(48, 40)
    vols = []
    for order in ((0, 1, 2), (2, 1, 0)):
        vol = sparse_volume(TWIN_GRID, capacity=4)
        for k in order:
            allocate(vol, frames[k])
            vol.commit()
        for fr in frames:
            integrate(vol, fr)
        vols.append(vol)
    a, b = vols
    assert a.growths >= 2 and a.capacity >= a.num_bricks == b.num_bricks
    assert not torch.equal(a.brick_table, b.brick_table) and torch.equal(a.brick_table >= 0, b.brick_table >= 0)
    da, db = a.to_dense(), b.to_dense()
    assert all(torch.equal(bits(getattr(da, n)), bits(getattr(db, n))) for n in ("tsdf", "weight", "color"))
    ma, mb = a.extract_mesh(return_cells=True), b.extract_mesh(return_cells=True)
    assert ma[0].shape[0] > 0 and all(torch.equal(x, y) for x, y in zip(ma, mb))               # not canonicalised: the order itself


# ---- degenerate cases ---------------------------------------------------------------------------------------------------------
def test_degenerate_volumes_and_frames():
    frames = TR.make_frames(48, 40)
    for dims in ((1, 33, 37), (40, 1, 37), (40, 33, 1)):                        # thinner than 2 voxels: an empty mesh
        grid = TR.Grid(dims, [-0.02 if n == 1 else o for n, o in zip(dims, (-1.0, -0.8, -0.9))], 0.05, 0.1)     # the slab cuts the sphere
        vol = sparse_volume(grid)
        for fr in frames:
            allocate(vol, fr)
            integrate(vol, fr)
        got = vol.extract_mesh(return_cells=True)
        assert vol.num_bricks > 0 and [tuple(t.shape) for t in got] == [(0, 3)] * 4
    vol = sparse_volume(TWIN_GRID)                                              # no allocated brick: an empty mesh, and integrate writes nothing
    integrate(vol, frames[0])
    got = vol.extract_mesh(return_cells=True)
    assert vol.num_bricks == 0 and [tuple(t.shape) for t in got] == [(0, 3)] * 4 and got[1].dtype == torch.int32
    assert vol.commit() == 0                                                    # nothing pending: nothing happens
    for fr in frames[:2]:
        allocate(vol, fr)
    new = vol.commit()
    assert new == vol.num_bricks > 0
    for fr in frames[:2]:
        integrate(vol, fr)
    table, coords = vol.brick_table.clone(), vol.brick_coords.clone()
    state = [bits(t).clone() for t in (vol.tsdf, vol.weight, vol.color)]
    assert vol.commit() == 0 and torch.equal(vol.brick_table, table) and torch.equal(vol.brick_coords, coords)
    allocate(vol, frames[0])                                                    # bricks that exist already: no new slot, no reordering
    assert vol.commit() == 0 and torch.equal(vol.brick_table, table) and torch.equal(vol.brick_coords, coords)
    blind = TR.sphere_frame(TR.look_at((4.0, 0.0, 0.0), (8.0, 0.0, 0.0)), 48, 40)       # looks away from everything: alpha 0 everywhere
    assert not blind.valid.any()
    allocate(vol, blind)
    integrate(vol, blind)
    nothing = TR.Frame(frames[0].V, np.zeros((0, 40), np.float32), np.zeros((0, 40), np.float32), np.zeros((3, 0, 40), np.float32), 0.7, 0.55)
    allocate(vol, nothing)
    integrate(vol, nothing)
    assert torch.equal(vol.brick_table, table) and all(torch.equal(bits(t), s) for t, s in zip((vol.tsdf, vol.weight, vol.color), state))
