"""Fixtures and the binary64 restatement of the sparse TSDF volume's marking rule (diff_gaussian_rasterization/tsdf.py SparseTSDFVolume,
csrc/gsr_tsdf_sparse_math.h), shared by tests/test_tsdf_sparse_ref.py and tests/test_gpu_tsdf_sparse.py.

`marks_ref` restates the rule in an independent form: the full 4 x 4 inverse of the view matrix by numpy, homogeneous corner points,
the bricks of a pixel as slices of a boolean array.  `needed_bricks` is what the marks are for, computed from the dense fusion rule of
tests/tsdf_ref.py: the bricks that hold a voxel within Chebyshev distance 1 of a voxel that receives a sample |s| < sdf_trunc from the
frame.  Nothing here comes from what the code under test gives.

The sandwich.  The code under test evaluates the box in binary32 (or, the float64 twin, in another order of operations), so its marks
at `pad` need not equal the restatement's at `pad`; but a coordinate of a few hundred voxels carries a rounding far below a quarter
voxel (2^-24 x 1000 voxels x a handful of operations < 0.001), so they lie between the restatement's marks at pad - 0.25 and at
pad + 0.25.  The superset property is asserted for the restatement at pad - 0.25, and so holds for everything above it.
"""
import functools

import numpy as np

import tsdf_ref as TR

PAD = 1.5
SLACK = 0.25


def brick_dims(dims):
    return tuple((n + 7) // 8 for n in dims)


def plane_frame(V, W, H, normal, offset, tanfov=TR.TANFOV, depth_max=np.inf, alpha=0.9):
    """The maps of a camera that sees the plane normal . p = offset (alpha 0 where the ray misses it or meets it behind the camera)."""
    V64 = np.asarray(V, np.float64)
    R, c = V64[:3, :3], -V64[3, :3] @ V64[:3, :3].T
    fx, fy = W / (2.0 * tanfov[0]), H / (2.0 * tanfov[1])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dw = np.stack([(x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, np.ones_like(x)], -1) @ R.T
    n = np.asarray(normal, np.float64)
    den = dw @ n
    lam = np.where(np.abs(den) > 1e-9, (offset - c @ n) / np.where(np.abs(den) > 1e-9, den, 1.0), -1.0)
    hit = lam > 0
    a = np.where(hit, alpha, 0.0).astype(np.float32)
    depth = (np.where(hit, lam, 0.0).astype(np.float32) * a).astype(np.float32)
    color = np.stack([a * 0.3, a * 0.6, a * 0.9]).astype(np.float32)
    return TR.Frame(V, depth, a, color, tanfov[0], tanfov[1], 0.5, depth_max)


def silhouette_frame(V, W, H):
    """A sphere of radius 0.5 around (-0.5, 0, 0) in front of the plane x = 2.5: neighbouring pixels at its rim are metres apart."""
    back = plane_frame(V, W, H, (1.0, 0.0, 0.0), 2.5)
    V64 = np.asarray(V, np.float64)
    shift = np.eye(4)
    shift[3, :3] = (-0.5, 0.0, 0.0)                                             # the sphere's frame: the world moved by its centre
    front = TR.sphere_frame((shift @ V64).astype(np.float32), W, H, radius=0.5, holes=False)
    use = front.alpha > 0
    return TR.Frame(V, np.where(use, front.depth, back.depth), np.where(use, front.alpha, back.alpha),
                    np.where(use[None], front.color, back.color), TR.TANFOV[0], TR.TANFOV[1], 0.5, np.inf)


@functools.lru_cache(maxsize=None)
def fixtures():
    """name -> (grid, [frames]): what the issue lists.  Every grid has a dimension that is no multiple of 8."""
    out = {}
    three = TR.make_frames(48, 40)
    # a sphere seen from outside (and the two other posed cameras of tests/tsdf_ref.py: one inside the volume, one cut by depth_max)
    out["sphere_outside"] = (TR.Grid((40, 33, 37), (-1.0, -0.8, -0.9), 0.05, 0.1), [three[0]])
    out["camera_inside"] = (TR.Grid((40, 33, 37), (-1.0, -0.8, -0.9), 0.05, 0.1), [three[1]])
    out["depth_max_cut"] = (TR.Grid((40, 33, 37), (-1.0, -0.8, -0.9), 0.05, 0.1), [three[2]])
    # the plane z = 0 from a camera 0.15 above it: rays meet it at a few degrees
    out["plane_grazing"] = (TR.Grid((50, 27, 13), (-1.0, -0.65, -0.3), 0.05, 0.1),
                            [plane_frame(TR.look_at((-1.5, 0.05, 0.15), (0.6, 0.0, 0.0), roll=0.1), 40, 30, (0.0, 0.0, 1.0), 0.0)])
    out["silhouette"] = (TR.Grid((63, 41, 39), (-3.0, -2.0, -1.9), 0.1, 0.2), [silhouette_frame(TR.look_at((-2.6, 0.1, 0.05), (0.5, 0.0, 0.0)), 36, 28)])
    # 6 x 5 pixels on a grid of 2 cm voxels: a pixel's footprint at the sphere is 0.35 m, a brick 0.16 m
    out["wide_pixels"] = (TR.Grid((61, 59, 60), (-0.13, -0.9, -0.38), 0.02, 0.06), [TR.sphere_frame(three[0].V, 6, 5, holes=False)])
    # a camera inside the sphere 0.1 from its wall, sdf_trunc 0.15: d - sdf_trunc < 0
    out["near_zero"] = (TR.Grid((30, 29, 31), (-0.1, -0.75, -0.75), 0.05, 0.15),
                        [TR.sphere_frame(TR.look_at((0.5, 0.0, 0.0), (1.0, 0.02, 0.01)), 24, 20, holes=False)])
    return out


def streaming_frames(W=48, H=40):
    """Three frames for which streaming and two passes differ: one camera sees a sphere of radius 0.3, then the same camera one of 0.6
    (its near side lies in the free space the first frame carved, in bricks the first frame did not allocate), then the camera inside
    of tests/tsdf_ref.py.  No one scene shows all three; the rule under test is arithmetic."""
    V = TR.look_at((1.9, -1.2, 0.9), (0.05, 0.0, -0.1), roll=0.35)
    return [TR.sphere_frame(V, W, H, radius=0.3, seed=5), TR.sphere_frame(V, W, H, seed=6), TR.make_frames(W, H)[1]]


def marks_ref(grid, fr, pad):
    """The marking rule in binary64 -> bool [nbz,nby,nbx]."""
    nx, ny, nz = grid.dims
    nbx, nby, nbz = brick_dims(grid.dims)
    marks = np.zeros((nbz, nby, nbx), bool)
    Minv = np.linalg.inv(fr.V.astype(np.float64))
    fx, fy = fr.W / (2.0 * fr.tanfovx), fr.H / (2.0 * fr.tanfovy)
    trunc, voxel, origin = float(grid.trunc), float(grid.voxel), grid.origin.astype(np.float64)
    for py, px in zip(*np.nonzero(fr.valid)):
        d = float(fr.depth[py, px]) / float(fr.alpha[py, px])
        if d > fr.depth_max:
            continue
        pts = []
        for z in (max(d - trunc, 0.0), d + trunc):
            for cy in (py, py + 1):
                for cx in (px, px + 1):
                    pts.append([(cx - fr.W / 2.0) / fx * z, (cy - fr.H / 2.0) / fy * z, z, 1.0])
        vox = ((np.asarray(pts) @ Minv)[:, :3] - origin) / voxel
        first = np.maximum(np.ceil(vox.min(0) - pad), 0).astype(np.int64)
        last = np.minimum(np.floor(vox.max(0) + pad), np.array([nx, ny, nz]) - 1).astype(np.int64)
        if (first > last).any():
            continue
        marks[first[2] // 8:last[2] // 8 + 1, first[1] // 8:last[1] // 8 + 1, first[0] // 8:last[0] // 8 + 1] = True
    return marks


def near_surface(grid, fr):
    """bool [nz,ny,nx]: the voxels the dense rule gives a sample |s| < sdf_trunc from this frame (binary64, tests/tsdf_ref.py's form)."""
    ix, iy, iz = grid.coords()
    P = np.stack([grid.origin[0].astype(np.float64) + float(grid.voxel) * ix, grid.origin[1].astype(np.float64) + float(grid.voxel) * iy,
                  grid.origin[2].astype(np.float64) + float(grid.voxel) * iz, np.ones(grid.n)], 1)
    pv = P @ fr.V.astype(np.float64)
    z = pv[:, 2]
    front = z > 0
    zs = np.where(front, z, 1.0)
    u = fr.W / (2.0 * fr.tanfovx) * pv[:, 0] / zs + fr.W / 2.0
    v = fr.H / (2.0 * fr.tanfovy) * pv[:, 1] / zs + fr.H / 2.0
    seen = front & (u >= 0) & (u < fr.W) & (v >= 0) & (v < fr.H)
    px, py = np.floor(np.where(seen, u, 0)).astype(np.int64), np.floor(np.where(seen, v, 0)).astype(np.int64)
    ok = seen & fr.valid[py, px]
    d = np.where(ok, fr.depth[py, px].astype(np.float64), 1.0) / np.where(ok, fr.alpha[py, px].astype(np.float64), 1.0)
    ok &= ~(d > fr.depth_max) & (np.abs(d - z) < float(grid.trunc))
    nx, ny, nz = grid.dims
    return ok.reshape(nz, ny, nx)


def needed_bricks(grid, fr):
    """bool [nbz,nby,nbx]: the bricks that hold a voxel within Chebyshev distance 1 of a voxel of near_surface."""
    near = near_surface(grid, fr)
    nz, ny, nx = near.shape
    grown = np.zeros_like(near)
    padded = np.pad(near, 1)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                grown |= padded[dz:dz + nz, dy:dy + ny, dx:dx + nx]
    nbx, nby, nbz = brick_dims(grid.dims)
    full = np.zeros((nbz * 8, nby * 8, nbx * 8), bool)
    full[:nz, :ny, :nx] = grown
    return full.reshape(nbz, 8, nby, 8, nbx, 8).any((1, 3, 5))


def check_marks(got, grid, fr, what, pad=PAD):
    """The sandwich and the superset property for the marks `got` (bool [nbz,nby,nbx]) of one frame at `pad`; prints the counts."""
    got = np.asarray(got).astype(bool)
    inner, outer, need = marks_ref(grid, fr, pad - SLACK), marks_ref(grid, fr, pad + SLACK), needed_bricks(grid, fr)
    print(f"{what}: {int(need.sum())} bricks needed, {int(inner.sum())} / {int(got.sum())} / {int(outer.sum())} marked at pad - 0.25 / by the code "
          f"under test / at pad + 0.25, of {got.size}")
    assert got.shape == inner.shape
    assert need.any(), f"{what}: the fixture needs no brick"
    assert not (need & ~inner).any(), f"{what}: the restatement at pad - 0.25 misses a needed brick"
    assert not (inner & ~got).any(), f"{what}: a brick the restatement marks at pad - 0.25 is not marked"
    assert not (got & ~outer).any(), f"{what}: a brick is marked that the restatement does not mark at pad + 0.25"
    assert not got.all() and not outer.all(), f"{what}: every brick is marked: the fixture cannot tell the rule from 'mark everything'"
