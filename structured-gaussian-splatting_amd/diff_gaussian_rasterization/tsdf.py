"""TSDF fusion of depth maps and mesh extraction by surface nets: where the surface pipeline of 2DGS, Gaussian Opacity Fields, RaDe-GS
and PGSR ends.  Depth maps rendered from the training cameras are fused into a truncated signed distance volume, and a triangle mesh
is extracted from it (csrc/gsr_tsdf.hip; C ABI: include/gsrast_tsdf.h).

  TSDFVolume.integrate      one frame into the volume: one HIP launch, a thread per voxel, no host synchronisation
  TSDFVolume.extract_mesh   naive surface nets (the dual of marching cubes: no case table) in three HIP stages, one host readback
  SparseTSDFVolume          the same grid as bricks of 8 x 8 x 8 voxels allocated where a depth map put a surface: allocate (a thread per
                            pixel), integrate (a block per brick), extract_mesh (through the brick table); DESIGN section 30

fp32 device volumes run the kernels; host volumes, and `native=False`, take the same rules as torch ops (`integrate_torch`,
`extract_mesh_torch`, in the volume's dtype).  `native=True` on host tensors raises: there is no silent fallback.  No atomic is used:
the same frames in the same order give the same bits, and so does the same volume.

Conventions (those of normals.py): row-vector matrices (p_view = p @ V[:3,:3] + V[3,:3]); fx = W / (2 tanfovx), fy = H / (2 tanfovy);
pixel (x, y) has its centre at x + 0.5.  The volume is indexed [z, y, x]; voxel (ix, iy, iz) has its centre at
origin + voxel_size * (ix, iy, iz).

The fusion rule is KinectFusion's and Open3D's projective rule with free-space carving, restated from the literature.  Out of scope:
unbounded (contracted) volumes, hashing in place of the sparse volume's dense brick table, brick deallocation and decimation (mesh
cleaning: meshops.py; median depth: normals.surface_depth).
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .normals import _focal

MAX_VOXELS = 2 ** 31 - 1


def _refuse_grad(what: str, **maps) -> None:
    if torch.is_grad_enabled():
        for name, t in maps.items():
            if t.requires_grad:
                raise ValueError(f"{what}: {name} requires grad, and the fusion gives the maps no gradient (detach it, or fuse under "
                                 "torch.no_grad())")


def _check_frame(what, vol, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max):
    given = tuple((name, t) for name, t in (("depth", depth), ("alpha", alpha), ("color", color), ("viewmatrix", viewmatrix)) if t is not None)
    for name, t in given:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[0] != 1):
        raise ValueError(f"{what}: depth [1,H,W] or [H,W] expected, got {tuple(depth.shape)}")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if alpha.dim() not in (2, 3) or tuple(alpha.shape[-2:]) != (H, W) or alpha.numel() != H * W:
        raise ValueError(f"{what}: alpha [1,H,W] or [H,W] expected for H, W = {H}, {W}, got {tuple(alpha.shape)}")
    if color is not None and tuple(color.shape) != (3, H, W):
        raise ValueError(f"{what}: color [3,H,W] expected for H, W = {H}, {W}, got {tuple(color.shape)}")
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix [4,4] expected, got {tuple(viewmatrix.shape)}")
    for name, t in given:
        if t.dtype != vol.tsdf.dtype or t.device != vol.tsdf.device:
            raise ValueError(f"{what}: {name} is {t.dtype} on {t.device}, the volume {vol.tsdf.dtype} on {vol.tsdf.device}: one device and "
                             "one float dtype expected")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous")
    if not (tanfovx > 0 and tanfovy > 0 and alpha_min > 0 and np.isfinite([tanfovx, tanfovy, alpha_min]).all()):
        raise ValueError(f"{what}: tanfovx = {tanfovx}, tanfovy = {tanfovy}, alpha_min = {alpha_min}: positive and finite expected")
    if not depth_max > 0:
        raise ValueError(f"{what}: depth_max = {depth_max}: positive expected (inf cuts nothing)")
    _refuse_grad(what, **dict(given))
    return H, W


def integrate_torch(vol: "TSDFVolume", depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf):
    """The fusion rule as torch ops over the whole volume, in the volume's dtype.  Skipped voxels are not written."""
    H, W = _check_frame("integrate_torch", vol, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
    if H * W == 0:
        return
    dt, dev = vol.tsdf.dtype, vol.tsdf.device
    nx, ny, nz = vol.dims
    with torch.no_grad():
        V = viewmatrix
        wx = (vol.voxel_size * torch.arange(nx, dtype=dt, device=dev) + vol.origin[0]).view(1, 1, nx)
        wy = (vol.voxel_size * torch.arange(ny, dtype=dt, device=dev) + vol.origin[1]).view(1, ny, 1)
        wz = (vol.voxel_size * torch.arange(nz, dtype=dt, device=dev) + vol.origin[2]).view(nz, 1, 1)
        x, y, z = (wx * V[0, j] + (wy * V[1, j] + (wz * V[2, j] + V[3, j])) for j in range(3))
        ok = z > 0
        zs = torch.where(ok, z, torch.ones_like(z))
        u = (_focal(W, tanfovx, dt) * x) / zs + 0.5 * W
        v = (_focal(H, tanfovy, dt) * y) / zs + 0.5 * H
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        idx = ok.reshape(-1).nonzero()[:, 0]                                       # the voxels that see a pixel
        if idx.numel() == 0:
            return
        pix = torch.floor(v.reshape(-1)[idx]).long() * W + torch.floor(u.reshape(-1)[idx]).long()
        d_sum, a = depth.reshape(-1)[pix], alpha.reshape(-1)[pix]
        valid = (a >= float(np.float32(alpha_min))) & (d_sum > 0)                  # (the cut-off is a binary32 number in every dtype)
        one = torch.ones_like(a)
        d = torch.where(valid, d_sum, one) / torch.where(valid, a, one)
        s = d - z.reshape(-1)[idx]
        take = valid & ~(d > depth_max) & (s > -vol.sdf_trunc)
        idx, pix, s = idx[take], pix[take], s[take]
        t = torch.clamp(s / vol.sdf_trunc, max=1.0)
        w = vol.weight.view(-1)[idx]
        tsdf, col = vol.tsdf.view(-1), vol.color.view(3, -1)
        tsdf[idx] = (tsdf[idx] * w + t) / (w + 1)
        for c in range(3):
            col[c, idx] = (col[c, idx] * w + color[c].reshape(-1)[pix]) / (w + 1)
        vol.weight.view(-1)[idx] = w + 1


_CORNERS = tuple((k & 1, (k >> 1) & 1, k >> 2) for k in range(8))                # corner k = x + 2 y + 4 z


def extract_mesh_torch(vol: "TSDFVolume", min_weight=1.0, return_cells=False):
    """Surface nets as torch ops, in the volume's dtype -> (vertices [V,3], faces [F,3] int32, colors [V,3]); with return_cells also
    [V,3] int32, the lowest-corner voxel (ix, iy, iz) of every vertex's cell."""
    dt, dev = vol.tsdf.dtype, vol.tsdf.device
    nx, ny, nz = vol.dims
    empty = (torch.zeros(0, 3, dtype=dt, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), torch.zeros(0, 3, dtype=dt, device=dev))
    if return_cells:
        v, f, c = extract_mesh_torch(vol, min_weight)
        with torch.no_grad():                                                      # the cells again, as the vertices were ordered
            obs, inside = vol.weight >= min_weight, vol.tsdf < 0
            if v.shape[0] == 0:
                return v, f, c, torch.zeros(0, 3, dtype=torch.int32, device=dev)
            sl = lambda t, k: t[_CORNERS[k][2]:nz - 1 + _CORNERS[k][2], _CORNERS[k][1]:ny - 1 + _CORNERS[k][1], _CORNERS[k][0]:nx - 1 + _CORNERS[k][0]]
            all_obs = torch.stack([sl(obs, k) for k in range(8)]).all(0)
            ins = torch.stack([sl(inside, k) for k in range(8)])
            cz, cy, cx = (all_obs & ins.any(0) & ~ins.all(0)).nonzero(as_tuple=True)
            return v, f, c, torch.stack([cx, cy, cz], 1).to(torch.int32)
    if min(nx, ny, nz) < 2:
        return empty
    with torch.no_grad():
        tsdf, obs, inside = vol.tsdf, vol.weight >= min_weight, vol.tsdf < 0

        def corner(t, k):
            dx, dy, dz = _CORNERS[k]
            return t[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]

        all_obs, any_in, any_out = corner(obs, 0).clone(), corner(inside, 0).clone(), ~corner(inside, 0)
        for k in range(1, 8):
            all_obs &= corner(obs, k)
            any_in |= corner(inside, k)
            any_out |= ~corner(inside, k)
        active = all_obs & any_in & any_out                                        # [nz-1, ny-1, nx-1]
        cz, cy, cx = active.nonzero(as_tuple=True)                                 # ascending cell index
        nv = int(cx.numel())
        if nv == 0:
            return empty
        vid = torch.full(active.shape, -1, dtype=torch.int64, device=dev)
        vid[cz, cy, cx] = torch.arange(nv, device=dev)
        # ---- vertices: the sign-changing edges in the fixed order
        f = [tsdf[cz + dz, cy + dy, cx + dx] for dx, dy, dz in _CORNERS]
        rgb = [[vol.color[c, cz + dz, cy + dy, cx + dx] for dx, dy, dz in _CORNERS] for c in range(3)]
        acc = [torch.zeros(nv, dtype=dt, device=dev) for _ in range(3)]
        cacc = [torch.zeros(nv, dtype=dt, device=dev) for _ in range(3)]
        count = torch.zeros(nv, dtype=dt, device=dev)
        zero = torch.zeros(nv, dtype=dt, device=dev)
        for a in range(3):
            for ka in range(8):
                if ka & (1 << a):
                    continue
                kb = ka | (1 << a)
                cross = (f[ka] < 0) != (f[kb] < 0)
                den = torch.where(cross, f[ka] - f[kb], torch.ones_like(zero))
                t = f[ka] / den
                for j in range(3):
                    acc[j] = acc[j] + torch.where(cross, t if j == a else torch.full_like(zero, float(_CORNERS[ka][j])), zero)
                for c in range(3):
                    cacc[c] = cacc[c] + torch.where(cross, (rgb[c][kb] - rgb[c][ka]) * t + rgb[c][ka], zero)
                count = count + cross.to(dt)
        inv = 1.0 / count
        base = (cx.to(dt), cy.to(dt), cz.to(dt))
        vertices = torch.stack([vol.voxel_size * (acc[j] * inv + base[j]) + vol.origin[j] for j in range(3)], 1)
        colors = torch.stack([cacc[c] * inv for c in range(3)], 1)
        # ---- faces: per axis, the edges whose two voxels are observed and differ in sign and whose four cells are active
        n = (nx, ny, nz)
        keys, quads, flips = [], [], []
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            lo = [1, 1, 1]
            lo[a] = 0
            if any(n[j] - 1 - lo[j] <= 0 for j in range(3)):
                continue

            def view(t, off, cells=False):
                """t over the candidate voxels shifted by off = (dx, dy, dz)"""
                sl = tuple(slice(lo[j] + off[j], n[j] - 1 + off[j]) for j in (2, 1, 0))
                return t[sl]
            e = [0, 0, 0]
            e[a] = 1
            m = view(obs, (0, 0, 0)) & view(obs, e) & (view(inside, (0, 0, 0)) != view(inside, e))
            offs = []
            for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):
                o = [0, 0, 0]
                o[b], o[c] = ob, oc
                offs.append(o)
                m = m & view(active, o)
            qz, qy, qx = m.nonzero(as_tuple=True)
            if qx.numel() == 0:
                continue
            p = [qx + lo[0], qy + lo[1], qz + lo[2]]
            keys.append(((p[2] * ny + p[1]) * nx + p[0]) * 3 + a)
            quads.append(torch.stack([vid[p[2] + o[2], p[1] + o[1], p[0] + o[0]] for o in offs], 1))
            flips.append(~inside[p[2], p[1], p[0]])
        if not keys:
            return vertices, empty[1], colors
        order = torch.argsort(torch.cat(keys))
        q, flip = torch.cat(quads)[order], torch.cat(flips)[order]
        v0, v1, v2, v3 = q.unbind(1)
        first = torch.stack([v0, torch.where(flip, v2, v1), torch.where(flip, v1, v2)], 1)
        second = torch.stack([v0, torch.where(flip, v3, v2), torch.where(flip, v2, v3)], 1)
        faces = torch.stack([first, second], 1).reshape(-1, 3).to(torch.int32)
        return vertices, faces, colors


def _init_grid(self, who, origin, voxel_size, dims, sdf_trunc, dtype):
    """The virtual grid both volumes share: validates it and sets origin, voxel_size, sdf_trunc and dims."""
    origin = tuple(float(v) for v in (origin.tolist() if hasattr(origin, "tolist") else origin))
    dims = tuple(int(v) for v in dims)
    if len(origin) != 3 or not np.isfinite(origin).all():
        raise ValueError(f"{who}: origin = {origin}: three finite numbers expected")
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"{who}: dims = {dims}: three dimensions of at least one voxel expected")
    if not (voxel_size > 0 and math.isfinite(voxel_size)):
        raise ValueError(f"{who}: voxel_size = {voxel_size}: positive and finite expected")
    if not (sdf_trunc > 0 and math.isfinite(sdf_trunc)):
        raise ValueError(f"{who}: sdf_trunc = {sdf_trunc}: positive and finite expected")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{who}: dtype = {dtype}: float32 (the kernels') or float64 (the torch twin only)")
    f32 = dtype == torch.float32                       # a binary32 volume holds the binary32 numbers the kernels receive
    self.origin = tuple(float(np.float32(v)) for v in origin) if f32 else origin
    self.voxel_size = float(np.float32(voxel_size)) if f32 else float(voxel_size)
    self.sdf_trunc = float(np.float32(sdf_trunc)) if f32 else float(sdf_trunc)
    self.dims = dims


class TSDFVolume:
    """A truncated signed distance volume of dims = (nx, ny, nz) voxels: `tsdf` and `weight` [nz,ny,nx], `color` [3,nz,ny,nx],
    contiguous and zero at first.  Indexing is 64-bit; a volume of more than 2^31 - 1 voxels is refused."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc, device="cuda", dtype=torch.float32):
        _init_grid(self, "TSDFVolume", origin, voxel_size, dims, sdf_trunc, dtype)
        dims = self.dims
        if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise ValueError(f"TSDFVolume: dims = {dims} are {dims[0] * dims[1] * dims[2]} voxels, more than 2^31 - 1")
        nx, ny, nz = dims
        self.tsdf = torch.zeros(nz, ny, nx, dtype=dtype, device=device)
        self.weight = torch.zeros(nz, ny, nx, dtype=dtype, device=device)
        self.color = torch.zeros(3, nz, ny, nx, dtype=dtype, device=device)

    def _use_native(self, native, what):
        on_gpu = self.tsdf.is_cuda and self.tsdf.dtype == torch.float32
        if native is None:
            return on_gpu
        if native and not on_gpu:
            raise RuntimeError(f"{what}: native=True needs an fp32 device volume (the HIP kernels have no CPU path)")
        return bool(native)

    def integrate(self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf, native=None):
        """Fuses one frame: `depth` and `alpha` are the [1,H,W] (or [H,W]) maps of depth_alpha=True as they are (`depth` the unnormalised
        weighted sum), `color` the image [3,H,W].  Per voxel, in this order: p_view of its centre, skipped unless z > 0; the pixel
        (floor(fx x / z + W/2), floor(fy y / z + H/2)), skipped unless inside the image; the pixel is valid when alpha >= alpha_min and
        depth > 0, then d = depth / alpha, skipped when invalid or d > depth_max; s = d - z, skipped unless s > -sdf_trunc;
        t = min(1, s / sdf_trunc) enters the running means of tsdf and colour, and the weight counts it.  A skipped voxel keeps every
        bit.  On the caller's stream, without a host synchronisation.  The maps receive no gradient (one that requires grad with grad
        mode on is a ValueError)."""
        H, W = _check_frame("TSDFVolume.integrate", self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        if not self._use_native(native, "TSDFVolume.integrate"):
            return integrate_torch(self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        if H * W == 0:
            return
        from . import _native
        _native.tsdf_integrate(self.dims, self.origin, self.voxel_size, self.sdf_trunc, viewmatrix.detach(), depth.detach(), alpha.detach(),
                               color.detach(), float(tanfovx), float(tanfovy), float(alpha_min), float(depth_max), self.tsdf, self.weight, self.color)

    def extract_mesh(self, min_weight=1.0, native=None):
        """-> (vertices [V,3] float32, faces [F,3] int32, colors [V,3] float32) by naive surface nets.  A voxel is observed when
        weight >= min_weight and inside when tsdf < 0; a cell (8 neighbouring voxels) is active when all 8 are observed and both signs
        occur, and owns one vertex: the mean of the crossing points of its sign-changing edges, coloured by the same interpolation.  A
        grid edge between two observed voxels of different sign emits one quad (two triangles, wound so that the normal points from
        the inside voxel to the outside one) when its four adjacent cells exist and are active.  Vertices come in ascending cell
        index, faces in ascending (voxel index, axis); every sign decision is made on the stored values, so the topology is exact.
        A volume thinner than 2 voxels along an axis, or without an active cell, gives an empty mesh."""
        if not self._use_native(native, "TSDFVolume.extract_mesh"):
            return extract_mesh_torch(self, min_weight)
        from . import _native
        return _native.tsdf_extract_mesh(self.dims, self.origin, self.voxel_size, float(min_weight), self.tsdf, self.weight, self.color)


# ---- the sparse volume (C ABI: include/gsrast_tsdf_sparse.h) ---------------------------------------------------------

BRICK = 8                                  # voxels along a brick's side
BRICK_VOXELS = BRICK ** 3
MAX_DIM = 32768
MAX_BRICKS = MAX_VOXELS // BRICK_VOXELS    # the pool's limit: 512 B <= 2^31 - 1
MIN_PAD = 1.25


def affine_inverse(viewmatrix):
    """The inverse of the view matrix's affine part (p_world = p_view @ M[:3,:3] + M[3,:3]) by the adjugate, in binary64 on the matrix's
    device and rounded to its dtype: element-wise torch ops, no host synchronisation."""
    M = viewmatrix.detach().double()
    r0, r1, r2, t = M[0, :3], M[1, :3], M[2, :3], M[3, :3]
    c0, c1, c2 = torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)
    inv = torch.stack([c0, c1, c2], 1) / (r0 * c0).sum()
    out = torch.zeros(4, 4, dtype=torch.float64, device=M.device)
    out[:3, :3] = inv
    out[3, :3] = -(t[:, None] * inv).sum(0)
    out[3, 3] = 1.0
    return out.to(viewmatrix.dtype).contiguous()


def allocate_torch(vol: "SparseTSDFVolume", depth, alpha, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf):
    """The marking rule as torch ops, in the volume's dtype: per valid pixel the box of its frustum piece's eight corners in voxel-index
    coordinates, grown by vol.pad, and a mark on every brick that holds an integer voxel coordinate of the grid inside it."""
    H, W = _check_frame("allocate_torch", vol, depth, alpha, None, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
    if H * W == 0:
        return
    dt, dev = vol.tsdf.dtype, vol.tsdf.device
    with torch.no_grad():
        Vinv = affine_inverse(viewmatrix)
        d_sum, a = depth.reshape(-1), alpha.reshape(-1)
        valid = (a >= float(np.float32(alpha_min))) & (d_sum > 0)
        one = torch.ones_like(a)
        d = torch.where(valid, d_sum, one) / torch.where(valid, a, one)
        p = (valid & ~(d > depth_max)).nonzero()[:, 0]
        if p.numel() == 0:
            return
        d, px, py = d[p], (p % W).to(dt), torch.div(p, W, rounding_mode="floor").to(dt)
        fx, fy = _focal(W, tanfovx, dt), _focal(H, tanfovy, dt)
        xs, ys = ((px - 0.5 * W) / fx, (px + 1 - 0.5 * W) / fx), ((py - 0.5 * H) / fy, (py + 1 - 0.5 * H) / fy)
        zs = (torch.clamp(d - vol.sdf_trunc, min=0.0), d + vol.sdf_trunc)
        lo = torch.full((p.numel(), 3), math.inf, dtype=dt, device=dev)
        hi = -lo
        for k in range(8):
            z = zs[k >> 2]
            x, y = xs[k & 1] * z, ys[(k >> 1) & 1] * z
            v = torch.stack([((x * Vinv[0, j] + (y * Vinv[1, j] + (z * Vinv[2, j] + Vinv[3, j]))) - vol.origin[j]) / vol.voxel_size for j in range(3)], 1)
            lo, hi = torch.minimum(lo, v), torch.maximum(hi, v)
        top = torch.tensor([n - 1 for n in vol.dims], dtype=dt, device=dev)
        first, last = torch.clamp(torch.ceil(lo - vol.pad), min=0.0), torch.minimum(torch.floor(hi + vol.pad), top)
        ok = (first <= last).all(1)                                                # (false for an empty range and for a NaN)
        if not bool(ok.any()):
            return
        blo, bhi = first[ok].long() >> 3, last[ok].long() >> 3
        nbx, nby, _ = vol.brick_dims
        marks = vol._marks.view(-1)
        ext = ((bhi - blo).max(0).values + 1).tolist()
        for dz in range(ext[2]):
            for dy in range(ext[1]):
                for dx in range(ext[0]):
                    b = blo + torch.tensor([dx, dy, dz], device=dev)
                    m = (b <= bhi).all(1)
                    marks[((b[m, 2] * nby + b[m, 1]) * nbx + b[m, 0])] = 1


def sparse_integrate_torch(vol: "SparseTSDFVolume", depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf):
    """integrate_torch's rule, operation for operation, over the voxels of the allocated bricks that lie inside the grid."""
    H, W = _check_frame("sparse_integrate_torch", vol, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
    B = vol._num
    if H * W == 0 or B == 0:
        return
    dt, dev = vol.tsdf.dtype, vol.tsdf.device
    nx, ny, nz = vol.dims
    with torch.no_grad():
        V = viewmatrix
        l = torch.arange(BRICK_VOXELS, device=dev)
        c = vol.brick_coords.long()
        ix, iy, iz = (BRICK * c[:, 0:1] + (l & 7)[None]).reshape(-1), (BRICK * c[:, 1:2] + ((l >> 3) & 7)[None]).reshape(-1), (BRICK * c[:, 2:3] + (l >> 6)[None]).reshape(-1)
        pool = ((ix < nx) & (iy < ny) & (iz < nz)).nonzero()[:, 0]                  # slot 512 + local of the voxels inside the grid
        wx, wy, wz = (vol.voxel_size * i[pool].to(dt) + o for i, o in zip((ix, iy, iz), vol.origin))
        x, y, z = (wx * V[0, j] + (wy * V[1, j] + (wz * V[2, j] + V[3, j])) for j in range(3))
        ok = z > 0
        zs = torch.where(ok, z, torch.ones_like(z))
        u = (_focal(W, tanfovx, dt) * x) / zs + 0.5 * W
        v = (_focal(H, tanfovy, dt) * y) / zs + 0.5 * H
        ok &= (u >= 0) & (u < W) & (v >= 0) & (v < H)
        sel = ok.nonzero()[:, 0]
        if sel.numel() == 0:
            return
        pix = torch.floor(v[sel]).long() * W + torch.floor(u[sel]).long()
        d_sum, a = depth.reshape(-1)[pix], alpha.reshape(-1)[pix]
        valid = (a >= float(np.float32(alpha_min))) & (d_sum > 0)
        one = torch.ones_like(a)
        d = torch.where(valid, d_sum, one) / torch.where(valid, a, one)
        s = d - z[sel]
        take = valid & ~(d > depth_max) & (s > -vol.sdf_trunc)
        idx, pix, s = pool[sel[take]], pix[take], s[take]
        t = torch.clamp(s / vol.sdf_trunc, max=1.0)
        tsdf, weight, col = vol.tsdf.reshape(-1), vol.weight.reshape(-1), vol.color.reshape(-1)      # (views: the pool is contiguous)
        w = weight[idx]
        tsdf[idx] = (tsdf[idx] * w + t) / (w + 1)
        cidx = torch.div(idx, BRICK_VOXELS, rounding_mode="floor") * (3 * BRICK_VOXELS) + idx % BRICK_VOXELS
        for ch in range(3):
            col[cidx + ch * BRICK_VOXELS] = (col[cidx + ch * BRICK_VOXELS] * w + color[ch].reshape(-1)[pix]) / (w + 1)
        weight[idx] = w + 1


def brick_order_key(cells, dims):
    """[V,3] voxel coordinates -> the int64 key of the sparse volume's order: 512 (brick linear index) + local voxel index."""
    nbx, nby = (dims[0] + BRICK - 1) // BRICK, (dims[1] + BRICK - 1) // BRICK
    x, y, z = (cells[:, j].long() for j in range(3))
    return (((z >> 3) * nby + (y >> 3)) * nbx + (x >> 3)) * BRICK_VOXELS + (((z & 7) << 6) | ((y & 7) << 3) | (x & 7))


def sparse_extract_mesh_torch(vol: "SparseTSDFVolume", min_weight=1.0, return_cells=False):
    """The torch twin of SparseTSDFVolume.extract_mesh: extract_mesh_torch on to_dense() (so at most 2^31 - 1 voxels), its vertices and
    quads then taken to the sparse volume's order.  A quad is two consecutive faces (v0, v1, v2), (v0, v2, v3) or their mirror images;
    v2 is the vertex of its voxel's own cell, and the axis is the coordinate in which the cells of v0 and v2 agree."""
    v, f, c, cells = extract_mesh_torch(vol.to_dense(), min_weight, return_cells=True)
    with torch.no_grad():
        if v.shape[0]:
            perm = torch.argsort(brick_order_key(cells, vol.dims))
            inv = torch.empty_like(perm)
            inv[perm] = torch.arange(perm.numel(), device=perm.device)
            v, c, cells = v[perm], c[perm], cells[perm]
            if f.shape[0]:
                q = f.long().reshape(-1, 6)
                a, b = q[:, 1], q[:, 2]
                own = torch.where((a == q[:, 4]) | (a == q[:, 5]), a, b)
                same = cells[inv[own]] == cells[inv[q[:, 0]]]
                axis = same.to(torch.int64).argmax(1)
                order = torch.argsort(brick_order_key(cells[inv[own]], vol.dims) * 3 + axis)
                f = inv[q[order]].reshape(-1, 3).to(torch.int32)
    return (v, f, c, cells) if return_cells else (v, f, c)


class SparseTSDFVolume:
    """TSDFVolume's virtual grid (origin, voxel_size, dims = (nx, ny, nz), sdf_trunc), stored as bricks of 8 x 8 x 8 voxels that exist only
    where a depth map put a surface.  Brick (bx, by, bz) holds the voxels 8 bx .. 8 bx + 7 along x and likewise along y and z; dims
    need not be multiples of 8, and no dimension may exceed 32768.

      brick_table [nbz,nby,nbx] int32    the slot of an allocated brick, -1 elsewhere (at most 2^31 - 1 entries)
      brick_coords [B,3] int32           (bx, by, bz) of every slot; num_bricks == B
      tsdf, weight [B,8,8,8], color [B,3,8,8,8]     a brick's voxels [z,y,x]: views of capacity buffers that grow geometrically, zero at
                                         allocation; at most 2^31 - 1 voxels in the pool

    A voxel of an unallocated brick is unobserved (weight 0); a voxel of an allocated brick beyond dims is never written.

    allocate(frame) marks the bricks the frame's depths can reach; the marks are pending until the next integrate, extract_mesh,
    num_bricks or commit(), which gives the newly marked bricks the next slots in ascending brick linear index (one host
    synchronisation per commit, not per allocate).  Allocated bricks keep their slots and contents.

    Every frame's allocate first and every frame's integrate afterwards (two passes): every voxel of an allocated brick holds the bits
    TSDFVolume holds after the same frames, and extract_mesh gives TSDFVolume's mesh - the same vertices, colours and faces - in the
    order documented there.  allocate(f); integrate(f) frame by frame (streaming, Open3D's behaviour): a brick holds exactly the frames
    from the one that allocated it on, and the free-space carving of earlier frames is lost there.

    Why the marks suffice (pad >= 1): a voxel that receives a sample |s| < sdf_trunc from a pixel lies in that pixel's frustum piece;
    every voxel within Chebyshev distance 1 of it lies in the marked box; surface nets reads the 2 x 2 x 2 voxels of a cell and the
    2 x 3 x 3 voxels around an edge, all within Chebyshev distance 1 of the edge's inside voxel; and a voxel with tsdf < 0 received
    s < 0 from some frame.  pad < 1.25 is a ValueError: the quarter voxel pays for the binary32 evaluation of the box."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc, device="cuda", dtype=torch.float32, pad=1.5, capacity=0):
        _init_grid(self, "SparseTSDFVolume", origin, voxel_size, dims, sdf_trunc, dtype)
        if max(self.dims) > MAX_DIM:
            raise ValueError(f"SparseTSDFVolume: dims = {self.dims}: no dimension may exceed {MAX_DIM}")
        self.brick_dims = tuple((n + BRICK - 1) // BRICK for n in self.dims)
        nbx, nby, nbz = self.brick_dims
        if nbx * nby * nbz > MAX_VOXELS:
            raise ValueError(f"SparseTSDFVolume: dims = {self.dims} need a brick table of {nbx * nby * nbz} entries, more than 2^31 - 1")
        if not (pad >= MIN_PAD and math.isfinite(pad)):
            raise ValueError(f"SparseTSDFVolume: pad = {pad} voxels: at least {MIN_PAD} (1 for the stencils, 0.25 for the rounding) and finite expected")
        self.pad = float(np.float32(pad))
        self.brick_table = torch.full((nbz, nby, nbx), -1, dtype=torch.int32, device=device)
        self._marks = torch.zeros(nbz, nby, nbx, dtype=torch.int32, device=device)
        self._dtype, self._num, self._pending, self.growths = dtype, 0, False, 0
        self._tsdf = self._weight = self._color = self._coords = self._order = self._rank = None
        self._resize(int(capacity))

    # ---- the pool
    @property
    def capacity(self):
        return int(self._coords.shape[0])

    def _resize(self, capacity):
        if capacity < 0 or capacity > MAX_BRICKS:
            raise ValueError(f"SparseTSDFVolume: a pool of {capacity} bricks is {capacity * BRICK_VOXELS} voxels, more than 2^31 - 1")
        dev, B = self.brick_table.device, self._num
        new = (torch.zeros(capacity, BRICK, BRICK, BRICK, dtype=self._dtype, device=dev), torch.zeros(capacity, BRICK, BRICK, BRICK, dtype=self._dtype, device=dev),
               torch.zeros(capacity, 3, BRICK, BRICK, BRICK, dtype=self._dtype, device=dev), torch.zeros(capacity, 3, dtype=torch.int32, device=dev),
               torch.zeros(capacity, dtype=torch.int32, device=dev), torch.zeros(capacity, dtype=torch.int32, device=dev))
        old = (self._tsdf, self._weight, self._color, self._coords, self._order, self._rank)
        if B:
            for n, o in zip(new, old):
                n[:B].copy_(o[:B])
        self._tsdf, self._weight, self._color, self._coords, self._order, self._rank = new

    def _make_room(self, need):
        if need <= self.capacity:
            return
        if need > MAX_BRICKS:
            raise ValueError(f"SparseTSDFVolume: {need} bricks are {need * BRICK_VOXELS} voxels, more than 2^31 - 1")
        self._resize(min(max(need, 2 * self.capacity), MAX_BRICKS))
        self.growths += 1

    @property
    def num_bricks(self):
        self.commit()
        return self._num

    tsdf = property(lambda self: self._tsdf[:self._num])
    weight = property(lambda self: self._weight[:self._num])
    color = property(lambda self: self._color[:self._num])
    brick_coords = property(lambda self: self._coords[:self._num])

    def _use_native(self, native, what):
        on_gpu = self.brick_table.is_cuda and self._dtype == torch.float32
        if native is None:
            return on_gpu
        if native and not on_gpu:
            raise RuntimeError(f"{what}: native=True needs an fp32 device volume (the HIP kernels have no CPU path)")
        return bool(native)

    # ---- the three operations
    def allocate(self, depth, alpha, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf, native=None):
        """Marks the bricks this frame's depths can reach: one HIP launch, a thread per pixel, on the caller's stream, without a host
        synchronisation.  A pixel is valid by integrate's own tests (alpha >= alpha_min, depth > 0, d = depth / alpha <= depth_max); its
        frustum piece - the footprint [px, px + 1] x [py, py + 1] between the view depths max(d - sdf_trunc, 0) and d + sdf_trunc - goes
        to world space by its eight corners through the inverse of the view matrix's affine part (affine_inverse, on the device);
        every brick that holds an integer voxel coordinate of the grid inside the corners' axis-aligned box, grown by `pad` voxels, is
        marked.  The marks are pending until the next commit."""
        H, W = _check_frame("SparseTSDFVolume.allocate", self, depth, alpha, None, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        self._pending = True
        if not self._use_native(native, "SparseTSDFVolume.allocate"):
            return allocate_torch(self, depth, alpha, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        if H * W == 0:
            return
        from . import _native
        _native.tsdf_sparse_allocate(self.dims, self.origin, self.voxel_size, self.sdf_trunc, self.pad, affine_inverse(viewmatrix), depth.detach(),
                                     alpha.detach(), float(tanfovx), float(tanfovy), float(alpha_min), float(depth_max), self._marks)

    def commit(self, native=None):
        """Gives the bricks marked since the last commit their slots, in ascending brick linear index, grows the pool if they need it
        and clears the marks -> the number of new bricks.  One host readback; with nothing pending it does nothing at all."""
        if not self._pending:
            return 0
        nbx, nby, _ = self.brick_dims
        if self._use_native(native, "SparseTSDFVolume.commit"):
            from . import _native
            new, ws, nbytes = _native.tsdf_sparse_commit_count(self.dims, self._marks, self.brick_table)
            self._make_room(self._num + new)
            _native.tsdf_sparse_commit_assign(self.dims, self._num, self._marks, self.brick_table, ws, nbytes, self._coords, self._order, self._rank)
        else:
            with torch.no_grad():
                table = self.brick_table.view(-1)
                e = ((self._marks.view(-1) != 0) & (table < 0)).nonzero()[:, 0]
                new = int(e.numel())
                self._make_room(self._num + new)
                table[e] = torch.arange(self._num, self._num + new, dtype=torch.int32, device=table.device)
                self._coords[self._num:self._num + new] = torch.stack([e % nbx, torch.div(e, nbx, rounding_mode="floor") % nby,
                                                                       torch.div(e, nbx * nby, rounding_mode="floor")], 1).to(torch.int32)
                live = table[table >= 0]                                            # the slots in ascending brick linear index
                self._order[:live.numel()] = live
                self._rank[live.long()] = torch.arange(live.numel(), dtype=torch.int32, device=table.device)
                self._marks.zero_()
        self._num += new
        self._pending = False
        return new

    def integrate(self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min=0.5, depth_max=math.inf, native=None):
        """Commits the pending marks, then fuses one frame by TSDFVolume.integrate's rule - the same per-voxel functions, free-space
        carving included - into every voxel of every allocated brick: one HIP launch, a block per brick, on the caller's stream.  A
        skipped voxel keeps every bit; a brick wholly behind the camera or wholly outside one side of the frustum returns as a whole
        (every voxel of it would have been skipped)."""
        H, W = _check_frame("SparseTSDFVolume.integrate", self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        native = self._use_native(native, "SparseTSDFVolume.integrate")
        self.commit(native)
        if not native:
            return sparse_integrate_torch(self, depth, alpha, color, viewmatrix, tanfovx, tanfovy, alpha_min, depth_max)
        if H * W == 0 or self._num == 0:
            return
        from . import _native
        _native.tsdf_sparse_integrate(self.dims, self.origin, self.voxel_size, self.sdf_trunc, viewmatrix.detach(), depth.detach(), alpha.detach(),
                                      color.detach(), float(tanfovx), float(tanfovy), float(alpha_min), float(depth_max), self._num, self._coords,
                                      self._tsdf, self._weight, self._color)

    def extract_mesh(self, min_weight=1.0, return_cells=False, native=None):
        """TSDFVolume.extract_mesh's surface nets through the brick table: an unallocated brick, a voxel outside dims and a voxel with
        weight < min_weight are unobserved.  Vertices come in ascending (brick linear index, local voxel index) of their cell's
        lowest corner, faces in ascending (that order, axis), so the mesh does not depend on the order in which bricks were allocated.
        return_cells=True adds [V,3] int32, the lowest-corner voxel (ix, iy, iz) of every vertex's cell."""
        native = self._use_native(native, "SparseTSDFVolume.extract_mesh")
        self.commit(native)
        if not native:
            return sparse_extract_mesh_torch(self, min_weight, return_cells)
        from . import _native
        v, f, c, cells = _native.tsdf_sparse_extract_mesh(self.dims, self.origin, self.voxel_size, float(min_weight), self._num, self._tsdf, self._weight,
                                                          self._color, self.brick_table, self._coords, self._order, self._rank, return_cells)
        return (v, f, c, cells) if return_cells else (v, f, c)

    def to_dense(self) -> TSDFVolume:
        """The same volume as a TSDFVolume (unallocated bricks zero), for tests and small volumes: more than 2^31 - 1 voxels are refused."""
        self.commit()
        dense = TSDFVolume(self.origin, self.voxel_size, self.dims, self.sdf_trunc, device=self.brick_table.device, dtype=self._dtype)
        nx, ny, nz = self.dims
        nbx, nby, nbz = self.brick_dims
        if nbx * nby * nbz * BRICK_VOXELS > MAX_VOXELS:
            raise ValueError(f"SparseTSDFVolume.to_dense: {nbx * nby * nbz} bricks are more than 2^31 - 1 voxels")
        bx, by, bz = (self.brick_coords[:, j].long() for j in range(3))
        with torch.no_grad():
            for dst, src in ((dense.tsdf, self.tsdf), (dense.weight, self.weight)) + tuple((dense.color[c], self.color[:, c]) for c in range(3)):
                padded = torch.zeros(nbz, BRICK, nby, BRICK, nbx, BRICK, dtype=self._dtype, device=dst.device)
                padded[bz, :, by, :, bx, :] = src
                dst.copy_(padded.view(nbz * BRICK, nby * BRICK, nbx * BRICK)[:nz, :ny, :nx])
        return dense
