"""TSDF fusion of depth maps and mesh extraction by surface nets: where the surface pipeline of 2DGS, Gaussian Opacity Fields, RaDe-GS
and PGSR ends.  Depth maps rendered from the training cameras are fused into a truncated signed distance volume, and a triangle mesh
is extracted from it (csrc/gsr_tsdf.hip; C ABI: include/gsrast_tsdf.h).

  TSDFVolume.integrate      one frame into the volume: one HIP launch, a thread per voxel, no host synchronisation
  TSDFVolume.extract_mesh   naive surface nets (the dual of marching cubes: no case table) in three HIP stages, one host readback

fp32 device volumes run the kernels; host volumes, and `native=False`, take the same rules as torch ops (`integrate_torch`,
`extract_mesh_torch`, in the volume's dtype).  `native=True` on host tensors raises: there is no silent fallback.  No atomic is used:
the same frames in the same order give the same bits, and so does the same volume.

Conventions (those of normals.py): row-vector matrices (p_view = p @ V[:3,:3] + V[3,:3]); fx = W / (2 tanfovx), fy = H / (2 tanfovy);
pixel (x, y) has its centre at x + 0.5.  The volume is indexed [z, y, x]; voxel (ix, iy, iz) has its centre at
origin + voxel_size * (ix, iy, iz).

The fusion rule is KinectFusion's and Open3D's projective rule with free-space carving, restated from the literature.  Out of scope:
median depth, unbounded (contracted) volumes, sparse voxel hashing and decimation (mesh cleaning: meshops.py).
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
    for name, t in (("depth", depth), ("alpha", alpha), ("color", color), ("viewmatrix", viewmatrix)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: {name} must be a tensor, got {type(t).__name__}")
    if depth.dim() not in (2, 3) or (depth.dim() == 3 and depth.shape[0] != 1):
        raise ValueError(f"{what}: depth [1,H,W] or [H,W] expected, got {tuple(depth.shape)}")
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    if alpha.dim() not in (2, 3) or tuple(alpha.shape[-2:]) != (H, W) or alpha.numel() != H * W:
        raise ValueError(f"{what}: alpha [1,H,W] or [H,W] expected for H, W = {H}, {W}, got {tuple(alpha.shape)}")
    if tuple(color.shape) != (3, H, W):
        raise ValueError(f"{what}: color [3,H,W] expected for H, W = {H}, {W}, got {tuple(color.shape)}")
    if tuple(viewmatrix.shape) != (4, 4):
        raise ValueError(f"{what}: viewmatrix [4,4] expected, got {tuple(viewmatrix.shape)}")
    for name, t in (("depth", depth), ("alpha", alpha), ("color", color), ("viewmatrix", viewmatrix)):
        if t.dtype != vol.tsdf.dtype or t.device != vol.tsdf.device:
            raise ValueError(f"{what}: {name} is {t.dtype} on {t.device}, the volume {vol.tsdf.dtype} on {vol.tsdf.device}: one device and "
                             "one float dtype expected")
        if not t.is_contiguous():
            raise ValueError(f"{what}: {name} is not contiguous")
    if not (tanfovx > 0 and tanfovy > 0 and alpha_min > 0 and np.isfinite([tanfovx, tanfovy, alpha_min]).all()):
        raise ValueError(f"{what}: tanfovx = {tanfovx}, tanfovy = {tanfovy}, alpha_min = {alpha_min}: positive and finite expected")
    if not depth_max > 0:
        raise ValueError(f"{what}: depth_max = {depth_max}: positive expected (inf cuts nothing)")
    _refuse_grad(what, depth=depth, alpha=alpha, color=color, viewmatrix=viewmatrix)
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


def extract_mesh_torch(vol: "TSDFVolume", min_weight=1.0):
    """Surface nets as torch ops, in the volume's dtype -> (vertices [V,3], faces [F,3] int32, colors [V,3])."""
    dt, dev = vol.tsdf.dtype, vol.tsdf.device
    nx, ny, nz = vol.dims
    empty = (torch.zeros(0, 3, dtype=dt, device=dev), torch.zeros(0, 3, dtype=torch.int32, device=dev), torch.zeros(0, 3, dtype=dt, device=dev))
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


class TSDFVolume:
    """A truncated signed distance volume of dims = (nx, ny, nz) voxels: `tsdf` and `weight` [nz,ny,nx], `color` [3,nz,ny,nx],
    contiguous and zero at first.  Indexing is 64-bit; a volume of more than 2^31 - 1 voxels is refused."""

    def __init__(self, origin, voxel_size, dims, sdf_trunc, device="cuda", dtype=torch.float32):
        origin = tuple(float(v) for v in (origin.tolist() if hasattr(origin, "tolist") else origin))
        dims = tuple(int(v) for v in dims)
        if len(origin) != 3 or not np.isfinite(origin).all():
            raise ValueError(f"TSDFVolume: origin = {origin}: three finite numbers expected")
        if len(dims) != 3 or min(dims) < 1:
            raise ValueError(f"TSDFVolume: dims = {dims}: three dimensions of at least one voxel expected")
        if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
            raise ValueError(f"TSDFVolume: dims = {dims} are {dims[0] * dims[1] * dims[2]} voxels, more than 2^31 - 1")
        if not (voxel_size > 0 and math.isfinite(voxel_size)):
            raise ValueError(f"TSDFVolume: voxel_size = {voxel_size}: positive and finite expected")
        if not (sdf_trunc > 0 and math.isfinite(sdf_trunc)):
            raise ValueError(f"TSDFVolume: sdf_trunc = {sdf_trunc}: positive and finite expected")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError(f"TSDFVolume: dtype = {dtype}: float32 (the kernels') or float64 (the torch twin only)")
        f32 = dtype == torch.float32                   # a binary32 volume holds the binary32 numbers the kernels receive
        self.origin = tuple(float(np.float32(v)) for v in origin) if f32 else origin
        self.voxel_size = float(np.float32(voxel_size)) if f32 else float(voxel_size)
        self.sdf_trunc = float(np.float32(sdf_trunc)) if f32 else float(sdf_trunc)
        self.dims = dims
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
