"""From a trained cloud to a triangle mesh: render depth from every camera, fuse the depth maps into a truncated signed distance volume,
extract the surface (diff_gaussian_rasterization/tsdf.py).  The route 2DGS, Gaussian Opacity Fields, RaDe-GS and PGSR
all end in, without leaving the device.

The functions work with any model render() accepts: a GaussianModel (with or without a 3D filter), a LatentGaussianModel.  Projective
fusion of a few views leaves holes and silhouette artefacts by nature: clean_mesh (diff_gaussian_rasterization/meshops.py, DESIGN
section 27) drops the small detached pieces on the device.  depth_ratio (2DGS's; 0, the default: the expected depth; 2DGS uses 1, the
median depth, for bounded scenes) chooses the depth that is fused (diff_gaussian_rasterization.normals.surface_depth, DESIGN section
28): at a silhouette or behind a thin layer the expected depth is a blend at which nothing exists, the median is a splat's own.
sparse=True fuses into a SparseTSDFVolume (bricks of 8 x 8 x 8 voxels allocated where the depth maps put a surface):
the same mesh at a fraction of the memory, and the resolutions the dense volume cannot hold.  Decimation, unbounded (contracted)
volumes, hashing in place of the dense brick table and brick deallocation are out of scope.
"""
import math
import os

import numpy as np
import torch

VOLUME_RESOLUTION = 512          # voxels along the default cube's side
SPARSE_RESOLUTION = 1024         # the same of a sparse volume (2DGS's mesh_res)
TRUNC_VOXELS = 5.0               # the default sdf_trunc, in voxels


def _tanfov(cam):
    return math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)


def fuse_depth_maps(pc, cameras, pipe, background, volume, alpha_min=0.5, depth_max=None, depth_ratio=0.0, two_pass=True):
    """Per camera, under torch.no_grad(): render(..., depth_alpha=True), then volume.integrate of its depth, alpha and colour maps.
    depth_max None: nothing is cut.  depth_ratio in [0, 1] (0: the calls made without it): above 0 the frame also renders the median
    depth and surface_depth(depth, alpha, median, depth_ratio) is integrated in the depth map's place, beside the same alpha.
    two_pass applies to a SparseTSDFVolume alone (a dense volume takes the calls above, whatever it says).  True: the frames are
    rendered twice, first for volume.allocate and then for volume.integrate, and the maps are not kept: every allocated brick holds
    what the dense volume holds.  False: one render per frame, volume.allocate and volume.integrate on it (streaming: a brick holds
    the frames from the one that allocated it on).  Returns the volume."""
    from gaussian_renderer import render
    from diff_gaussian_rasterization.normals import surface_depth
    depth_max = math.inf if depth_max is None else float(depth_max)
    depth_ratio = float(depth_ratio)
    if not 0.0 <= depth_ratio <= 1.0:
        raise ValueError(f"fuse_depth_maps: depth_ratio {depth_ratio} outside [0, 1]")
    sparse = hasattr(volume, "allocate")
    for step in (("allocate", "integrate") if sparse and two_pass else ("both",) if sparse else ("integrate",)):
        with torch.no_grad():
            for cam in cameras:
                if depth_ratio > 0.0:
                    pkg = render(cam, pc, pipe, background, depth_alpha=True, median_depth=True)
                    pkg["depth"] = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], depth_ratio)
                else:
                    pkg = render(cam, pc, pipe, background, depth_alpha=True)
                tx, ty = _tanfov(cam)
                if step != "integrate":
                    volume.allocate(pkg["depth"].contiguous(), pkg["alpha"].contiguous(), cam.world_view_transform.contiguous(), tx, ty,
                                    alpha_min=alpha_min, depth_max=depth_max)
                if step != "allocate":
                    volume.integrate(pkg["depth"].contiguous(), pkg["alpha"].contiguous(), pkg["render"].contiguous(),
                                     cam.world_view_transform.contiguous(), tx, ty, alpha_min=alpha_min, depth_max=depth_max)
    return volume


def camera_bounds(cameras):
    """(lo [3], side): the cube around the centroid of the camera centres whose half-side is the largest camera distance from the
    centroid (2DGS's bounded mode)."""
    centres = torch.stack([c.camera_center.detach().reshape(3).double().cpu() for c in cameras])
    centroid = centres.mean(0)
    half = float((centres - centroid).norm(dim=1).max())
    if not half > 0:
        raise ValueError("extract_mesh: the cameras share one centre, which bounds no volume: pass bounds=(lo, hi)")
    return (centroid - half).tolist(), 2.0 * half


def clean_mesh(vertices, faces, colors=None, **kw):
    """diff_gaussian_rasterization.meshops.clean_mesh: drops the faces of components smaller than max(min_faces, the size of the
    keep_largest-th largest component), invalid faces and unused vertices (kw: min_faces, keep_largest, return_index, native)."""
    from diff_gaussian_rasterization.meshops import clean_mesh as clean
    return clean(vertices, faces, colors, **kw)


def extract_mesh(pc, cameras, pipe, background, voxel_size=None, sdf_trunc=None, bounds=None, depth_max=None, min_weight=1.0,
                 min_component_faces=None, keep_largest=None, depth_ratio=0.0, sparse=False, resolution=None, two_pass=True):
    """-> (vertices [V,3] float32, faces [F,3] int32, colors [V,3] float32) of the surface the cameras see.
    bounds: (lo [3], hi [3]); default camera_bounds(cameras).  voxel_size: default the bounds' longest side / resolution; resolution
    (voxels along the longest side; giving both is a ValueError): default 512, and 1024 with sparse=True.  sparse: fuse into a
    SparseTSDFVolume (two_pass: fuse_depth_maps'); the mesh is the dense volume's at the same voxel size, its vertices and faces in
    the sparse volume's order.  sdf_trunc: default
    5 voxel_size.  depth_max: default the bounds' longest side.  min_component_faces, keep_largest: when either is given the mesh is
    cleaned after the extraction (clean_mesh's min_faces and keep_largest); with both None it is returned as extracted.
    depth_ratio: fuse_depth_maps' (0: the expected depth; 1: the median depth, 2DGS's choice for bounded scenes)."""
    from diff_gaussian_rasterization.tsdf import SparseTSDFVolume, TSDFVolume
    cameras = list(cameras)
    if not cameras:
        raise ValueError("extract_mesh: no cameras")
    if bounds is None:
        lo, side = camera_bounds(cameras)
        hi = [v + side for v in lo]
    else:
        lo, hi = ([float(v) for v in b] for b in bounds)
        if len(lo) != 3 or len(hi) != 3 or not all(h > l for l, h in zip(lo, hi)):
            raise ValueError(f"extract_mesh: bounds = {bounds}: (lo [3], hi [3]) with hi > lo expected")
        side = max(h - l for l, h in zip(lo, hi))
    if resolution is not None and (voxel_size is not None or not resolution >= 1):
        raise ValueError(f"extract_mesh: resolution = {resolution}, voxel_size = {voxel_size}: one of them, the resolution at least 1 voxel")
    if resolution is None:
        resolution = SPARSE_RESOLUTION if sparse else VOLUME_RESOLUTION
    voxel_size = side / resolution if voxel_size is None else float(voxel_size)
    sdf_trunc = TRUNC_VOXELS * voxel_size if sdf_trunc is None else float(sdf_trunc)
    depth_max = side if depth_max is None else float(depth_max)
    if not voxel_size > 0:
        raise ValueError(f"extract_mesh: voxel_size = {voxel_size}: positive expected")
    # the bounds cut into voxels, a voxel's centre in the middle of its cut: side / voxel_size voxels along the longest side
    dims = tuple(max(int(math.ceil((h - l) / voxel_size - 1e-6)), 1) for l, h in zip(lo, hi))
    volume = (SparseTSDFVolume if sparse else TSDFVolume)([l + 0.5 * voxel_size for l in lo], voxel_size, dims, sdf_trunc, device=pc.get_xyz.device)
    fuse_depth_maps(pc, cameras, pipe, background, volume, depth_max=depth_max, depth_ratio=depth_ratio, two_pass=two_pass)
    mesh = volume.extract_mesh(min_weight=min_weight)
    if min_component_faces is None and keep_largest is None:
        return mesh
    return clean_mesh(*mesh, min_faces=1 if min_component_faces is None else min_component_faces, keep_largest=keep_largest)


_PLY_VERTEX = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
_PLY_FACE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def save_mesh_ply(path, vertices, faces, colors):
    """Binary little-endian PLY: float positions, uchar colours (rounded from [0,1], clamped), int32 triangle lists."""
    host = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v, f, c = host(vertices).astype(np.float32).reshape(-1, 3), host(faces).astype(np.int32).reshape(-1, 3), host(colors).astype(np.float64).reshape(-1, 3)
    if c.shape[0] != v.shape[0]:
        raise ValueError(f"save_mesh_ply: {v.shape[0]} vertices, {c.shape[0]} colours")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("save_mesh_ply: a face names a vertex that does not exist")
    vert = np.empty(v.shape[0], _PLY_VERTEX)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    rgb = np.rint(np.clip(np.nan_to_num(c), 0.0, 1.0) * 255.0).astype(np.uint8)
    vert["red"], vert["green"], vert["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    face = np.empty(f.shape[0], _PLY_FACE)
    face["n"], face["v"] = 3, f
    header = ("ply\nformat binary_little_endian 1.0\n"
              f"element vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\n"
              f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as fh:
        fh.write(header.encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


def load_mesh_ply(path):
    """What save_mesh_ply wrote -> (vertices [V,3] float32, faces [F,3] int32, colors [V,3] uint8) as numpy arrays."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    if lines[0] != "ply" or lines[1] != "format binary_little_endian 1.0":
        raise ValueError(f"load_mesh_ply: {path} is not a binary little-endian PLY")
    counts = {w[1]: int(w[2]) for w in (line.split() for line in lines) if len(w) == 3 and w[0] == "element"}
    props = [line for line in lines if line.startswith("property")]
    want = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
            "property list uchar int vertex_indices"]
    if props != want or set(counts) != {"vertex", "face"}:
        raise ValueError(f"load_mesh_ply: {path} does not have save_mesh_ply's layout")
    nv, nf = counts["vertex"], counts["face"]
    if len(data) != end + nv * _PLY_VERTEX.itemsize + nf * _PLY_FACE.itemsize:
        raise ValueError(f"load_mesh_ply: {path} is {len(data)} bytes, its header describes {end + nv * _PLY_VERTEX.itemsize + nf * _PLY_FACE.itemsize}")
    vert = np.frombuffer(data, _PLY_VERTEX, nv, end)
    face = np.frombuffer(data, _PLY_FACE, nf, end + nv * _PLY_VERTEX.itemsize)
    if nf and not (face["n"] == 3).all():
        raise ValueError(f"load_mesh_ply: {path} holds a face that is not a triangle")
    return (np.stack([vert["x"], vert["y"], vert["z"]], 1).astype(np.float32).reshape(-1, 3), face["v"].astype(np.int32).reshape(-1, 3),
            np.stack([vert["red"], vert["green"], vert["blue"]], 1).astype(np.uint8).reshape(-1, 3))
