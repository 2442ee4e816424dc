"""Mesh cleaning on the device: the connected pieces of a triangle mesh are labelled, the small ones dropped, then the vertices nobody
uses - the step every surface pipeline (2DGS, Gaussian Opacity Fields, RaDe-GS, PGSR) ends with, behind tsdf.py's extraction
(csrc/gsr_mesh.hip; C ABI: include/gsrast_mesh.h).

  face_components   a lock-free union-find over the vertices in three HIP launches: no host loop, no readback
  clean_mesh        the components, a threshold chosen on the device, an ordered compaction in six launches and one host readback

The rule (csrc/gsr_mesh_math.h states it once).  A mesh is faces [F,3] int32 over V vertices.  A face is valid when its three indices
lie in [0, V) and are pairwise different; any other face joins nothing, belongs to no component and is always dropped.  Two valid faces
are connected when they share a VERTEX (Open3D's cluster_connected_triangles connects over shared edges: the two rules differ only
where sheets touch in a single point).  A component's label is the smallest vertex index it contains: labels [F] holds it per face, -1
for an invalid face; sizes [V] holds at index `label` the component's number of faces, 0 elsewhere.  threshold = max(min_faces, s_n),
s_n the size of the keep_largest-th largest component (absent when keep_largest is None or there are fewer components); a face is kept
when it is valid and sizes[label] >= threshold, so ties at the threshold are all kept (2DGS's post-processing rule, restated from its
description).  A vertex is kept when a kept face names it; kept faces and vertices keep their relative order, faces are re-indexed.

Device tensors run the kernels; host tensors, and `native=False`, take the same rule as torch ops (`face_components_torch`,
`clean_mesh_torch`: the same integers).  `native=True` on host tensors raises: there is no silent fallback.  The kernels move integers
only; positions and colours are gathered with index_select, which is bit-exact.  No atomic decides an order or a label: the same mesh
gives the same integers.

Out of scope: shared-edge connectivity, vertex normals, smoothing, decimation, hole filling.
"""
from __future__ import annotations

import torch

MAX_ROWS = 2 ** 31 - 1


def _check_faces(what, faces, num_vertices):
    if not isinstance(faces, torch.Tensor):
        raise ValueError(f"{what}: faces must be a tensor, got {type(faces).__name__}")
    if faces.dim() != 2 or faces.shape[1] != 3 or faces.dtype != torch.int32:
        raise ValueError(f"{what}: faces [F,3] int32 expected, got {tuple(faces.shape)} {faces.dtype}")
    if not faces.is_contiguous():
        raise ValueError(f"{what}: faces is not contiguous")
    V = int(num_vertices)
    if V < 0 or V > MAX_ROWS or faces.shape[0] > MAX_ROWS:
        raise ValueError(f"{what}: V = {V}, F = {faces.shape[0]}: 0 .. 2^31 - 1 each expected")
    return V, int(faces.shape[0])


def _use_native(native, faces, what):
    if native is None:
        return faces.is_cuda
    if native and not faces.is_cuda:
        raise RuntimeError(f"{what}: native=True needs device tensors (the HIP kernels have no CPU path)")
    return bool(native)


def face_components_torch(faces, num_vertices):
    """The rule as torch ops -> (labels [F] int32, sizes [V] int32): min-label propagation over the faces (scatter_reduce_ "amin") and
    pointer jumping, to a fixpoint."""
    V, F = _check_faces("face_components_torch", faces, num_vertices)
    dev = faces.device
    f = faces.long()
    valid = ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])
    fv = f[valid]
    lab = torch.arange(V, dtype=torch.int64, device=dev)
    flat = fv.reshape(-1)
    while fv.shape[0]:
        new = lab.clone()
        new.scatter_reduce_(0, flat, lab[fv].amin(1).repeat_interleave(3), "amin")         # a face's vertices take its smallest label
        while True:                                                                        # pointer jumping: new[v] <= v, so it ends
            hop = new[new]
            if torch.equal(hop, new):
                break
            new = hop
        if torch.equal(new, lab):
            break
        lab = new
    labels = torch.full((F,), -1, dtype=torch.int32, device=dev)
    labels[valid] = lab[fv[:, 0]].to(torch.int32)
    sizes = torch.bincount(lab[fv[:, 0]], minlength=V)[:V].to(torch.int32) if V else torch.zeros(0, dtype=torch.int32, device=dev)
    return labels, sizes


def face_components(faces, num_vertices, native=None):
    """-> (labels [F] int32, sizes [V] int32) of faces [F,3] int32 over num_vertices vertices: a component's label is the smallest vertex
    index it contains (-1 for an invalid face), sizes[label] its number of faces (0 elsewhere).  On the caller's current stream and
    the faces' device, without a host synchronisation.  The union-find's loops are bounded by what their proof allows; a bound that
    is hit is reported by clean_mesh (RuntimeError) - here the results would be unspecified."""
    V, _ = _check_faces("face_components", faces, num_vertices)
    if not _use_native(native, faces, "face_components"):
        return face_components_torch(faces, V)
    from . import _native
    return _native.mesh_components(faces, V)[:2]


def _check_mesh(what, vertices, faces, colors, min_faces, keep_largest):
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError(f"{what}: vertices [V,3] expected, got {tuple(vertices.shape) if isinstance(vertices, torch.Tensor) else type(vertices).__name__}")
    V, F = _check_faces(what, faces, vertices.shape[0])
    if colors is not None and (not isinstance(colors, torch.Tensor) or tuple(colors.shape) != (V, 3)):
        raise ValueError(f"{what}: colors [V,3] expected for V = {V}, got {tuple(colors.shape) if isinstance(colors, torch.Tensor) else type(colors).__name__}")
    for name, t in (("faces", faces), ("colors", colors)):
        if t is not None and t.device != vertices.device:
            raise ValueError(f"{what}: {name} is on {t.device}, vertices on {vertices.device}: one device expected")
    if int(min_faces) != min_faces or min_faces < 1:
        raise ValueError(f"{what}: min_faces = {min_faces}: an integer >= 1 expected")
    if keep_largest is not None and (int(keep_largest) != keep_largest or keep_largest < 1):
        raise ValueError(f"{what}: keep_largest = {keep_largest}: None or an integer >= 1 expected")
    return V, F


def _threshold(sizes, min_faces, keep_largest):
    """max(min_faces, s_n) as a one-element int32 tensor on sizes' device, without a synchronisation: s_n by torch.topk over sizes (a
    zero there: fewer components than keep_largest, and min_faces >= 1 wins)."""
    thr = torch.full((1,), min(int(min_faces), MAX_ROWS), dtype=torch.int32, device=sizes.device)
    if keep_largest is not None and sizes.numel():
        k = min(int(keep_largest), sizes.numel())
        thr = torch.maximum(thr, torch.topk(sizes, k).values[k - 1:k])
    return thr


def _gather(vertices, colors, vertex_src, face_src, faces_out, return_index):
    idx = vertex_src.long()
    out = (vertices.index_select(0, idx), faces_out, None if colors is None else colors.index_select(0, idx))
    return out + (vertex_src, face_src) if return_index else out


def clean_mesh_torch(vertices, faces, colors=None, *, min_faces=1, keep_largest=None, return_index=False):
    """clean_mesh as torch ops: face_components_torch, then nonzero / cumsum compaction.  The same integers as the kernels."""
    V, F = _check_mesh("clean_mesh_torch", vertices, faces, colors, min_faces, keep_largest)
    labels, sizes = face_components_torch(faces, V)
    thr = _threshold(sizes, min_faces, keep_largest)
    valid = labels >= 0
    keep = valid & (sizes[labels.clamp(min=0).long()] >= thr) if V else valid
    face_src = keep.nonzero()[:, 0]
    kept = faces[face_src].long()
    used = torch.zeros(V, dtype=torch.bool, device=faces.device)
    used[kept.reshape(-1)] = True
    vertex_src = used.nonzero()[:, 0]
    remap = torch.cumsum(used, 0) - 1
    faces_out = remap[kept].to(torch.int32).reshape(-1, 3)
    return _gather(vertices, colors, vertex_src.to(torch.int32), face_src.to(torch.int32), faces_out, return_index)


def clean_mesh(vertices, faces, colors=None, *, min_faces=1, keep_largest=None, return_index=False, native=None):
    """-> (vertices' [V',3], faces' [F',3] int32, colors' [V',3] or None) - with return_index=True also (vertex_src [V'] int32, face_src
    [F'] int32), the old index of every kept row, ascending.  Faces of components smaller than threshold = max(min_faces, the size of
    the keep_largest-th largest component) are dropped (ties at the threshold are all kept), then invalid faces and the vertices no
    kept face names; with the defaults only the last two.  vertices' = vertices[vertex_src] and colors' likewise, bit for bit.
    On the caller's current stream and the tensors' device; the threshold is chosen on the device, and the one host synchronisation
    is the readback of the two totals that size the outputs.  RuntimeError when the union-find gave up at a loop bound."""
    V, F = _check_mesh("clean_mesh", vertices, faces, colors, min_faces, keep_largest)
    if not _use_native(native, faces, "clean_mesh"):
        return clean_mesh_torch(vertices, faces, colors, min_faces=min_faces, keep_largest=keep_largest, return_index=return_index)
    from . import _native
    with torch.cuda.device(faces.device):
        labels, sizes, ws, nbytes = _native.mesh_components(faces, V)
        thr = _threshold(sizes, min_faces, keep_largest)
        vertex_src, face_src, faces_out = _native.mesh_clean(faces, V, labels, sizes, thr, ws, nbytes)
        return _gather(vertices, colors, vertex_src, face_src, faces_out, return_index)
