"""An independent reference of mesh cleaning (diff_gaussian_rasterization/meshops.py, csrc/gsr_mesh.hip): a plain
sequential numpy union-find with path halving and the rule, and the shared cases - the smallest shapes at which the kernels can go
wrong - generated with fixed seeds.  Used by tests/test_mesh_clean_ref.py (twins, host program) and tests/test_gpu_mesh_clean.py.

The rule.  A face is valid when its three indices lie in [0, V) and are pairwise different; two valid faces are connected when they
share a vertex; a component's label is the smallest vertex index it contains (labels: -1 for an invalid face); sizes[label] is its
number of faces; threshold = max(min_faces, size of the keep_largest-th largest component, where there is one); a face is kept when it
is valid and sizes[label] >= threshold; a vertex is kept when a kept face names it; order is kept, faces are re-indexed."""
import functools

import numpy as np


def face_valid(faces, V):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return ((f >= 0) & (f < V)).all(1) & (f[:, 0] != f[:, 1]) & (f[:, 0] != f[:, 2]) & (f[:, 1] != f[:, 2])


def components_ref(faces, V):
    """-> (labels [F] int32, sizes [V] int32): sequential union-find, union by smaller index, path halving."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    valid = face_valid(f, V)
    parent = list(range(V))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b, c in f[valid].tolist():
        for u, w in ((a, b), (a, c)):
            ru, rw = find(u), find(w)
            if ru != rw:
                parent[max(ru, rw)] = min(ru, rw)
    labels = np.full(f.shape[0], -1, np.int32)
    sizes = np.zeros(V, np.int32)
    for i in np.nonzero(valid)[0].tolist():
        r = find(int(f[i, 0]))
        labels[i] = r
        sizes[r] += 1
    return labels, sizes


def threshold_ref(sizes, min_faces=1, keep_largest=None):
    comp = np.sort(sizes[sizes > 0])[::-1]
    if keep_largest is not None and len(comp) >= keep_largest:
        return max(int(min_faces), int(comp[keep_largest - 1]))
    return int(min_faces)


def clean_ref(faces, V, min_faces=1, keep_largest=None, components=None):
    """-> dict(labels, sizes, threshold, vertex_src, face_src, faces_out), the last three int32.  components: components_ref's, if at hand."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    labels, sizes = components_ref(f, V) if components is None else components
    thr = threshold_ref(sizes, min_faces, keep_largest)
    keep = np.zeros(f.shape[0], bool)
    for i in range(f.shape[0]):
        keep[i] = labels[i] >= 0 and sizes[labels[i]] >= thr
    face_src = np.nonzero(keep)[0]
    used = np.zeros(V, bool)
    for i in face_src.tolist():
        used[f[i]] = True
    vertex_src = np.nonzero(used)[0]
    new = np.full(V, -1, np.int64)
    new[vertex_src] = np.arange(len(vertex_src))
    faces_out = new[f[face_src]].reshape(-1, 3)
    return dict(labels=labels, sizes=sizes, threshold=thr, vertex_src=vertex_src.astype(np.int32), face_src=face_src.astype(np.int32),
                faces_out=faces_out.astype(np.int32))


# ---- the shared cases ------------------------------------------------------------------------------------------------------------
def sheet(nx, ny, base=0):
    """A grid of nx x ny quads as 2 nx ny triangles over (nx + 1)(ny + 1) vertices from `base`."""
    idx = lambda i, j: base + j * (nx + 1) + i
    out = []
    for j in range(ny):
        for i in range(nx):
            out += [(idx(i, j), idx(i + 1, j), idx(i + 1, j + 1)), (idx(i, j), idx(i + 1, j + 1), idx(i, j + 1))]
    return out, (nx + 1) * (ny + 1)


def _shuffled(faces, V, rng, shuffle_faces=True):
    perm = rng.permutation(V)
    f = perm[np.asarray(faces, np.int64)]
    if shuffle_faces:
        f = f[rng.permutation(len(f))]
    return f.astype(np.int32)


def _path():
    rng = np.random.default_rng(11)
    p = rng.permutation(5002)
    return 5002, np.stack([p[:-2], p[1:-1], p[2:]], 1).astype(np.int32)


def _star():
    """Every face names V - 1, and the faces come with k descending: every link lowers the root above V - 1 and so contends for the
    current root's word in whatever order the lanes run; the smallest index, in the last face, must win."""
    F = 4096
    V = 2 * F + 1
    k = np.arange(F)[::-1]
    return V, np.stack([np.full(F, V - 1), 2 * k, 2 * k + 1], 1).astype(np.int32)


def islands(seed=12):
    """(V, faces): 1 000 isolated triangles and one sheet of 300 faces, vertices and faces shuffled by `seed` (the shapes do not depend on it)."""
    rng = np.random.default_rng(seed)
    faces, n = sheet(15, 10)                                        # 300 faces over 176 vertices
    faces += [(n + 3 * k, n + 3 * k + 1, n + 3 * k + 2) for k in range(1000)]
    V = n + 3000
    return V, _shuffled(faces, V, rng)


def _pinch(duplicated):
    a, na = sheet(3, 3)                                             # 18 faces over vertices 0 .. 15; its last vertex is 15
    b, nb = sheet(3, 3, base=na - 1 if not duplicated else na)      # the second sheet starts AT vertex 15, or at its duplicate 16
    V = (na - 1 if not duplicated else na) + nb
    return V, np.asarray(a + b, np.int32)


def _mixed():
    """Two sheets of 18 faces (a tie), one of 8, three single triangles, duplicates of two faces, every kind of invalid face, and
    unreferenced vertices at the front (0, 1), in the middle and at the end."""
    faces, base = [], 2
    for nx, ny in ((3, 3), (3, 3), (2, 2)):
        s, n = sheet(nx, ny, base)
        faces += s
        base += n + (3 if nx == 3 else 0)                           # a gap of unreferenced vertices behind the sheets of 18
    for _ in range(3):
        faces.append((base, base + 1, base + 2))
        base += 3
    V = base + 4                                                    # four unreferenced vertices at the end
    dup = [faces[36], faces[40]]                                    # two of the sheet of 8 (-> 10 faces; the sheets of 18 stay a tie)
    a, b = faces[5][0], faces[5][1]
    invalid = [(-1, a, b), (a, V, b), (a, a, b), (a, b, a), (b, a, a), (a, b, 2 ** 31 - 1), (-2 ** 31, a, b)]
    rng = np.random.default_rng(13)
    f = np.asarray(faces + dup + invalid, np.int64)
    return V, f[rng.permutation(len(f))].astype(np.int32)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (V, faces [F,3] int32)}"""
    out = {"empty_0_0": (0, np.zeros((0, 3), np.int32)), "empty_5_0": (5, np.zeros((0, 3), np.int32)),
           "no_vertex": (0, np.asarray([[0, 1, 2], [-1, 0, 1]], np.int32)),
           "one_triangle": (5, np.asarray([[3, 1, 2]], np.int32))}
    for name, (V, f) in (("path", _path()), ("star", _star()), ("islands", islands()), ("pinch_shared", _pinch(False)),
                         ("pinch_duplicated", _pinch(True)), ("mixed", _mixed())):
        out[name] = (V, np.ascontiguousarray(f))
    return out


# (min_faces, keep_largest) per case: at, one below and one above a component's size; a tie at the n-th size; more than there are components
THRESHOLDS = {
    "islands": [(1, None), (299, None), (300, None), (301, None), (2, None), (1, 1), (1, 2), (1, 5000), (400, 1)],
    "mixed": [(1, None), (17, None), (18, None), (19, None), (10, None), (11, None), (1, 1), (1, 2), (1, 3), (1, 4), (1, 100), (12, 3)],
    "pinch_shared": [(1, None), (36, None), (37, None), (1, 1)],
    "pinch_duplicated": [(1, None), (18, None), (19, None), (1, 1), (1, 2), (1, 3)],
}
DEFAULT_THRESHOLDS = [(1, None), (2, None), (1, 1), (1, 3)]


def thresholds(name):
    return THRESHOLDS.get(name, DEFAULT_THRESHOLDS)


@functools.lru_cache(maxsize=None)
def _components(name):
    V, f = cases()[name]
    return components_ref(f, V)


def _read_only(ref):
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name, min_faces=1, keep_largest=None):
    """clean_ref of a case, computed once and shared; the arrays are read-only."""
    V, f = cases()[name]
    return _read_only(clean_ref(f, V, min_faces, keep_largest, _components(name)))


# ---- the large mesh: past the first round of the kernels' scans, its reference known by construction --------------------------------
# k_mesh_scan walks the blocks' counts (256 faces or vertices each) in rounds of 8 192 blocks = 2 097 152 elements.  At scale 1 the mesh
# below has F = 4 505 500 and V = 4 751 825: three rounds of the face scan and three of the vertex scan.  The sequential references
# above take minutes at that size, so this one comes from how the mesh is built, in vectorised numpy, and is held to the sequential
# ones at a small scale and to scipy at the full one (tests/test_mesh_clean_ref.py).
BIG_SHEETS = ((900, 900), (700, 600), (500, 500), (500, 500), (120, 100))      # quads; the two equal sheets tie as third largest
BIG_TRIANGLES = 1_000_000                                   # isolated: one face and three vertices each
BIG_INVALID = 3000                                          # of each of _mixed's seven kinds
BIG_DUPLICATES = 500                                        # faces of the smallest sheet that come twice
BIG_UNUSED = (1000, 2000, 1500)                             # unreferenced vertices at the front, in the middle, at the end
BIG_TIE = 3                                                 # keep_largest = 3: the threshold is the equal sheets' size, and both stay
BIG_THRESHOLDS = [(1, None), (2, None), (1, 1), (1, 2), (1, BIG_TIE)]
SMALL_SCALE = 0.001                                         # a few thousand faces: the sequential references' size


def sheet_faces(nx, ny, base=0):
    """sheet() without its loop -> (faces [2 nx ny, 3] int64 in sheet()'s order, the number of vertices)."""
    j, i = np.mgrid[0:ny, 0:nx]
    v = base + j * (nx + 1) + i
    return np.stack([v, v + 1, v + nx + 2, v, v + nx + 2, v + nx + 1], -1).reshape(-1, 3).astype(np.int64), (nx + 1) * (ny + 1)


@functools.lru_cache(maxsize=None)
def _big(scale):
    rng = np.random.default_rng(14)
    k = float(scale) ** 0.5
    dims = [(max(2, round(nx * k)), max(2, round(ny * k))) for nx, ny in BIG_SHEETS]
    n_tri, n_inv, n_dup = max(8, round(BIG_TRIANGLES * scale)), max(2, round(BIG_INVALID * scale)), max(2, round(BIG_DUPLICATES * scale))
    unused = [max(2, round(u * scale)) for u in BIG_UNUSED]
    # the valid faces over local vertex indices: sheet after sheet, then the triangles; `comp` numbers the components in that order
    faces, comp, starts, base = [], [], [], 0
    for c, (nx, ny) in enumerate(dims):
        f, n = sheet_faces(nx, ny, base)
        faces.append(f)
        comp.append(np.full(len(f), c, np.int64))
        starts.append(base)
        base += n
    faces.append(faces[-1][rng.choice(len(faces[-1]), n_dup, replace=False)])               # the duplicates
    comp.append(np.full(n_dup, len(dims) - 1, np.int64))
    tri0 = base + 3 * np.arange(n_tri, dtype=np.int64)
    faces.append(tri0[:, None] + np.arange(3)[None])
    comp.append(len(dims) + np.arange(n_tri, dtype=np.int64))
    starts = np.concatenate([np.asarray(starts, np.int64), tri0])
    R = base + 3 * n_tri                                                                    # referenced vertices
    V = R + sum(unused)
    # where the referenced vertices go: a random permutation over every place that is not kept free
    free = np.zeros(V, bool)
    free[:unused[0]] = True
    free[V // 2:V // 2 + unused[1]] = True
    free[V - unused[2]:] = True
    place = np.nonzero(~free)[0][rng.permutation(R)]
    valid = place[np.concatenate(faces)]
    la = rng.integers(R, size=(7, n_inv))
    a, b = place[la], place[(la + 1 + rng.integers(R - 1, size=(7, n_inv))) % R]              # two different vertices
    kinds = [(np.full(n_inv, -1), a[0], b[0]), (a[1], np.full(n_inv, V), b[1]), (a[2], a[2], b[2]), (a[3], b[3], a[3]), (b[4], a[4], a[4]),
             (a[5], b[5], np.full(n_inv, 2 ** 31 - 1)), (np.full(n_inv, -2 ** 31), a[6], b[6])]
    invalid = np.concatenate([np.stack(kd, 1) for kd in kinds]).astype(np.int64)
    allf = np.concatenate([valid, invalid])
    comp = np.concatenate(comp + [np.full(len(invalid), -1, np.int64)])
    order = rng.permutation(len(allf))
    allf, comp = allf[order], comp[order]
    # by construction: a component's label is the smallest place of its vertices
    smallest = np.minimum.reduceat(place, starts)
    labels = np.where(comp >= 0, smallest[np.maximum(comp, 0)], -1).astype(np.int32)
    sizes = np.bincount(labels[labels >= 0], minlength=V).astype(np.int32)
    faces32 = np.ascontiguousarray(allf.astype(np.int32))
    assert np.array_equal(faces32.astype(np.int64), allf)
    out = dict(V=V, faces=faces32, labels=labels, sizes=sizes, free=free, sheet_faces=[2 * nx * ny for nx, ny in dims], triangles=n_tri,
               invalid=len(invalid), duplicates=n_dup)
    return _read_only(out)


def big_mesh(scale=1.0):
    """(V, faces [F,3] int32): BIG_SHEETS with their sides scaled by sqrt(scale) (two of them equal), BIG_TRIANGLES x scale isolated
    triangles, duplicates of faces of the smallest sheet, every kind of invalid face of _mixed, unreferenced vertices at the front, in
    the middle and at the end; the vertex indices randomly permuted, the faces shuffled.  Fixed seed; computed once; read-only."""
    b = _big(scale)
    return b["V"], b["faces"]


def big_info(scale=1.0):
    """What big_mesh(scale) was built from: dict(V, faces, labels, sizes, free (the vertices kept unreferenced), sheet_faces, triangles,
    invalid, duplicates)."""
    return _big(scale)


def clean_vectorised(faces, V, labels, sizes, min_faces=1, keep_largest=None):
    """clean_ref's rule without its loops, from given components."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    thr = threshold_ref(sizes, min_faces, keep_largest)
    keep = (labels >= 0) & (sizes[np.maximum(labels, 0)] >= thr) if V else np.zeros(len(f), bool)
    face_src = np.nonzero(keep)[0]
    used = np.zeros(V, bool)
    used[f[face_src].reshape(-1)] = True
    vertex_src = np.nonzero(used)[0]
    new = np.cumsum(used) - 1
    return dict(labels=labels, sizes=sizes, threshold=thr, vertex_src=vertex_src.astype(np.int32), face_src=face_src.astype(np.int32),
                faces_out=new[f[face_src]].reshape(-1, 3).astype(np.int32))


@functools.lru_cache(maxsize=None)
def big_reference(scale=1.0, min_faces=1, keep_largest=None):
    """The reference of big_mesh(scale): labels and sizes by construction, the rest by the rule; computed once and shared; read-only."""
    b = _big(scale)
    return _read_only(clean_vectorised(b["faces"], b["V"], b["labels"], b["sizes"], min_faces, keep_largest))
