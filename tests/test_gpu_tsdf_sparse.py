"""The sparse TSDF volume on the GPU (csrc/gsr_tsdf.hip through diff_gaussian_rasterization/tsdf.py SparseTSDFVolume)
against the device's own dense volume, bit for bit: two passes over three posed frames into a 40 x 33 x 37 volume (5 x 5 x 5 bricks, no
dimension a multiple of 8); a volume near 200^3 whose bricks outnumber one round of k_sn_scan, from a small pool that has to grow;
streaming, where the slots a frame allocated hold the frames from that one on; the device's marks under the sandwich and the superset
property of tests/tsdf_sparse_ref.py, on every fixture of the CPU test; the same frames allocated in another order; the conservative
brick cull under a camera that sees a third of the volume; scene.mesh.extract_mesh(sparse=True) against sparse=False.  Every test
prints the figures it judged."""
import numpy as np
import pytest
import torch

import tsdf_ref as TR
import tsdf_sparse_ref as SR
from test_tsdf_sparse_ref import TWIN_GRID, allocate, allocated_voxels, bits, dense_volume, integrate, sparse_volume

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FIXTURES = sorted(SR.fixtures())


def dense_key(cells, dims):
    return (cells[:, 2].long() * dims[1] + cells[:, 1].long()) * dims[0] + cells[:, 0].long()


def sorted_rows(f):
    f = f.long().cpu().numpy()
    return f[np.lexsort(f.T[::-1])] if len(f) else f


def assert_mesh_equals_dense(sparse_mesh, dense_mesh, dims, what):
    """sparse_mesh = (v, f, c, cells) of SparseTSDFVolume.extract_mesh(return_cells=True); dense_mesh = TSDFVolume.extract_mesh()'s, whose
    vertices come in ascending dense cell index."""
    v, f, c, cells = sparse_mesh
    dv, df, dc = dense_mesh
    print(f"{what}: {v.shape[0]} vertices, {f.shape[0]} faces (the dense volume's: {dv.shape[0]}, {df.shape[0]})")
    assert v.shape == dv.shape and f.shape == df.shape and c.shape == dc.shape and dv.shape[0] > 0 and df.shape[0] > 0
    assert f.dtype == torch.int32 and cells.dtype == torch.int32 and v.dtype == torch.float32
    key = dense_key(cells, dims)
    order = torch.argsort(key)
    assert bool((key[order][1:] > key[order][:-1]).all()), "two vertices share a cell"
    assert torch.equal(bits(v[order]), bits(dv)) and torch.equal(bits(c[order]), bits(dc)), f"{what}: a vertex or a colour differs in a bit"
    inv = torch.empty_like(order)
    inv[order] = torch.arange(order.numel(), device=order.device)
    assert np.array_equal(sorted_rows(inv[f.long()]), sorted_rows(df)), f"{what}: the faces differ as a set of rows"


def assert_allocated_bits_equal(vol, dense, what):
    m, back = allocated_voxels(vol), vol.to_dense()
    print(f"{what}: {vol.num_bricks} of {vol.brick_table.numel()} bricks, {int(m.sum())} of {m.numel()} voxels allocated")
    for name in ("tsdf", "weight"):
        assert torch.equal(bits(getattr(dense, name)[m]), bits(getattr(back, name)[m])), f"{what}: {name} differs in an allocated brick"
    assert torch.equal(bits(dense.color[:, m]), bits(back.color[:, m])), f"{what}: color differs in an allocated brick"
    return m


def beyond_dims_is_zero(vol):
    nx, ny, nz = vol.dims
    nbx, nby, nbz = vol.brick_dims
    c = vol.brick_coords.long()
    pool = torch.zeros(nbz, 8, nby, 8, nbx, 8, device=vol.tsdf.device)
    pool[c[:, 2], :, c[:, 1], :, c[:, 0], :] = vol.weight.abs() + vol.tsdf.abs() + vol.color.abs().sum(1)
    inside = torch.zeros(nbz * 8, nby * 8, nbx * 8, dtype=torch.bool, device=vol.tsdf.device)
    inside[:nz, :ny, :nx] = True
    return not bool(pool.view(nbz * 8, nby * 8, nbx * 8)[~inside].any())


# ---- two passes -----------------------------------------------------------------------------------------------------------------
def test_two_pass_equality_at_the_smallest_shape():
    frames = TR.make_frames(48, 40)
    dense, vol = dense_volume(TWIN_GRID, DEV), sparse_volume(TWIN_GRID, DEV)
    for fr in frames:
        allocate(vol, fr, native=True)
    for fr in frames:
        integrate(dense, fr, native=True)
        integrate(vol, fr, native=True)
    assert vol.brick_dims == (5, 5, 5) and 0 < vol.num_bricks < 125
    assert vol.tsdf.shape == (vol.num_bricks, 8, 8, 8) and vol.color.shape == (vol.num_bricks, 3, 8, 8, 8)
    c = vol.brick_coords.long()
    assert torch.equal(vol.brick_table[c[:, 2], c[:, 1], c[:, 0]], torch.arange(vol.num_bricks, dtype=torch.int32, device=DEV))
    assert int((vol.brick_table >= 0).sum()) == vol.num_bricks and not bool(vol._marks.any())
    m = assert_allocated_bits_equal(vol, dense, "two passes, 40 x 33 x 37")
    assert int((dense.weight[m] > 0).sum()) > 1000 and beyond_dims_is_zero(vol)
    twin = sparse_volume(TWIN_GRID)                                             # the torch twin allocates the same bricks here or a few more or less
    for fr in frames:
        allocate(twin, fr)
    print(f"bricks: kernel {vol.num_bricks}, twin {twin.num_bricks}")
    for min_weight in (1.0, 2.0):
        assert_mesh_equals_dense(vol.extract_mesh(min_weight, return_cells=True, native=True), dense.extract_mesh(min_weight, native=True), TWIN_GRID.dims,
                                 f"two passes min_weight {min_weight}")
    again = vol.extract_mesh(return_cells=True, native=True)
    assert all(torch.equal(a, b) for a, b in zip(again, vol.extract_mesh(return_cells=True, native=True))), "two extractions of one volume differ"
    from diff_gaussian_rasterization.tsdf import brick_order_key
    key = brick_order_key(again[3], TWIN_GRID.dims)
    assert bool((key[1:] > key[:-1]).all()), "the vertices are not in ascending (brick, local voxel) order"
    host = vol.extract_mesh(return_cells=True, native=False)                    # the twin on the same device volume: the same order and integers
    assert torch.equal(again[1], host[1]) and torch.equal(again[3], host[3]) and float((again[0] - host[0]).abs().max()) <= 1e-5


BIG_GRID = TR.Grid((200, 197, 203), (-1.0, -0.985, -1.015), 0.01, 0.12)


def test_past_round_0_of_the_scan_from_a_pool_that_grows():
    """k_sn_scan takes 8 192 blocks of 256 voxels a round, that is 4 096 bricks: a sphere of 90 voxels radius under sdf_trunc = 12 voxels
    needs more (5 144 by the binary32 twin), so the bricks of rank 4 096 and above own vertices placed by the carry between rounds."""
    frames = [TR.sphere_frame(TR.look_at(c, (0, 0, 0)), 96, 80, radius=0.9, holes=False) for c in ((3.2, 0.3, 0.2), (-3.2, -0.3, -0.2))]
    dense, vol = dense_volume(BIG_GRID, DEV), sparse_volume(BIG_GRID, DEV, capacity=64)
    counts = []
    for fr in frames:
        allocate(vol, fr, native=True)
        counts.append(vol.num_bricks)                                           # a commit per frame: the second grows a pool that holds bricks
    assert vol.capacity >= vol.num_bricks > 4096 and vol.growths >= 2 and 64 < counts[0] < counts[1]
    c = vol.brick_coords.long()
    assert torch.equal(vol.brick_table[c[:, 2], c[:, 1], c[:, 0]], torch.arange(vol.num_bricks, dtype=torch.int32, device=DEV))
    for fr in frames:
        integrate(dense, fr, native=True)
        integrate(vol, fr, native=True)
    print(f"bricks after each frame {counts}, capacity {vol.capacity}, growths {vol.growths}; pool {vol.num_bricks * 512 * 20 / 2 ** 20:.0f} MiB, "
          f"dense {BIG_GRID.n * 20 / 2 ** 20:.0f} MiB")
    assert_allocated_bits_equal(vol, dense, "near 200^3")
    got = vol.extract_mesh(return_cells=True, native=True)
    assert_mesh_equals_dense(got, dense.extract_mesh(native=True), BIG_GRID.dims, "near 200^3")
    from diff_gaussian_rasterization.tsdf import brick_order_key
    rank = torch.div(brick_order_key(got[3], BIG_GRID.dims), 512, rounding_mode="floor")
    live = torch.sort(torch.unique(rank)).values                                # brick linear indices that own vertices
    all_live = (vol.brick_table.view(-1) >= 0).nonzero()[:, 0]
    ranks = torch.searchsorted(all_live, live)
    print(f"{int((ranks >= 4096).sum())} bricks of rank 4096 and above own vertices")
    assert int((ranks >= 4096).sum()) > 100


# ---- streaming ------------------------------------------------------------------------------------------------------------------
def test_streaming_holds_the_frames_from_a_bricks_allocation_on():
    frames = SR.streaming_frames()
    vol = sparse_volume(TWIN_GRID, DEV)
    first = []
    for fr in frames:
        before = vol.num_bricks
        allocate(vol, fr, native=True)
        integrate(vol, fr, native=True)
        first.append((before, vol.num_bricks))
    print("slots allocated per frame:", first)
    assert all(b > a for a, b in first)
    for k, (a, b) in enumerate(first):
        dense = dense_volume(TWIN_GRID, DEV)
        for fr in frames[k:]:
            integrate(dense, fr, native=True)
        c = vol.brick_coords[a:b].long()
        for name in ("tsdf", "weight", "color"):
            padded = torch.zeros((3,) * (name == "color") + (40, 40, 40), device=DEV)
            padded[..., :37, :33, :40] = getattr(dense, name)
            want = padded.view((3,) * (name == "color") + (5, 8, 5, 8, 5, 8))                  # (indices apart from each other: their dimension comes first)
            want = want[:, c[:, 2], :, c[:, 1], :, c[:, 0], :] if name == "color" else want[c[:, 2], :, c[:, 1], :, c[:, 0], :]
            assert want.shape == getattr(vol, name)[a:b].shape and torch.equal(bits(want), bits(getattr(vol, name)[a:b])), (k, name)
    full = dense_volume(TWIN_GRID, DEV)
    for fr in frames:
        integrate(full, fr, native=True)
    m = allocated_voxels(vol)
    lost = int((vol.to_dense().weight[m] != full.weight[m]).sum())
    print(f"{lost} voxels of allocated bricks differ from the two-pass volume")
    assert lost > 0, "streaming and two passes agree everywhere: the fixture cannot tell the rule"


# ---- marks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_device_marks_pass_the_sandwich_and_the_superset_property(name):
    grid, frames = SR.fixtures()[name]
    for k, fr in enumerate(frames):
        vol = sparse_volume(grid, DEV)
        allocate(vol, fr, native=True)
        marked = vol._marks.cpu().numpy() != 0
        SR.check_marks(marked, grid, fr, f"kernel {name} frame {k}")
        assert vol.num_bricks == int(marked.sum()) and not bool(vol._marks.any())
        assert np.array_equal(vol.brick_table.cpu().numpy() >= 0, marked)
        lin = np.flatnonzero(marked.reshape(-1))                                # slots in ascending brick linear index
        assert np.array_equal(vol.brick_table.cpu().numpy().reshape(-1)[lin], np.arange(len(lin)))
        nbx, nby, _ = vol.brick_dims
        assert np.array_equal(vol.brick_coords.cpu().numpy(), np.stack([lin % nbx, lin // nbx % nby, lin // (nbx * nby)], 1))


# ---- order independence ---------------------------------------------------------------------------------------------------------
def test_allocation_order_changes_the_slots_and_nothing_else():
    frames = TR.make_frames(48, 40)
    vols = []
    for order in ((0, 1, 2), (2, 1, 0)):
        vol = sparse_volume(TWIN_GRID, DEV, capacity=4)
        for k in order:
            allocate(vol, frames[k], native=True)
            vol.commit()
        for fr in frames:
            integrate(vol, fr, native=True)
        vols.append(vol)
    a, b = vols
    assert a.growths >= 2 and a.num_bricks == b.num_bricks
    assert not torch.equal(a.brick_table, b.brick_table) and torch.equal(a.brick_table >= 0, b.brick_table >= 0)
    da, db = a.to_dense(), b.to_dense()
    assert all(torch.equal(bits(getattr(da, n)), bits(getattr(db, n))) for n in ("tsdf", "weight", "color"))
    ma, mb = a.extract_mesh(return_cells=True, native=True), b.extract_mesh(return_cells=True, native=True)
    assert ma[0].shape[0] > 0 and ma[1].shape[0] > 0 and all(torch.equal(x, y) for x, y in zip(ma, mb))      # not canonicalised: the order itself


# ---- the brick cull -------------------------------------------------------------------------------------------------------------
def test_the_conservative_brick_cull_changes_no_bit():
    """A volume in use (random means and counts) under a narrow camera inside it.  Against the dense kernel on the same state every
    allocated voxel agrees, so no brick was culled that held a voxel to update; and the bricks whose 512 voxel centres all lie behind
    the camera or outside the image by the binary64 projection keep every bit, and are a good part of the allocated bricks."""
    frames = TR.make_frames(48, 40)
    vol = sparse_volume(TWIN_GRID, DEV)
    for fr in frames:
        allocate(vol, fr, native=True)
    B = vol.num_bricks
    g = torch.Generator().manual_seed(11)
    vol.tsdf.copy_(torch.rand(vol.tsdf.shape, generator=g) * 2 - 1)
    vol.weight.copy_(torch.randint(0, 3, vol.weight.shape, generator=g).float())
    vol.color.copy_(torch.rand(vol.color.shape, generator=g))
    start = [bits(t).clone() for t in (vol.tsdf, vol.weight, vol.color)]
    dense = vol.to_dense()
    narrow = TR.sphere_frame(TR.look_at((0.1, 0.05, 0.0), (1.0, 0.2, 0.3)), 40, 32, holes=False, tanfov=(0.45, 0.4))
    integrate(dense, narrow, native=True)
    integrate(vol, narrow, native=True)
    m = allocated_voxels(vol)
    back = vol.to_dense()
    for name in ("tsdf", "weight", "color"):
        mm = m if name != "color" else m[None].expand(3, -1, -1, -1)
        assert torch.equal(bits(getattr(dense, name))[mm], bits(getattr(back, name))[mm]), f"{name} differs from the dense kernel"
    c = vol.brick_coords.cpu().numpy().astype(np.int64)
    l = np.arange(512)
    ijk = np.stack([8 * c[:, None, 0] + (l & 7), 8 * c[:, None, 1] + ((l >> 3) & 7), 8 * c[:, None, 2] + (l >> 6)], -1).astype(np.float64)    # [B,512,3]
    pv = (TWIN_GRID.origin.astype(np.float64) + float(TWIN_GRID.voxel) * ijk) @ narrow.V[:3, :3].astype(np.float64) + narrow.V[3, :3].astype(np.float64)
    z = pv[..., 2]
    zs = np.where(z > 1e-6, z, 1.0)
    u = narrow.W / (2 * narrow.tanfovx) * pv[..., 0] / zs + narrow.W / 2
    v = narrow.H / (2 * narrow.tanfovy) * pv[..., 1] / zs + narrow.H / 2
    eps = 1e-3
    out = (z <= 1e-6) | (u < -eps) | (u > narrow.W + eps) | (v < -eps) | (v > narrow.H + eps)
    outside = torch.as_tensor(out.all(1))
    changed = torch.stack([(bits(t) != s).reshape(B, -1).any(1).cpu() for t, s in zip((vol.tsdf, vol.weight, vol.color), start)]).any(0)
    print(f"{int(outside.sum())} of {B} bricks lie outside the narrow frustum; {int(changed.sum())} bricks changed")
    assert B // 4 <= int(outside.sum()) < B and int(changed.sum()) > 0
    assert not bool((changed & outside).any()), "a brick outside the frustum changed"


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def canonical_mesh(mesh):
    """(vertices, faces, colors) -> vertices and colours as rows in lexicographic order of their bits, faces re-indexed and sorted."""
    v, f, c = (t.detach().cpu() for t in mesh)
    rows = torch.cat([bits(v), bits(c)], 1).numpy().astype(np.int64)
    order = np.lexsort(rows.T[::-1])
    assert len(np.unique(rows[:, :3], axis=0)) == len(rows), "two vertices share a position"
    inv = np.empty(len(order), np.int64)
    inv[order] = np.arange(len(order))
    return rows[order], sorted_rows(torch.as_tensor(inv[f.long().numpy()]))


@pytest.mark.parametrize("keep_largest", [None, 1])
def test_scene_extract_mesh_sparse_equals_dense(keep_largest):
    from gaussian_params import Pipe
    from scene import GaussianModel
    from test_gpu_tsdf import BOUNDS, _ring_cameras, _shell_scene
    gm = GaussianModel(0)
    gm.adopt_scene(_shell_scene(1500), device=DEV)
    cams, bg = _ring_cameras(4), torch.zeros(3, device=DEV)
    kw = dict(bounds=BOUNDS, resolution=64, keep_largest=keep_largest)
    want = gm.extract_mesh(cams, Pipe(), bg, sparse=False, **kw)
    got = gm.extract_mesh(cams, Pipe(), bg, sparse=True, **kw)
    old = gm.extract_mesh(cams, Pipe(), bg, bounds=BOUNDS, voxel_size=2.0 / 64, keep_largest=keep_largest)     # the call of before the keywords
    print(f"keep_largest {keep_largest}: {got[0].shape[0]} vertices, {got[1].shape[0]} faces (dense: {want[0].shape[0]}, {want[1].shape[0]})")
    assert want[0].shape[0] > 100 and want[1].shape[0] > 100 and got[1].dtype == torch.int32
    assert all(torch.equal(a, b) for a, b in zip(want, old))
    (gv, gf), (wv, wf) = canonical_mesh(got), canonical_mesh(want)
    assert np.array_equal(gv, wv) and np.array_equal(gf, wf)
    if keep_largest is None:                                                    # streaming runs, and is a mesh too
        v, f, c = gm.extract_mesh(cams, Pipe(), bg, sparse=True, two_pass=False, **kw)
        assert v.shape[0] > 100 and f.shape[0] > 100 and int(f.max()) < v.shape[0] and bool(torch.isfinite(v).all())
