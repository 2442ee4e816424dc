"""The mesh-cleaning kernels on the GPU (csrc/gsr_mesh.hip through diff_gaussian_rasterization/meshops.py) against the
independent reference of tests/mesh_ref.py, exactly: every shared case - empty meshes, one triangle, a path of 5 000 triangles over a
random permutation, a star whose 4 096 faces contend for one root, 1 000 islands and a sheet, sheets that touch in one point, invalid
and duplicate faces, unreferenced vertices - and every threshold case, labels and sizes, the three outputs and the two index arrays,
attribute rows bit for bit (random bits, NaN payloads among them); the same call twice gives the same integers.  End to end: an
analytic volume of two spheres, extracted and cleaned, equals the extraction of the big sphere alone; a shell of Gaussians from eight
cameras through scene.mesh.extract_mesh(keep_largest=1) is one component and its PLY file reads back.  Past the first round of
k_mesh_scan (every case above stays inside it: 33 blocks at most): a mesh of 4 505 500 faces over 4 751 825 vertices - sheets, two of
them equal, a million isolated triangles, invalid and duplicate faces, unreferenced vertices - whose reference is known by
construction, three rounds of the face scan and of the vertex scan, at five thresholds; and the three-round volume of
tests/tsdf_ref.py, extracted and cleaned, equals the extraction of its plane alone.  The references are computed once (tests/mesh_ref.py's
caches) and shared."""
import numpy as np
import pytest
import torch

import mesh_ref as MR
import streams as ST
import tsdf_ref as TR
from test_mesh_clean_ref import CASE_THRESHOLDS, big_conditions, big_tensors, case_tensors, check_clean, check_components
from test_tsdf_ref import three_round_conditions, volume_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("name", list(MR.cases()))
def test_components_against_the_reference_and_twice_the_same(name):
    from diff_gaussian_rasterization.meshops import face_components
    V, f = MR.cases()[name]
    faces = torch.as_tensor(f).to(DEV)
    got = face_components(faces, V, native=True)
    check_components(got, MR.reference(name), f"kernel {name}")
    again = face_components(faces, V, native=True)
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two runs on one mesh differ"


@pytest.mark.parametrize("name, min_faces, keep_largest", CASE_THRESHOLDS)
def test_clean_against_the_reference_and_twice_the_same(name, min_faces, keep_largest):
    from diff_gaussian_rasterization.meshops import clean_mesh
    v, f, c = case_tensors(name, DEV)
    ref = MR.reference(name, min_faces, keep_largest)
    got = clean_mesh(v, f, c, min_faces=min_faces, keep_largest=keep_largest, return_index=True, native=True)
    check_clean(got, ref, v, c, f"kernel {name} min_faces {min_faces} keep_largest {keep_largest}")
    again = clean_mesh(v, f, c, min_faces=min_faces, keep_largest=keep_largest, return_index=True)      # device tensors take the kernels
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two runs on one mesh differ"
    three = clean_mesh(v, f, None, min_faces=min_faces, keep_largest=keep_largest, native=True)
    assert len(three) == 3 and three[2] is None and np.array_equal(three[1].cpu().numpy(), ref["faces_out"])


# ---- past the first round of k_mesh_scan ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big():
    """MR.big_mesh(1.0) with attribute rows of random bits on the device, uploaded once (about 170 MB)."""
    return big_tensors(1.0, DEV)


def test_components_of_the_big_mesh_against_the_reference_and_twice_the_same(big):
    from diff_gaussian_rasterization.meshops import face_components
    info = MR.big_info(1.0)
    V, faces = info["V"], big[1]
    print(f"big mesh: V = {V}, F = {faces.shape[0]}, {int((info['sizes'] > 0).sum())} components, the largest of {int(info['sizes'].max())} faces")
    got = face_components(faces, V, native=True)
    check_components(got, info, "kernel big mesh")
    again = face_components(faces, V, native=True)
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two runs on one mesh differ"


@pytest.mark.parametrize("min_faces, keep_largest", MR.BIG_THRESHOLDS)
def test_clean_past_the_first_round_of_the_face_scan_and_of_the_vertex_scan(big, min_faces, keep_largest):
    """4 505 500 faces are 17 600 blocks and 4 751 825 vertices 18 562: three rounds of each call of mesh_scan_counts.  The rows that
    faces and vertices of rounds 1 and 2 go to are placed by the carry between rounds."""
    from diff_gaussian_rasterization.meshops import clean_mesh
    ref = big_conditions(1.0, min_faces, keep_largest, "kernel")
    v, f, c = big
    got = clean_mesh(v, f, c, min_faces=min_faces, keep_largest=keep_largest, return_index=True, native=True)
    print(f"big mesh min_faces {min_faces} keep_largest {keep_largest}: kept V = {got[0].shape[0]} of {v.shape[0]}, F = {got[1].shape[0]} of {f.shape[0]}")
    check_clean(got, ref, v, c, f"kernel big mesh min_faces {min_faces} keep_largest {keep_largest}")
    again = clean_mesh(v, f, c, min_faces=min_faces, keep_largest=keep_largest, return_index=True, native=True)
    assert all(torch.equal(a, b) for a, b in zip(got[1:2] + got[3:], again[1:2] + again[3:])), "two runs on one mesh differ"
    assert ST.same_bits(got[0], again[0]) and ST.same_bits(got[2], again[2])


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_the_three_round_volume_cleaned_equals_the_plane_alone():
    """test_two_spheres_cleaned_equal_the_big_sphere_alone past the first round of k_sn_scan: the volume of tests/tsdf_ref.py's
    three_round_volume holds a plane with a hole and a sphere; without the sphere every vertex and face of the plane is the same."""
    from diff_gaussian_rasterization.meshops import clean_mesh, face_components
    grid, ref = three_round_conditions(1.0, "kernel")
    both = volume_of(*TR.three_round_volume(), DEV).extract_mesh(native=True)
    alone = volume_of(*TR.three_round_volume(small=False), DEV).extract_mesh(native=True)
    f_plane, f_small = alone[1].shape[0], both[1].shape[0] - alone[1].shape[0]
    print(f"plane and sphere: V = {both[0].shape[0]}, F = {both[1].shape[0]}; the plane alone: V = {alone[0].shape[0]}, F = {f_plane}")
    assert 0 < f_small < f_plane and both[0].shape[0] > alone[0].shape[0] and both[1].shape[0] == len(ref["faces"])
    _, sizes = face_components(both[1], both[0].shape[0], native=True)
    assert sorted(sizes[sizes > 0].tolist()) == [f_small, f_plane]              # two surfaces, no cell in common; the hole splits nothing
    got = clean_mesh(*both, keep_largest=1, native=True)
    assert ST.same_bits(got[0].cpu(), alone[0].cpu()), "vertices differ from the plane's"
    assert torch.equal(got[1].cpu(), alone[1].cpu()), "faces differ from the plane's"
    assert ST.same_bits(got[2].cpu(), alone[2].cpu()), "colours differ from the plane's"
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(clean_mesh(*both, keep_largest=2, native=True), both))


N_E2E, BIG, SMALL = 48, ((16.0, 24.0, 24.0), 8.0), ((40.0, 24.0, 23.0), 2.0)      # centres and radii in voxels: 14 voxels of air between them


def _spheres(which):
    """An analytic volume of 48^3 voxels (voxel size 1, weight 1) that holds the spheres `which`; the colour is a function of the place."""
    grid = TR.Grid((N_E2E,) * 3, (0.0, 0.0, 0.0), 1.0, 3.0)
    ix, iy, iz = grid.coords()
    p = np.stack([ix, iy, iz], 1).astype(np.float64)
    sdf = np.min([np.linalg.norm(p - np.asarray(c)[None], axis=1) - r for c, r in which], 0)
    tsdf = np.clip(sdf / 3.0, -1, 1).astype(np.float32).reshape((N_E2E,) * 3)
    color = (p.T / N_E2E).astype(np.float32).reshape(3, N_E2E, N_E2E, N_E2E)
    return volume_of(grid, tsdf, np.ones((N_E2E,) * 3, np.float32), color, DEV)


def test_two_spheres_cleaned_equal_the_big_sphere_alone():
    from diff_gaussian_rasterization.meshops import clean_mesh, face_components
    both, big = _spheres((BIG, SMALL)).extract_mesh(native=True), _spheres((BIG,)).extract_mesh(native=True)
    f_big, f_small = big[1].shape[0], both[1].shape[0] - big[1].shape[0]
    print(f"both spheres: V = {both[0].shape[0]}, F = {both[1].shape[0]}; the big one alone: V = {big[0].shape[0]}, F = {f_big}")
    assert 0 < f_small < f_big and both[0].shape[0] > big[0].shape[0]
    labels, sizes = face_components(both[1], both[0].shape[0], native=True)
    assert sorted(sizes[sizes > 0].tolist()) == [f_small, f_big]                # two closed surfaces, no cell in common
    for kw in (dict(min_faces=(f_small + f_big) // 2), dict(min_faces=f_small + 1), dict(min_faces=f_big), dict(keep_largest=1)):
        got = clean_mesh(*both, native=True, **kw)
        assert ST.same_bits(got[0].cpu(), big[0].cpu()), f"{kw}: vertices differ from the big sphere's"
        assert torch.equal(got[1].cpu(), big[1].cpu()), f"{kw}: faces differ from the big sphere's"
        assert ST.same_bits(got[2].cpu(), big[2].cpu()), f"{kw}: colours differ from the big sphere's"
    for kw in (dict(min_faces=f_small), dict(keep_largest=2), dict()):          # at the small sphere's size: everything stays
        got = clean_mesh(*both, native=True, **kw)
        assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, both)), kw
    assert clean_mesh(*both, min_faces=f_big + 1, native=True)[1].shape == (0, 3)


def test_extract_mesh_keep_largest_from_gaussians_to_a_ply_file(tmp_path):
    from gaussian_params import Pipe
    from scene import GaussianModel
    from scene.mesh import load_mesh_ply, save_mesh_ply
    from test_gpu_tsdf import BOUNDS, _ring_cameras, _shell_scene
    gm = GaussianModel(0)
    gm.adopt_scene(_shell_scene(), device=DEV)
    cams, bg = _ring_cameras(), torch.zeros(3, device=DEV)
    kw = dict(bounds=BOUNDS, voxel_size=2.0 / 48)
    raw = gm.extract_mesh(cams, Pipe(), bg, **kw)
    got = gm.extract_mesh(cams, Pipe(), bg, keep_largest=1, **kw)
    v, f, c = (t.cpu().numpy() for t in got)
    ref = MR.clean_ref(raw[1].cpu().numpy(), raw[0].shape[0], keep_largest=1)
    pieces = int((ref["sizes"] > 0).sum())
    print(f"extracted: V = {raw[0].shape[0]}, F = {raw[1].shape[0]} in {pieces} components; the largest: V = {len(v)}, F = {len(f)}")
    assert len(f) > 0 and f.dtype == np.int32 and f.min() >= 0 and f.max() < len(v) and v.shape == c.shape
    assert np.array_equal(f, ref["faces_out"])
    idx = torch.from_numpy(ref["vertex_src"].astype(np.int64))
    assert ST.same_bits(got[0].cpu(), raw[0].cpu()[idx]) and ST.same_bits(got[2].cpu(), raw[2].cpu()[idx])
    _, sizes = MR.components_ref(f, len(v))
    assert int((sizes > 0).sum()) == 1 and int(sizes.max()) == len(f) == int(ref["sizes"].max())
    assert np.unique(f).size == len(v)                                           # no vertex is left that nobody uses
    path = str(tmp_path / "clean.ply")
    save_mesh_ply(path, *got)
    v2, f2, c2 = load_mesh_ply(path)
    assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)
    assert np.array_equal(c2, np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    same = gm.extract_mesh(cams, Pipe(), bg, min_component_faces=None, keep_largest=None, **kw)
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(same, raw))
