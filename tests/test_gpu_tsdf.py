"""The TSDF kernels on the GPU (csrc/gsr_tsdf.hip through diff_gaussian_rasterization/tsdf.py) against the binary64
restatement of tests/tsdf_ref.py under its error rule.  Fusion: three frames in sequence (a posed camera outside the volume, one inside
it, holes in alpha, a depth_max that cuts pixels) into volumes of 17 x 9 x 21, 1 x 1 x 1 and 64 x 64 x 64 voxels from maps of 33 x 17
and 96 x 96 pixels; skipped voxels keep every bit of a volume of random bits; the same frames give the same bits twice, and on a side
stream.  Extraction: on the GPU's own fused volume, the faces integer for integer and the vertices and colours within the replayed
bound, for one cell, an odd volume, a volume with block edges along every axis, a volume without an active cell and the analytic
sphere with its topological checks; and past the first round of k_sn_scan (every volume above stays inside it: 1 024 blocks at most), an
analytic volume of 131 x 127 x 300 voxels, three rounds, at two min_weight values.  End to end: Gaussians on a sphere shell, eight cameras, a 48^3 volume, a PLY file.  The references
are computed once (tests/test_tsdf_ref.py's caches) and shared.  Every test prints the figures it judged."""
import math

import numpy as np
import pytest
import torch

import scene_synth as S
import streams as ST
import tsdf_ref as TR
from test_tsdf_ref import (FUSION_CASES, check_mesh, fusion_reference, integrate_frames, make_volume, sphere_checks, sphere_reference,
                           three_round_conditions, volume_arrays, volume_of)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(vol):
    return {k: t.detach().cpu() for k, t in (("tsdf", vol.tsdf), ("weight", vol.weight), ("color", vol.color))}


# ---- fusion -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name, W, H", FUSION_CASES)
def test_fusion_against_the_reference(grid_name, W, H):
    grid, frames, ref = fusion_reference(grid_name, W, H)
    TR.assert_cap(ref, f"{grid_name} {W}x{H}")
    vol = integrate_frames(make_volume(grid, DEV), frames, native=True)
    assert TR.check_volume(*volume_arrays(vol), ref, f"kernel {grid_name} {W}x{H}") <= 1


def test_skipped_voxels_keep_every_bit_and_the_same_frames_give_the_same_bits():
    grid, frames, ref = fusion_reference("64x64x64", 96, 96)
    g = torch.Generator().manual_seed(3)
    start = {k: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, dtype=torch.int64).to(torch.int32)       # random bits: NaNs, infinities
             for k, shape in (("tsdf", (64, 64, 64)), ("weight", (64, 64, 64)), ("color", (3, 64, 64, 64)))}
    runs = []
    for _ in range(2):
        vol = make_volume(grid, DEV)
        for k, t in (("tsdf", vol.tsdf), ("weight", vol.weight), ("color", vol.color)):
            t.view(torch.int32).copy_(start[k])
        runs.append(bits(integrate_frames(vol, frames, native=True)))
    skipped = ((ref["state"].weight == 0) & ~ref["fragile"]).reshape(64, 64, 64)
    print(f"{int(skipped.sum())} of {skipped.numel()} voxels are skipped by every frame")
    assert int(skipped.sum()) > skipped.numel() // 2
    for k in ("tsdf", "weight", "color"):
        m = skipped if k != "color" else skipped[None].expand(3, -1, -1, -1)
        assert torch.equal(runs[0][k].view(torch.int32)[m], start[k][m]), f"a skipped voxel's {k} changed"
        assert ST.same_bits(runs[0][k], runs[1][k]), f"two runs of the same frames differ in {k}"
    changed = runs[0]["weight"].view(torch.int32) != start["weight"]
    assert int((changed & skipped).sum()) == 0 and int(changed.sum()) > 0


def _stream_make(seed, device):
    frames = TR.make_frames(33, 17, seed=seed)
    g = torch.Generator().manual_seed(700 + seed)
    st = {}
    for i, fr in enumerate(frames):
        st.update({f"depth{i}": fr.depth[None], f"alpha{i}": fr.alpha[None], f"color{i}": fr.color, f"V{i}": fr.V})
    n = TR.GRIDS["17x9x21"].dims
    st["tsdf"] = torch.rand(n[2], n[1], n[0], generator=g) * 2 - 1                # a volume in use: earlier frames' means and counts
    st["weight"] = torch.randint(0, 3, (n[2], n[1], n[0]), generator=g).float()
    st["vcolor"] = torch.rand(3, n[2], n[1], n[0], generator=g)
    out = {k: torch.as_tensor(v).to(device).contiguous() for k, v in st.items()}
    out["frames"] = frames
    return out


def _stream_staged(st):
    return [v for v in st.values() if isinstance(v, torch.Tensor)]


def _stream_run(st):
    grid = TR.GRIDS["17x9x21"]
    vol = make_volume(grid, st["tsdf"].device)
    vol.tsdf, vol.weight, vol.color = st["tsdf"], st["weight"], st["vcolor"]
    for i, fr in enumerate(st["frames"]):
        vol.integrate(st[f"depth{i}"], st[f"alpha{i}"], st[f"color{i}"], st[f"V{i}"], fr.tanfovx, fr.tanfovy, alpha_min=fr.alpha_min,
                      depth_max=fr.depth_max, native=True)
    v, f, c = vol.extract_mesh(min_weight=1.0, native=True)
    return dict(tsdf=vol.tsdf, weight=vol.weight, color=vol.color, vertices=v, faces=f, colors=c)


def test_fusion_and_extraction_on_a_side_stream():
    case = ST.Case("tsdf_integrate_extract", _stream_make, _stream_staged, _stream_run, blocking=True)
    got = ST.check_on_side_stream(case, torch.cuda.Stream(device=DEV), DEV)
    assert got["faces"].shape[0] > 0 and bool(torch.isfinite(got["vertices"]).all())


# ---- extraction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_name", ["2x2x2", "17x9x21", "65x33x70"])
def test_extraction_on_the_fused_volume_against_the_reference(grid_name):
    grid = TR.MESH_GRIDS.get(grid_name) or TR.GRIDS[grid_name]
    vol = integrate_frames(make_volume(grid, DEV), TR.make_frames(96, 96), native=True)
    tsdf, weight, color = (t.cpu().numpy() for t in (vol.tsdf, vol.weight, vol.color))
    for min_weight in (1.0, 2.0):
        ref = TR.surface_nets_ref(grid, tsdf, weight, color, min_weight)
        got = vol.extract_mesh(min_weight=min_weight, native=True)
        print(f"{grid_name} min_weight {min_weight}: V = {got[0].shape[0]}, F = {got[1].shape[0]}")
        assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
        check_mesh(got, ref, f"kernel {grid_name} min_weight {min_weight}")
        again = vol.extract_mesh(min_weight=min_weight, native=True)
        assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two extractions of one volume differ"
    assert TR.surface_nets_ref(grid, tsdf, weight, color, 1.0)["vertices"].v.shape[0] > 0
    if grid.n > 8:
        assert TR.surface_nets_ref(grid, tsdf, weight, color, 1.0)["faces"].shape[0] > 0 and (weight == 0).any()


def test_extraction_of_a_volume_without_an_active_cell_and_of_thin_volumes():
    grid = TR.Grid((19, 7, 11), (0, 0, 0), 0.1, 0.3)
    for tsdf, weight in ((np.full(grid.n, 0.5, np.float32), np.ones(grid.n, np.float32)),
                         (np.linspace(-1, 1, grid.n, dtype=np.float32), np.zeros(grid.n, np.float32))):
        v, f, c = volume_of(grid, tsdf, weight, np.zeros(3 * grid.n, np.float32), DEV).extract_mesh(native=True)
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3) and f.dtype == torch.int32
    for dims in ((1, 5, 5), (5, 1, 5), (5, 5, 1), (1, 1, 1)):
        grid = TR.Grid(dims, (0, 0, 0), 0.1, 0.3)
        v, f, c = volume_of(grid, np.linspace(-1, 1, grid.n, dtype=np.float32), np.ones(grid.n, np.float32), np.zeros(3 * grid.n, np.float32),
                            DEV).extract_mesh(native=True)
        assert v.shape == (0, 3) and f.shape == (0, 3) and c.shape == (0, 3)


@pytest.mark.parametrize("half", [False, True], ids=["observed", "half_unobserved"])
def test_extraction_of_the_analytic_sphere(half):
    grid, tsdf, weight, color, ref = sphere_reference(half)
    got = volume_of(grid, tsdf, weight, color, DEV).extract_mesh(native=True)
    check_mesh(got, ref, "kernel sphere" + (" (half unobserved)" if half else ""))
    v, f, _ = (a.cpu().numpy() for a in got)
    if not half:
        sphere_checks(grid, v, f, ref["vertices"].v.numpy(), "kernel")
    else:
        used = ref["cells"][np.unique(f)]
        obs = weight >= 1
        for dx, dy, dz in TR.CORNER:
            assert obs[used[:, 2] + dz, used[:, 1] + dy, used[:, 0] + dx].all(), "a face references a cell with an unobserved corner"


@pytest.fixture(scope="module")
def three_round_device_volume():
    """TR.three_round_volume() on the device, uploaded once (100 MB)."""
    return volume_of(*TR.three_round_volume(), DEV)


@pytest.mark.parametrize("min_weight", [1.0, 2.0])
def test_extraction_past_the_first_round_of_the_voxel_scan(three_round_device_volume, min_weight):
    """131 x 127 x 300 voxels are 19 497 blocks, three rounds of k_sn_scan: the vertices and quads that voxels of rounds 1 and 2 own
    are placed by the carry between rounds, and every face that names one of their vertices reads a prefix of those rounds."""
    grid, ref = three_round_conditions(min_weight, "kernel")
    vol = three_round_device_volume
    got = vol.extract_mesh(min_weight=min_weight, native=True)
    print(f"three rounds min_weight {min_weight}: V = {got[0].shape[0]}, F = {got[1].shape[0]}; vertices per round "
          f"{TR.scan_rounds(ref['vertex_owners'], grid.n).tolist()}, quads per round {TR.scan_rounds(ref['quad_owners'], grid.n).tolist()}")
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.int32 and got[2].dtype == torch.float32
    check_mesh(got, ref, f"kernel three rounds min_weight {min_weight}")
    again = vol.extract_mesh(min_weight=min_weight, native=True)
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two extractions of one volume differ"


# ---- end to end ---------------------------------------------------------------------------------------------------------------
W_E2E, H_E2E, P_E2E = 96, 96, 4000
BOUNDS = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def _shell_scene(P=P_E2E, radius=TR.SPHERE_R, seed=9):
    """P small, nearly opaque Gaussians on the sphere of `radius` around the origin, coloured by position."""
    g = torch.Generator().manual_seed(seed)
    d = torch.nn.functional.normalize(torch.randn(P, 3, generator=g), dim=1)
    shs = ((0.5 + 0.4 * d) - 0.5)[:, None, :] / S.SH_C0
    return S.Scene((radius * d).contiguous(), torch.full((P, 3), math.log(0.03)), torch.randn(P, 4, generator=g), torch.full((P, 1), 3.0),
                   shs.contiguous(), 0)


def _ring_cameras(n=8, distance=2.2):
    cams = []
    for i in range(n):
        a = 2 * math.pi * i / n
        V = TR.look_at((distance * math.cos(a), distance * math.sin(a), 0.6 * math.sin(2 * a) + 0.3), (0.0, 0.0, 0.0)).astype(np.float64)
        cams.append(S.make_camera(W_E2E, H_E2E, V[:3, :3], V[3, :3], tanfovy=0.45).to(DEV))
    return cams


def _mesh_is_sound(v, f, c, what):
    v, f, c = v.cpu().numpy(), f.cpu().numpy(), c.cpu().numpy()
    print(f"{what}: V = {len(v)}, F = {len(f)}")
    assert len(v) > 0 and len(f) > 0 and v.shape == c.shape and f.shape[1] == 3
    assert np.isfinite(v).all() and np.isfinite(c).all()
    assert (v >= np.asarray(BOUNDS[0])).all() and (v <= np.asarray(BOUNDS[1])).all()
    assert f.min() >= 0 and f.max() < len(v)
    return v, f, c


def test_end_to_end_from_gaussians_to_a_ply_file(tmp_path):
    """Asks nothing of the mesh's quality: projective fusion of eight views leaves holes and silhouette artefacts by nature."""
    from gaussian_params import Pipe
    from scene import GaussianModel
    from scene.mesh import load_mesh_ply, save_mesh_ply
    gm = GaussianModel(0)
    gm.adopt_scene(_shell_scene(), device=DEV)
    cams, bg = _ring_cameras(), torch.zeros(3, device=DEV)
    got = gm.extract_mesh(cams, Pipe(), bg, bounds=BOUNDS, voxel_size=2.0 / 48)
    v, f, c = _mesh_is_sound(*got, "sphere shell, 8 cameras, 48^3")
    r = np.linalg.norm(v, axis=1)
    print(f"vertex radii {r.min():.3f} .. {r.max():.3f} (the shell's {TR.SPHERE_R})")
    path = str(tmp_path / "mesh.ply")
    save_mesh_ply(path, *got)
    v2, f2, c2 = load_mesh_ply(path)
    assert np.array_equal(v2.view(np.int32), v.view(np.int32)) and np.array_equal(f2, f)
    assert np.array_equal(c2, np.rint(np.clip(c.astype(np.float64), 0, 1) * 255).astype(np.uint8))
    again = gm.extract_mesh(cams, Pipe(), bg, bounds=BOUNDS, voxel_size=2.0 / 48)
    assert all(ST.same_bits(a.cpu(), b.cpu()) for a, b in zip(got, again)), "two extractions of one model differ"
    # a model with a 3D filter renders its filtered scales, and the mesh follows
    gm.compute_3D_filter(cams)
    _mesh_is_sound(*gm.extract_mesh(cams, Pipe(), bg, bounds=BOUNDS, voxel_size=2.0 / 48), "with a 3D filter")


def test_end_to_end_with_a_latent_model():
    from gaussian_params import Pipe
    from scene import mesh
    from scene.latent_gaussian_model import LatentGaussianModel
    torch.manual_seed(4)
    m = LatentGaussianModel(0, _shell_scene(500).means3D.to(DEV), gaussians_per_structure=8)
    with torch.no_grad():
        m.structure_scales.fill_(-3.5)
        m()
    v, f, c = mesh.extract_mesh(m, _ring_cameras(), Pipe(), torch.zeros(3, device=DEV), bounds=BOUNDS, voxel_size=2.0 / 48)
    print(f"latent model: V = {v.shape[0]}, F = {f.shape[0]}")
    assert v.shape == c.shape and f.dtype == torch.int32 and bool(torch.isfinite(v).all())
    assert f.numel() == 0 or (int(f.min()) >= 0 and int(f.max()) < v.shape[0])
