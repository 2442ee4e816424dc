"""The vector-quantisation kernels (csrc/gsr_vq.hip) on the device against the float64 reference of tests/vq_ref.py: the distance
and index rules of the fused assignment at the smallest shapes that cross each edge of its tiling, the centroid update, bit-equal
repeats, k-means native against its torch twin, and the compressed checkpoint of a device model."""
import functools

import numpy as np
import pytest
import torch

import scene_synth as S
import vq_ref as R
from diff_gaussian_rasterization import vq

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (P, K, D): the 32-wide point and code tiles, odd D, the D limit, more than one block (256 points), more than one LDS stage of
# codes (128, or 64 from D = 65 on); the last three add the kernel instances for 49 <= D <= 64 and 65 <= D <= 96 and a multi-stage
# run of the widest one
ASSIGN_SHAPES = [(1, 1, 1), (33, 2, 1), (1000, 8, 1), (1000, 31, 2), (1000, 33, 3), (2000, 100, 9), (3000, 257, 24), (5000, 257, 45),
                 (2000, 65, 46), (4097, 1025, 45), (2000, 33, 128), (20000, 300, 45), (2000, 65, 50), (2000, 65, 70), (1500, 130, 100)]
# (40, 100, 5): K > P, empty codes.  From P >= 64 K on a code's run is cut into four quarters: (20000, 300, 45), and the last two
# (two columns per lane; runs of a few dozen members)
UPDATE_SHAPES = [(33, 2, 1), (1000, 33, 3), (5000, 257, 45), (20000, 300, 45), (40, 100, 5), (9000, 130, 100), (200, 3, 2)]


@functools.lru_cache(maxsize=None)
def _case(P, K, D):
    x, cb = R.fixture(P, K, D)
    return x, cb, R.Assign(x, cb)


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _bits(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int32)


@pytest.mark.parametrize("P,K,D", ASSIGN_SHAPES)
def test_assign_holds_the_distance_and_index_rules(P, K, D):
    x, cb, ref = _case(P, K, D)
    xd, cd = _dev(x), _dev(cb)
    idx, dist2 = vq.assign(xd, cd, native=True)
    assert idx.dtype == torch.int32 and dist2.dtype == torch.float32 and idx.shape == dist2.shape == (P,)
    ref.check(idx.cpu().numpy(), dist2.cpu().numpy())
    idx2, dist22 = vq.assign(xd, cd, native=True)
    assert np.array_equal(_bits(idx), _bits(idx2)) and np.array_equal(_bits(dist2), _bits(dist22))
    assert np.array_equal(_bits(xd), x.view(np.uint32)) and np.array_equal(_bits(cd), cb.view(np.uint32))


def test_duplicated_codes_go_to_the_lowest_index():
    x, cb, _ = _case(2000, 100, 9)
    cb = np.concatenate([cb, cb[:40], cb[60:]])                # code 100 + i = code i, code 140 + i = code 60 + i: across code tiles
    idx, dist2 = vq.assign(_dev(x), _dev(cb), native=True)
    ref = R.Assign(x, cb)
    ref.check(idx.cpu().numpy(), dist2.cpu().numpy(), index_rule=False)
    idx = idx.cpu().numpy()
    assert idx.max() < 100                                     # a copy never wins over its original
    only, _ = vq.assign(_dev(x), _dev(cb[:100].copy()), native=True)
    assert np.array_equal(idx, only.cpu().numpy())
    same = np.repeat(cb[:1], 70, 0)                            # every code the same row, over the two half-waves and three tiles
    idx, _ = vq.assign(_dev(x), _dev(same), native=True)
    assert not idx.any()


def test_a_point_equal_to_a_code_has_distance_zero():
    x, cb, _ = _case(3000, 257, 24)
    x = x.copy()
    x[::7] = cb[np.arange(len(x[::7])) % 257]
    idx, dist2 = vq.assign(_dev(x), _dev(cb), native=True)
    R.Assign(x, cb).check(idx.cpu().numpy(), dist2.cpu().numpy())
    assert not dist2.cpu().numpy()[::7].any()
    assert np.array_equal(idx.cpu().numpy()[::7], np.arange(len(x[::7])) % 257)


def test_offset_cloud_holds_the_distance_rule():
    """Every column + 10: B grows with the norms (the reason kmeans centres the table); the index rule is not applied."""
    x, cb, _ = _case(5000, 257, 45)
    x, cb = x + np.float32(10), cb + np.float32(10)
    idx, dist2 = vq.assign(_dev(x), _dev(cb), native=True)
    R.Assign(x, cb).check(idx.cpu().numpy(), dist2.cpu().numpy(), index_rule=False)


def test_no_points():
    idx, dist2 = vq.assign(torch.zeros(0, 5, device=DEV), torch.zeros(3, 5, device=DEV), native=True)
    assert idx.shape == dist2.shape == (0,) and idx.dtype == torch.int32 and dist2.dtype == torch.float32 and idx.is_cuda
    cb = _dev(R.fixture(1, 3, 5)[1])
    new, counts = vq.update_codebook(torch.zeros(0, 5, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), cb, native=True)
    assert np.array_equal(_bits(new), _bits(cb)) and not counts.any()


def test_unsupported_shape_raises():
    with pytest.raises(RuntimeError, match="D = 129"):
        vq.assign(torch.zeros(4, 129, device=DEV), torch.zeros(2, 129, device=DEV))
    idx, _ = vq.assign(torch.zeros(4, 129, device=DEV), torch.ones(2, 129, device=DEV), native=False)
    assert not idx.any()


@pytest.mark.parametrize("P,K,D", UPDATE_SHAPES)
def test_update_is_the_mean_of_the_members(P, K, D):
    x, cb, ref = _case(P, K, D)
    idx = ref.idx.astype(np.int32)
    xd, cd, idd = _dev(x), _dev(cb), _dev(idx)
    new, counts = vq.update_codebook(xd, idd, cd, native=True)
    R.check_update(x, idx, cb, new.cpu().numpy(), counts.cpu().numpy())
    if K > P:
        assert int((counts == 0).sum()) >= K - P
    new2, counts2 = vq.update_codebook(xd, idd, cd, native=True)
    assert np.array_equal(_bits(new), _bits(new2)) and np.array_equal(_bits(counts), _bits(counts2))
    assert np.array_equal(_bits(xd), x.view(np.uint32)) and np.array_equal(_bits(cd), cb.view(np.uint32)) and np.array_equal(_bits(idd), idx)


def test_update_ignores_indices_outside_the_codebook():
    x, cb, ref = _case(1000, 33, 3)
    idx = ref.idx.astype(np.int32)
    idx[::5] = 33
    idx[1::5] = -1
    keep = (idx >= 0) & (idx < 33)
    new, counts = vq.update_codebook(_dev(x), _dev(idx), _dev(cb), native=True)
    R.check_update(x[keep], idx[keep], cb, new.cpu().numpy(), counts.cpu().numpy())


def test_one_kmeans_iteration_native_against_torch():
    x, label, init = R.blobs()
    K = len(init)
    cb_n, idx_n = vq.kmeans(_dev(x), K, iters=1, init=torch.from_numpy(init), native=True)
    cb_t, idx_t = vq.kmeans(_dev(x), K, iters=1, init=torch.from_numpy(init), native=False)
    assert torch.equal(idx_n, idx_t) and np.array_equal(idx_n.cpu().numpy(), label)
    xc = x - x.mean(0, dtype=np.float64).astype(np.float32)
    _, _, tol = R.means(xc, label, np.zeros((K, x.shape[1]), np.float32))
    # both are within the update bound of the true mean on the centred table; the centring itself adds 2^-21 max |x| (test_vq_ref.py)
    assert (np.abs(cb_n.cpu().numpy().astype(np.float64) - cb_t.cpu().numpy()) <= 2 * tol + 2.0 ** -20 * np.abs(x).max()).all()
    again, _ = vq.kmeans(_dev(x), K, iters=1, init=torch.from_numpy(init), native=True)
    assert np.array_equal(_bits(again), _bits(cb_n))


def test_compressed_checkpoint_of_a_device_model_renders(tmp_path):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene.gaussian_model import GaussianModel
    W, H = 128, 96
    m = GaussianModel(3)
    m.adopt_scene(S.make_scene(3000, W, H, 3, 7, scale_lo=0.005, scale_hi=0.06), device=DEV)
    path = str(tmp_path / "model.gsq")
    m.save_compressed(path, sh_clusters=256, generator=torch.Generator().manual_seed(0))
    with np.load(path, allow_pickle=False) as z:
        assert z["codebook"].shape == (256, 45) and z["indices"].dtype == np.uint16 and z["indices"].max() < 256
    m2 = GaussianModel(3)
    m2.load_compressed(path, device=DEV)
    cam, bg = S.make_camera(W, H).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        a = render(cam, m, Pipe(), bg)["render"]
        b = render(cam, m2, Pipe(), bg)["render"]
    assert b.shape == a.shape == (3, H, W) and bool(torch.isfinite(b).all())
    mse = float((a - b).square().mean())
    print(f"compressed (256 SH codes, uint8 attributes) against the original render: PSNR {10 * np.log10(1.0 / max(mse, 1e-20)):.2f} dB")
