"""CPU checks of the vector-quantisation feature: the torch twins of diff_gaussian_rasterization.vq against the float64 reference
(tests/vq_ref.py) under the rules the HIP kernels are held to, k-means on separated blobs, the monotone objective, the compressed
checkpoint's round trip, and the C ABI's argument validation (which touches no device)."""
import ctypes as C

import numpy as np
import pytest
import torch

import scene_synth as S
import vq_ref as R
from diff_gaussian_rasterization import vq
from scene import compression
from scene.gaussian_model import GaussianModel

T = torch.from_numpy


@pytest.mark.parametrize("P,K,D", [(1, 1, 1), (33, 2, 1), (1000, 33, 3), (2000, 100, 9), (3000, 257, 45), (500, 33, 128), (300, 20, 200)])
def test_assign_twin_holds_the_distance_and_index_rules(P, K, D):
    x, cb = R.fixture(P, K, D)
    idx, dist2 = vq.assign(T(x), T(cb))
    assert idx.dtype == torch.int32 and dist2.dtype == torch.float32
    R.Assign(x, cb).check(idx.numpy(), dist2.numpy())


def test_assign_twin_chunks_p(monkeypatch):
    x, cb = R.fixture(1000, 31, 2)
    whole = vq.assign_torch(T(x), T(cb))
    monkeypatch.setattr(vq, "CHUNK_BYTES", 4 * 31 * 7)          # seven rows per chunk
    parts = vq.assign_torch(T(x), T(cb))
    R.Assign(x, cb).check(parts[0].numpy(), parts[1].numpy())
    assert torch.equal(whole[0], parts[0])


@pytest.mark.parametrize("P,K,D", [(33, 2, 1), (1000, 33, 3), (5000, 257, 45), (40, 100, 5)])
def test_update_twin_is_the_mean_of_the_members(P, K, D):
    x, cb = R.fixture(P, K, D)
    idx = R.Assign(x, cb).idx.astype(np.int32)
    new, counts = vq.update_codebook(T(x), T(idx), T(cb))
    R.check_update(x, idx, cb, new.numpy(), counts.numpy())
    if K > P:
        assert int((counts == 0).sum()) >= K - P


def test_kmeans_recovers_separated_blobs():
    x, label, init = R.blobs()
    K = len(init)
    cb, idx = vq.kmeans(T(x), K, iters=1, init=T(init))
    assert cb.shape == (K, x.shape[1]) and idx.dtype == torch.int32
    assert np.array_equal(idx.numpy(), label)                 # code k started inside blob k
    # the centroid is formed on the centred table: the update bound there, and three more roundings (x - mean, the mean's own
    # rounding seen through it, codebook + mean) of values no larger than 2 max |x|: 2^-21 max |x|
    x64 = x.astype(np.float64)
    want, n, tol = R.means(x - x.mean(0, dtype=np.float64).astype(np.float32), label, np.zeros((K, x.shape[1]), np.float32))
    blob_mean = np.stack([x64[label == k].mean(0) for k in range(K)])
    assert (n == 50).all()
    assert (np.abs(cb.numpy() - blob_mean) <= tol + 2.0 ** -21 * np.abs(x).max()).all()


def test_kmeans_shapes_and_host_sampling():
    x, _ = R.fixture(200, 1, 6)
    g = torch.Generator().manual_seed(3)
    cb, idx = vq.kmeans(T(x), 16, iters=3, generator=g)
    want = torch.randperm(200, generator=torch.Generator().manual_seed(3))[:16]
    cb0, _ = vq.kmeans(T(x), 16, iters=0, generator=torch.Generator().manual_seed(3))
    assert np.abs(cb0.numpy() - x[want.numpy()]).max() <= 2.0 ** -21 * np.abs(x).max()      # the rows, centred and moved back
    assert cb.shape == (16, 6) and idx.shape == (200,)
    again = vq.assign(T(x), cb)[0]
    assert (R.sqdist(x, cb.numpy()[again.numpy()]) <= R.sqdist(x, cb.numpy()[idx.numpy()]) + 2 * R.bound(x, cb.numpy())).all()
    cb, idx = vq.kmeans(T(x[:5]), 16)                          # K' = min(K, P)
    assert cb.shape == (5, 6) and sorted(idx.tolist()) == list(range(5))
    cb, idx = vq.kmeans(T(x[:0]), 16)
    assert cb.shape == (0, 6) and idx.shape == (0,)


def test_objective_never_increases():
    x, cb = R.fixture(3000, 40, 12)
    x = x + 0.5 * np.sign(x)                                   # some structure: two clumps per axis
    xt, cbt = T(x), T(cb)
    slack = 2 * R.bound(x, cb).sum()
    idx, _ = vq.assign(xt, cbt)
    prev = R.objective(x, cb, idx.numpy())
    for _ in range(6):
        cbt, _ = vq.update_codebook(xt, idx, cbt)
        idx, _ = vq.assign(xt, cbt)
        now = R.objective(x, cbt.numpy(), idx.numpy())
        assert now <= prev + slack, (now, prev)
        prev = now


def test_dispatch_and_input_checks():
    x, cb = R.fixture(10, 3, 4)
    with pytest.raises(RuntimeError, match="native=True needs device tensors"):
        vq.assign(T(x), T(cb), native=True)
    with pytest.raises(RuntimeError, match="native=True needs device tensors"):
        vq.kmeans(T(x), 3, native=True)
    with pytest.raises(ValueError, match="contiguous float32"):
        vq.assign(T(x).double(), T(cb).double())
    with pytest.raises(ValueError, match="contiguous float32"):
        vq.assign(T(x).t().contiguous().t(), T(cb))
    with pytest.raises(ValueError, match="int32"):
        vq.update_codebook(T(x), torch.zeros(10, dtype=torch.int64), T(cb))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        vq.assign(T(x), T(cb[:, :3].copy()))


def _host_model(P, D, seed=11):
    m = GaussianModel(D)
    m.adopt_scene(S.make_scene(P, 64, 48, D, seed), device="cpu")
    return m


def _check_round_trip(m, d, back):
    n = lambda t: t.detach().reshape(t.shape[0], -1).numpy()
    assert np.array_equal(back["xyz"].numpy(), n(m._xyz))
    for name, t in (("f_dc", m._features_dc), ("opacity", m._opacity), ("scaling", m._scaling), ("rotation", m._rotation)):
        v, got = n(t), back[name].reshape(t.shape[0], -1).numpy()
        assert d[name].dtype == np.uint8 and back[name].dtype == torch.float32 and back[name].shape == t.shape
        step = (d[name + "_max"].astype(np.float64) - d[name + "_min"]) / 255
        # half a step, and the decoder's two roundings (the product's and the sum's cast to float32)
        assert (np.abs(got.astype(np.float64) - v) <= step / 2 + 2.0 ** -23 * np.abs(v).max(0)).all(), name


@pytest.mark.parametrize("D", [3, 1])
def test_compressed_round_trip(tmp_path, D):
    m = _host_model(700, D)
    with torch.no_grad():
        m._t["scaling"][:, 1] = -3.25                          # a constant column
    path = str(tmp_path / "model.gsq")
    m.save_compressed(path, sh_clusters=64, iters=3, generator=torch.Generator().manual_seed(0))
    with np.load(path, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    assert d["indices"].dtype == np.uint16 and d["codebook"].shape == (64, 3 * ((D + 1) ** 2 - 1)) and int(d["sh_degree"]) == D
    back = compression.decompress(compression.load_compressed(path))
    _check_round_trip(m, d, back)
    assert np.array_equal(back["scaling"][:, 1].numpy(), np.full(700, -3.25, np.float32))
    assert np.array_equal(back["f_rest"].reshape(700, -1).numpy(), d["codebook"][d["indices"].astype(np.int64)])
    # the stored indices are the nearest codes of the model's rows
    rest = m._features_rest.detach().reshape(700, -1).numpy()
    R.Assign(rest, d["codebook"]).check(d["indices"].astype(np.int64), R.sqdist(rest, d["codebook"][d["indices"].astype(np.int64)]),
                                        index_rule=False)
    m2 = GaussianModel(D)
    m2.load_compressed(path, device="cpu")
    assert m2.active_sh_degree == D and m2._features.shape == m._features.shape and m2._xyz.requires_grad
    assert torch.equal(m2._features_rest.detach(), back["f_rest"])


def test_compressed_degree_zero_has_no_codebook(tmp_path):
    m = _host_model(300, 0)
    d = compression.compress(m)
    assert "codebook" not in d and "indices" not in d
    path = str(tmp_path / "dc.gsq")
    compression.save_compressed(path, d)
    back = compression.decompress(compression.load_compressed(path))
    _check_round_trip(m, d, back)
    assert back["f_rest"].shape == (300, 0, 3)
    m2 = GaussianModel(0)
    m2.load_compressed(path, device="cpu")
    assert m2._features.shape == (300, 1, 3)


def test_int32_index_files_load(tmp_path):
    m = _host_model(50, 1)
    d = compression.compress(m, sh_clusters=8, iters=1, generator=torch.Generator().manual_seed(0))
    assert d["indices"].dtype == np.uint16
    wide = dict(d, indices=d["indices"].astype(np.int32))       # what a codebook of more than 65 536 rows is stored with
    for name, dd in (("a", d), ("b", wide)):
        path = str(tmp_path / name)
        compression.save_compressed(path, dd)
        got = compression.load_compressed(path)
        assert got["indices"].dtype == dd["indices"].dtype
        assert np.array_equal(compression.decompress(got)["f_rest"].reshape(50, -1).numpy(), d["codebook"][d["indices"].astype(np.int64)])
    assert compression.MAX_U16_CODES == 65536
    with pytest.raises(ValueError, match="format version"):
        compression.decompress(dict(d, version=np.int32(99)))


def test_abi_refuses_unsupported_shapes():
    from diff_gaussian_rasterization import _native
    lib = _native.load()
    b = C.c_size_t(0)
    one = C.c_void_p(256)                                       # never dereferenced: the arguments are refused first
    for P, K, D, word in ((10, 5, 129, b"D = 129"), (10, 5, 0, b"D = 0"), (10, 0, 5, b"K = 0"), (-1, 5, 5, b"P = -1")):
        assert lib.gsr_vq_workspace_size(C.c_int64(P), C.c_int32(K), C.c_int32(D), C.byref(b)) == -1
        assert word in lib.gsr_last_error()
        assert lib.gsr_vq_assign(C.c_int64(P), C.c_int32(K), C.c_int32(D), one, one, one, one, one, C.c_size_t(1 << 30), None) == -1
        assert word in lib.gsr_last_error() and b"gsr_vq_assign" in lib.gsr_last_error()
        assert lib.gsr_vq_update(C.c_int64(P), C.c_int32(K), C.c_int32(D), one, one, one, one, one, one, C.c_size_t(1 << 30), None) == -1
        assert word in lib.gsr_last_error()
    assert _native.vq_workspace_size(0, 1, 1) > 0
    assert _native.vq_workspace_size(1_000_000, 65536, 45) >= 4 * 4 * 1_000_000 + 65536 * 12
    assert lib.gsr_vq_assign(C.c_int64(0), C.c_int32(4), C.c_int32(4), None, None, None, None, None, C.c_size_t(0), None) == 0      # P = 0
    assert lib.gsr_vq_assign(C.c_int64(8), C.c_int32(4), C.c_int32(4), one, one, one, one, one, C.c_size_t(16), None) == _native.ERR_WORKSPACE
    with pytest.raises(_native.GsrError, match="D = 129"):
        _native.vq_workspace_size(10, 5, 129)
