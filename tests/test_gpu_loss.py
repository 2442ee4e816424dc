"""The fused loss kernels (csrc/gsr_loss.hip: k_loss_fwd, k_loss_bwd, k_loss_finish, k_l1_bwd) against the binary64
reference of tests/loss_ref.py, pixel by pixel, held to what plain binary32 reaches on the same inputs (check_loss).

Outputs are prefilled with NaN (the gradient) and 0xFF bytes (the workspace, so its derivative maps read NaN where
nothing was written).  The maps are read from the workspace as carve_loss lays it out: three C*H*W float planes at
256-byte aligned offsets, then the per-block partial sums.

Shapes run with uniform noise and a smooth image against its target + N(0, 1e-3^2) at C = 3; every content class runs at
1080p; channel counts, lambda, upstream and the staging pairs run on small shapes.  The 4K frame is checked in row bands.
The per-class table (device | yardstick, p50 / p99 / max of |e| / (eps32 * magnitude)) prints at the end.
"""
import math

import numpy as np
import pytest
import torch

import loss_ref as L
import scene_synth as S

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ALIGN = 256                                 # kAlign of csrc/gsr_internal.h: the workspace's plane alignment
REPORT = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    """Prints the per-class table of whatever ran in this module once it is done: device | yardstick, p50 / p99 / max of
    |e| / (eps32 * magnitude); sums in eps32 * sum|terms|."""
    REPORT.clear()
    yield
    print("\nfused loss vs binary64 (device | binary32 yardstick)")
    for label, out in REPORT:
        print(L.format_row(label, out))


def _align(v):
    return (v + ALIGN - 1) // ALIGN * ALIGN


class Dev:
    """A device evaluation: grad [C, H, W], d_mu / d_eaa / d_eab [C, H, W] (workspace planes), out (out3 or out2)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def band(self, ref):
        """The rows `ref` describes, with its sums: whole image from out3 (means times n), slab from out2 (raw sums)."""
        (y0, y1), (mb, me) = ref.rows, ref.map_rows
        b = Dev(grad=self.grad[:, y0:y1], d_mu=self.d_mu[:, mb:me], d_eaa=self.d_eaa[:, mb:me], d_eab=self.d_eab[:, mb:me])
        if self.rows is None:
            b.l1_sum, b.ssim_sum = float(self.out[1]) * ref.n, float(self.out[2]) * ref.n
        else:
            b.l1_sum, b.ssim_sum = float(self.out[0]), float(self.out[1])
        return b


def run_device(a, b, lam=0.2, up=1.0, rows=None, offset=False):
    """Forward + backward through the C ABI.  offset=True: image, target and workspace are views 4 bytes past a 16-byte
    boundary, which forces scalar staging in both kernels."""
    from diff_gaussian_rasterization import _native as N
    C, H, W = a.shape
    n = C * H * W
    size = N.loss_workspace_size(C, H, W)
    if offset:
        bufs = [torch.empty(n + 8, dtype=torch.float32, device=DEV) for _ in range(2)]
        ad, bd = (buf[1:1 + n].view(C, H, W) for buf in bufs)
        ad.copy_(a.to(DEV))
        bd.copy_(b.to(DEV))
        wsbuf = torch.full((size + 16,), 0xFF, dtype=torch.uint8, device=DEV)
        ws = wsbuf[4:4 + size]
        assert ad.data_ptr() % 16 == 4 and ws.data_ptr() % 16 == 4
    else:
        ad, bd = a.to(DEV).contiguous(), b.to(DEV).contiguous()
        ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)
    grad = torch.full((C, H, W), math.nan, dtype=torch.float32, device=DEV)
    upt = torch.tensor([up], dtype=torch.float32, device=DEV)
    if rows is None:
        out = torch.full((3,), math.nan, dtype=torch.float32, device=DEV)
        N.loss_forward(ad, bd, lam, ws, out)
        N.loss_backward(ad, bd, lam, upt, ws, grad)
    else:
        out = torch.full((2,), math.nan, dtype=torch.float32, device=DEV)
        N.loss_forward_rows(ad, bd, ws, out, rows[0], rows[1])
        N.loss_backward_rows(ad, bd, lam, upt, ws, grad, rows[0], rows[1])
    torch.cuda.synchronize()
    step = _align(4 * n)
    maps = [ws[k * step:k * step + 4 * n].view(torch.float32).view(C, H, W).cpu() for k in range(3)]
    return Dev(grad=grad.cpu(), d_mu=maps[0], d_eaa=maps[1], d_eab=maps[2], out=out.cpu().numpy().astype(np.float64),
               rows=rows)


def _check_value(dev, ref, ys, label):
    """out3[0], the loss, against binary64: c * eps32 * (sum of the magnitudes of its terms) / n, c from the yardstick as
    for the sums."""
    lam, n = ref.lam, ref.n
    mag = (1.0 - lam) * ref.l1_abs / n + lam * (1.0 + ref.ssim_abs / n)
    err = abs(float(dev.out[0]) - ref.loss) / (L.EPS32 * mag)
    ery = abs(ys.loss - ref.loss) / (L.EPS32 * mag)
    assert err <= max(L.CAP_SUM * ery, L.SUM_FLOOR), f"{label}: loss off by {err:.3g} eps32 * magnitude (yardstick {ery:.3g})"


def check(label, dev, ref, ys, value=True):
    out = L.check_loss(dev.band(ref), ref, ys, label=label, report=REPORT)
    if value and dev.rows is None and hasattr(ref, "loss"):
        _check_value(dev, ref, ys, label)
    return out


# ---------------------------------------------------------------------------------------------------------------- inputs

def make_input(content, C, H, W, seed=0):
    g = torch.Generator().manual_seed(1000 + seed + 7 * H + W)
    if content == "uniform":
        return torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
    if content.startswith("smooth"):
        return L.smooth_pair(C, H, W, float(content[6:]), seed=seed)
    if content == "equal":                  # a = b exactly, with a zero background
        a, _ = L.smooth_pair(C, H, W, 0.0, seed=seed)
        a[:, :, : W // 3] = 0.0
        a[:, H // 2:H // 2 + H // 8] = 0.0
        return a, a.clone()
    if content == "constant":               # flat planes: s1 = s2 = s12 = 0
        a = torch.rand(C, 1, 1, generator=g).expand(C, H, W).contiguous()
        b = torch.rand(C, 1, 1, generator=g).expand(C, H, W).contiguous()
        return a, b
    if content == "range15":                # values in [0, 1.5]
        return 1.5 * torch.rand(C, H, W, generator=g), 1.5 * torch.rand(C, H, W, generator=g)
    raise ValueError(content)


def cfg2_pair():
    """The rasterizer's cfg2 frame (800x800) as the target, its own render with the base colours jittered as the image."""
    import diff_gaussian_rasterization as dgr
    from util import raster_kwargs
    scene, cam = S.make_config("cfg2")
    kw = {k: (v.to(DEV).contiguous() if isinstance(v, torch.Tensor) else v) for k, v in raster_kwargs(scene, cam, as_numpy=False).items()}
    rs = dgr.GaussianRasterizationSettings(
        image_height=kw["image_height"], image_width=kw["image_width"], tanfovx=kw["tanfovx"], tanfovy=kw["tanfovy"], bg=kw["bg"],
        scale_modifier=kw["scale_modifier"], viewmatrix=kw["viewmatrix"], projmatrix=kw["projmatrix"], sh_degree=kw["sh_degree"],
        campos=kw["campos"], prefiltered=False, debug=False)
    shs = kw["shs"].float().clone()
    g = torch.Generator().manual_seed(21)
    shs[:, 0] += 0.05 * torch.randn(shs[:, 0].shape, generator=g).to(DEV)
    imgs = []
    for sh in (shs, kw["shs"].float()):
        color, _, _ = dgr.rasterize_forward(kw["means3D"].float(), sh, None, kw["opacities"].float(), kw["scales"].float(),
                                            kw["rotations"].float(), None, rs)
        imgs.append(color.detach().float().cpu().contiguous())
    return imgs[0], imgs[1]


# ---------------------------------------------------------------------------------------------------------------- tests

SHAPES = [(1, 1), (1, 37), (41, 1), (5, 7), (11, 11), (31, 33), (32, 32), (33, 33), (64, 96), (67, 101), (1080, 1920)]
BANDS_4K = [(0, 48), (2112, 2160), (1018, 1030), (1060, 1100)]     # top, bottom, across the 32-row seam at 1024, middle


@pytest.mark.parametrize("content", ["uniform", "smooth1e-3"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_shapes(shape, content):
    """Tile counts that are and are not multiples of 8 (the XCD-aware tile order), partial tiles, widths with and without
    float4 staging, degenerate 1-px images."""
    H, W = shape
    a, b = make_input(content, 3, H, W)
    dev = run_device(a, b)
    check(f"{content} 3x{H}x{W}", dev, L.ssim_l1_ref(a, b), L.yardstick32(a, b))


@pytest.mark.parametrize("content", ["uniform", "smooth1e-3"])
def test_4k_in_bands(content):
    C, H, W = 3, 2160, 3840
    a, b = make_input(content, C, H, W)
    dev = run_device(a, b)
    for rows in BANDS_4K:
        ref, ys = L.ssim_l1_ref(a, b, rows=rows), L.yardstick32(a, b, rows=rows)
        L.check_loss(dev.band(ref), ref, ys, label=f"{content} 4K rows {rows}", sums=False, report=REPORT)
    f64, ysum = L.ref_sums(a, b)
    n = float(C * H * W)
    whole = Dev(l1_sum=float(dev.out[1]) * n, ssim_sum=float(dev.out[2]) * n)
    for f, fa in (("l1_sum", "l1_abs"), ("ssim_sum", "ssim_abs")):
        rd = L.sum_ratio(getattr(whole, f), f64[f], f64[fa])
        ry = L.sum_ratio(ysum[f], f64[f], f64[fa])
        print(f"{content} 4K {f}: device {rd:.3g} | yardstick {ry:.3g} eps32 * sum|terms|")
        assert rd <= max(L.CAP_SUM * ry, L.SUM_FLOOR), (f, rd, ry)
    loss = 0.8 * f64["l1_sum"] / n + 0.2 * (1.0 - f64["ssim_sum"] / n)
    mag = 0.8 * f64["l1_abs"] / n + 0.2 * (1.0 + f64["ssim_abs"] / n)
    assert abs(float(dev.out[0]) - loss) <= L.SUM_FLOOR * L.EPS32 * mag


@pytest.mark.parametrize("content", ["smooth1e-1", "smooth1e-2", "equal", "constant", "range15", "cfg2"])
def test_content_classes(content):
    """Every content class at 1080p (uniform noise and sigma = 1e-3 run in test_shapes), and one real frame."""
    a, b = cfg2_pair() if content == "cfg2" else make_input(content, 3, 1080, 1920)
    dev = run_device(a, b)
    check(f"{content} {'x'.join(map(str, a.shape))}", dev, L.ssim_l1_ref(a, b), L.yardstick32(a, b))


SMALL = [(33, 33), (64, 96)]


@pytest.mark.parametrize("shape", SMALL, ids=[f"{h}x{w}" for h, w in SMALL])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_channels_lambda_upstream(shape, C):
    """lambda in {0, 0.2, 1} x upstream in {1, -3.5, 0}.  lambda = 0: the gradient is float32((1 - lambda) inv_count up) *
    sign(a - b) bit for bit (ties give 0)."""
    H, W = shape
    a, b = make_input("smooth1e-2", C, H, W, seed=C)
    b[:, : H // 4] = a[:, : H // 4]                       # exact ties
    for lam in (0.0, 0.2, 1.0):
        for up in (1.0, -3.5, 0.0):
            dev = run_device(a, b, lam, up)
            check(f"C={C} {H}x{W} lam={lam} up={up}", dev, L.ssim_l1_ref(a, b, lam, up), L.yardstick32(a, b, lam, up))
            if lam == 0.0:
                f = np.float32
                k = (f(1.0) - f(0.0)) * (f(1.0) / (f(C) * f(H) * f(W))) * f(up)
                want = torch.sign(a - b) * float(k)
                assert torch.equal(dev.grad, want), (C, shape, up)


def test_l1_backward_and_drop_in_ssim():
    """k_l1_bwd: sign(a - b) * float32(up / n) bit for bit, ties 0; loss_utils.ssim (lambda = 1, negated upstream) against
    d mean(SSIM) / d a in binary64."""
    from diff_gaussian_rasterization import _native as N
    import loss_utils
    a, b = make_input("smooth1e-2", 3, 67, 101)
    b[:, :10] = a[:, :10]
    n = a.numel()
    ad, bd = a.to(DEV), b.to(DEV)
    g = torch.full_like(ad, math.nan)
    up = -3.5
    N.loss_l1_backward(ad, bd, torch.tensor([up], device=DEV), g)
    f = np.float32
    assert torch.equal(g.cpu(), torch.sign(a - b) * float(f(up) * (f(1.0) / f(n))))
    x = ad.clone().requires_grad_(True)
    s = loss_utils.ssim(x, bd)
    (2.5 * s).backward()
    ref, ys = L.ssim_l1_ref(a, b, 1.0, -2.5), L.yardstick32(a, b, 1.0, -2.5)
    assert abs(float(s) - ref.ssim_sum / n) <= L.SUM_FLOOR * L.EPS32 * (ref.ssim_abs / n)
    dev = Dev(grad=x.grad.cpu())
    L.check_loss(dev, ref, ys, label="drop-in ssim", maps=False, sums=False, report=REPORT)


STAGING = [(5, 8), (32, 32), (67, 100), (64, 96), (1080, 1920)]


@pytest.mark.parametrize("shape", STAGING, ids=[f"{h}x{w}" for h, w in STAGING])
def test_staging_paths_bitwise(shape):
    """Width % 4 == 0 stages with float4 loads; the same pixels through views 4 bytes off a 16-byte boundary stage with
    scalar loads.  Everything after the LDS staging is the same code: out3, maps and gradient are bitwise equal."""
    H, W = shape
    a, b = make_input("smooth1e-2", 3, H, W, seed=3)
    for rows in (None, (min(7, H), H)):
        v = run_device(a, b, rows=rows)
        s = run_device(a, b, rows=rows, offset=True)
        assert np.array_equal(v.out, s.out, equal_nan=True), (shape, rows)
        for f in ("grad", "d_mu", "d_eaa", "d_eab"):
            assert torch.equal(torch.nan_to_num(getattr(v, f), nan=7.0), torch.nan_to_num(getattr(s, f), nan=7.0)), (shape, rows, f)


def _slabs(H):
    """Cuts at every offset class relative to the 32-row tiles and the 5-row halo."""
    cuts = [(0, 1), (0, 0), (0, 27), (5, 6), (27, 32), (31, 63), (40, 62), (45, 61), (50, 60), (58, 59), (32, 64), (37, 96),
            (27, 37), (64, 64), (59, 69), (96, 128), (H - 1, H), (H - 6, H), (100, H), (H, H), (0, H)]
    return sorted(set((max(0, min(y0, H)), max(0, min(y1, H))) for y0, y1 in cuts))


@pytest.mark.parametrize("W", [96, 67])
def test_slabs_against_float64(W):
    """gsr_loss_l1_ssim_forward_rows / backward_rows: each slab's two raw sums against the binary64 band sums, its gradient
    rows against the binary64 whole-image gradient, its derivative maps on [y0 - 5, y1 + 5) within the image; every
    other map row and gradient row stays unwritten (NaN)."""
    C, H = 3, 150
    a, b = make_input("smooth1e-2", C, H, W, seed=W)
    lam, up = 0.2, -3.5
    for (y0, y1) in _slabs(H):
        dev = run_device(a, b, lam, up, rows=(y0, y1))
        ref, ys = L.ssim_l1_ref(a, b, lam, up, rows=(y0, y1)), L.yardstick32(a, b, lam, up, rows=(y0, y1))
        mb, me = ref.map_rows
        check(f"slab W={W} [{y0}, {y1})", dev, ref, ys)
        assert bool(dev.grad[:, :y0].isnan().all()) and bool(dev.grad[:, y1:].isnan().all()), (y0, y1)
        for f in ("d_mu", "d_eaa", "d_eab"):
            m = getattr(dev, f)
            assert bool(m[:, :mb].isnan().all()) and bool(m[:, me:].isnan().all()), (y0, y1, f)


def test_determinism():
    a, b = make_input("uniform", 3, 1080, 1920, seed=9)
    r1, r2 = run_device(a, b), run_device(a, b)
    assert np.array_equal(r1.out, r2.out)
    for f in ("grad", "d_mu", "d_eaa", "d_eab"):
        assert torch.equal(getattr(r1, f), getattr(r2, f)), f
