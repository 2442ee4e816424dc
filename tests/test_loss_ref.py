"""CPU self-tests of tests/loss_ref.py: the binary64 reference of the fused loss reproduces the reference's golden values,
its folded derivative maps are torch autograd's, a row band is the same rows of the whole image, the gap between the
kernel's separable window and the reference's rounded 11x11 window is pinned, and check_loss names planted faults that
the tensor-wide bound of test_fused_loss_matches_reference_golden lets through."""
import os
import types

import numpy as np
import pytest
import torch

import loss_ref as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loss.npz")


def test_reference_window_reproduces_golden():
    """window="reference" against tests/golden/loss.npz (the reference's utils/loss_utils.py in binary32): values, the
    combined gradient and each function's own gradient, per pixel in units of eps32 * S_p."""
    gold = np.load(GOLDEN)
    consts = (0.01 ** 2, 0.03 ** 2)
    worst = 0.0
    for i in range(2):
        a, b = gold[f"a{i}"], gold[f"b{i}"]
        r = L.ssim_l1_ref(a, b, 0.2, 1.0, window="reference", consts=consts)
        n = r.n
        assert abs(r.loss - float(gold[f"loss_{i}"])) < 4 * L.EPS32
        assert abs(r.l1_sum / n - float(gold[f"l1_{i}"])) < 2 * L.EPS32 * r.l1_sum / n
        assert abs(r.ssim_sum / n - float(gold[f"ssim_{i}"])) < 4 * L.EPS32
        for key, lam, up in ((f"grad_a{i}", 0.2, 1.0), (f"grad_l1_a{i}", 0.0, 1.0), (f"grad_ssim_a{i}", 1.0, -1.0)):
            rk = L.ssim_l1_ref(a, b, lam, up, window="reference", consts=consts)
            e = (torch.from_numpy(gold[key]).double() - rk.grad).abs() / (L.EPS32 * rk.S)
            worst = max(worst, float(e.max()))
            assert float(e.max()) <= GOLDEN_MAX, (key, float(e.max()))
    print(f"golden: max |g_golden - g_64| / (eps32 S_p) = {worst:.2f}")


# binary32 torch (five 2-D convolutions and autograd through them) against binary64, over the three gradients of both golden
# pairs: measured max 9.54 eps32 * S_p; x 1.25
GOLDEN_MAX = 12.0


def _autograd_maps(a, b, window2d, consts):
    """torch binary64 autograd of loss_utils.ssim_torch with window2d substituted: d mean(SSIM) / d image, and the
    derivatives of sum(SSIM) with respect to the outputs of its mu1, E[a^2] and E[ab] convolutions."""
    import loss_utils
    C = a.shape[0]
    a64 = torch.from_numpy(a).double().unsqueeze(0).requires_grad_(True)
    b64 = torch.from_numpy(b).double().unsqueeze(0)
    key = (11, C, a64.device, a64.dtype)
    saved_w, saved_F = loss_utils._WINDOWS.get(key), loss_utils.F
    loss_utils._WINDOWS[key] = torch.from_numpy(window2d).double().expand(C, 1, 11, 11).contiguous()
    convs = []

    def conv2d(*args, **kw):
        y = torch.nn.functional.conv2d(*args, **kw)
        if y.requires_grad:
            y.retain_grad()
        convs.append(y)
        return y
    loss_utils.F = types.SimpleNamespace(conv2d=conv2d)
    try:
        s = loss_utils.ssim_torch(a64, b64)
    finally:
        loss_utils.F = saved_F
        if saved_w is None:
            del loss_utils._WINDOWS[key]
        else:
            loss_utils._WINDOWS[key] = saved_w
    n = a64.numel()
    s.backward()
    # ssim_torch's convolutions in order: mu1, mu2, E[a^2], E[b^2], E[ab]; it returns the mean
    return a64.grad[0], convs[0].grad[0] * n, convs[2].grad[0] * n, convs[4].grad[0] * n


@pytest.mark.parametrize("sigma", [1e-1, 1e-3])
def test_folded_maps_are_autograd_of_ssim_torch(sigma):
    """The kernel's folded derivative maps (d_mu, d_eaa, d_eab) in binary64 equal torch autograd of ssim_torch with the
    same (separable) window and constants, and so does the gradient they give: the kernel's algebra is the derivative."""
    a, b = (t.numpy() for t in L.smooth_pair(3, 48, 61, sigma, seed=4))
    g = L.kernel_taps().astype(np.float64)
    w2 = np.outer(g, g)                      # exact in binary64: two 24-bit significands
    consts = (0.01 ** 2, 0.03 ** 2)
    r = L.ssim_l1_ref(a, b, 1.0, -1.0, consts=consts)          # lam = 1, up = -1: d mean(SSIM) / d a
    grad, d_mu, d_eaa, d_eab = _autograd_maps(a, b, w2, consts)
    # relative to each value's own terms (d_mu and the gradient cancel towards zero as a -> b)
    for name, mine, want, mag in (("d_mu", r.d_mu, d_mu, r.T_mu), ("d_eaa", r.d_eaa, d_eaa, r.T_eaa), ("d_eab", r.d_eab, d_eab, r.T_eab),
                                  ("grad", r.grad, grad, r.S)):
        err = float(((mine - want).abs() / mag).max())
        assert err < 1e-10, (name, err)


def test_band_is_bit_for_bit_the_full_image():
    a, b = L.smooth_pair(3, 83, 45, 1e-2, seed=5)
    full = L.ssim_l1_ref(a, b)
    yfull = L.yardstick32(a, b)
    for (y0, y1) in ((0, 1), (0, 12), (3, 40), (31, 32), (40, 83), (82, 83), (20, 20), (0, 83)):
        band = L.ssim_l1_ref(a, b, rows=(y0, y1))
        yb = L.yardstick32(a, b, rows=(y0, y1))
        mb, me = band.map_rows
        assert (mb, me) == (max(0, y0 - 5), min(83, y1 + 5))
        for f in ("grad", "ssim_map", "S"):
            assert torch.equal(getattr(band, f), getattr(full, f)[:, y0:y1]), (y0, y1, f)
        for f in ("d_mu", "d_eaa", "d_eab", "T_mu"):
            assert torch.equal(getattr(band, f), getattr(full, f)[:, mb:me]), (y0, y1, f)
        for f in ("grad", "d_mu"):
            sl = slice(y0, y1) if f == "grad" else slice(mb, me)
            assert torch.equal(getattr(yb, f), getattr(yfull, f)[:, sl]), (y0, y1, f)
    f64, _ = L.ref_sums(a, b, band=16)
    assert abs(f64["ssim_sum"] - full.ssim_sum) < 1e-9 and abs(f64["l1_sum"] - full.l1_sum) < 1e-9


# The window gap: the kernel's separable window against the reference's rounded 11x11 one, both in binary64, on a smooth
# 3x256x320 image against its target plus N(0, sigma^2) noise, and on uniform noise.  Measured (|d mean SSIM|,
# max|dg| / max|g|), bounds: measured x 1.25.  At sigma = 0 (a = b) SSIM is 1 and its gradient is zero in both, up to
# binary64 rounding: that case is bounded by a few eps64 (of 1 for the mean, of max S_p for the gradient) instead.
EPS64 = float(np.finfo(np.float64).eps)
WINDOW_GAP = {                 # case: (measured |d mean SSIM|, measured max|dg| / max|g|)
    1e-1: (6.40e-6, 7.89e-5),
    1e-2: (4.53e-6, 1.60e-4),
    1e-3: (5.42e-8, 1.45e-4),
    0.0: (8 * EPS64 / 1.25, 8 * EPS64 / 1.25),        # zero up to rounding; gradient relative to max S_p
    "uniform": (4.78e-7, 9.22e-7),
}


def _gap_pair(case):
    if case == "uniform":
        g = torch.Generator().manual_seed(2)
        return torch.rand(3, 256, 320, generator=g), torch.rand(3, 256, 320, generator=g)
    return L.smooth_pair(3, 256, 320, case, seed=1)


@pytest.mark.parametrize("case", list(WINDOW_GAP))
def test_window_gap_is_pinned(case):
    a, b = _gap_pair(case)
    sep = L.ssim_l1_ref(a, b, window="separable")
    ref = L.ssim_l1_ref(a, b, window="reference")
    dssim = abs(sep.ssim_sum - ref.ssim_sum) / sep.n
    scale = float(sep.S.max()) if case == 0.0 else float(sep.grad.abs().max())
    dg = float((sep.grad - ref.grad).abs().max()) / scale
    print(f"window gap {case}: |d mean SSIM| {dssim:.3g}, max|dg| / {'max S' if case == 0.0 else 'max|g|'} {dg:.3g}")
    want_s, want_g = WINDOW_GAP[case]
    assert dssim <= 1.25 * want_s
    assert dg <= 1.25 * want_g
    # the gap is real where SSIM has a gradient: it is not rounding noise of either evaluation
    if case != 0.0:
        assert dg > 0.1 * want_g


# ---------------------------------------------------------------------------------------------------- planted faults

def _old_bound_holds(dev, ref):
    """test_fused_loss_matches_reference_golden's tensor-wide bound: max|dg| <= 2e-4 max|g|."""
    return float((dev.grad.double() - ref.grad).abs().max()) <= 2e-4 * float(ref.grad.abs().max())


def _fault_input(fault):
    """(a, b, rows, lambda) where each fault has something to act on: ties for the sign fault (a = b on a zero background), uniform noise
    for the map fault (no cancellation hides it), a smooth image with sigma = 1e-2 elsewhere."""
    C, H, W = 3, 70, 100
    if fault == "sign_tie":
        a, b = L.smooth_pair(C, H, W, 1e-2, seed=7)
        a[:, 20:50, 30:80] = 0.0
        b[:, 20:50, 30:80] = 0.0
        a[:, 5:15] = b[:, 5:15]
        return a, b, None, 0.2
    if fault in ("map_ulp", "small_g"):
        g = torch.Generator().manual_seed(8)
        a, b = torch.rand(C, H, W, generator=g), torch.rand(C, H, W, generator=g)
        if fault == "small_g":
            # SSIM alone (the drop-in ssim path): dark low-contrast noise on the top half (B1 B2 near C1 C2: the largest gradients),
            # full-range noise below, where |g| is 1e-3 of that without cancelling
            a[:, :35] = 0.005 * a[:, :35]
            b[:, :35] = 0.005 * b[:, :35]
            return a, b, None, 1.0
        return a, b, None, 0.2
    a, b = L.smooth_pair(C, H, W, 1e-2, seed=9)
    return a, b, ((20, 52) if fault == "slab_halo" else None), 0.2


FAULTS = ["seam_tap", "slab_halo", "small_g", "sign_tie", "map_ulp"]


@pytest.mark.parametrize("fault", FAULTS)
def test_check_loss_names_planted_fault(fault):
    a, b, rows, lam = _fault_input(fault)
    ref = L.ssim_l1_ref(a, b, lam, rows=rows)
    ys = L.yardstick32(a, b, lam, rows=rows)
    L.check_loss(ys, ref, ys, label="clean")                    # the clean yardstick passes its own check
    bad = L.yardstick32(a, b, lam, rows=rows, fault=fault)
    with pytest.raises(AssertionError) as info:
        L.check_loss(bad, ref, ys, label=fault, sums=fault in ("seam_tap",))
    old = _old_bound_holds(bad, ref)
    print(f"{fault}: check_loss fails ({str(info.value)[:160]}...); old tensor-wide 2e-4 bound "
          f"{'MISSES it' if old else 'catches it'}")
    if fault == "small_g":
        assert old, "fault 3 should pass the tensor-wide bound: that is the gap this checker closes"
