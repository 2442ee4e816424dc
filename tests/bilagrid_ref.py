"""Binary64 reference of the bilateral grid for tests/test_bilagrid_ref.py and tests/test_gpu_bilagrid.py: torch's
own grid_sample(mode="bilinear", padding_mode="border", align_corners=True) on the CPU in float64, the affine product, and autograd
for both gradients; the total variation as torch.diff.  A different implementation from the code under test (hand-written taps in
csrc/gsr_bilagrid_math.h), sharing only the rule.

THE ERROR RULE.  |got - ref| <= K u S with u = 2^-24 (half an ulp of binary32 at 1) and S the binary64 sum of the absolute values of
the terms of that output.  K counts roundings; it is derived here, not fitted to any implementation:

  coordinates   fx = (px + 0.5) / W (Gx - 1) takes two roundings of a number below Gx - 1 (three the way torch normalises to
                [-1, 1] and back), so the weight t = fx - floor fx is off by up to 3 (Gx - 1) u; likewise y.  The luma is three
                products and two sums of numbers of size ~1 (5 roundings), clamped, times (L - 1), rounded: up to 8 (L - 1) u on tz.
                A shifted t moves weight from one corner to its neighbour, whatever the weights are, which is why S takes the
                corners UNWEIGHTED: K_coord = 3 (Gx - 1) + 3 (Gy - 1) + 8 (L - 1).
  out           beyond K_coord: 1 - t (1), the product of three factors (2), weight x coefficient (1), the 8-corner sum (7), x the
                colour (1), the 4-term sum (3), and one for the order of factoring: K_out = K_coord + 16.
                S_out[c] = sum_j |in_j| sum_8 |grids[k = 4c + j, corner]|.
  dimage        the first term is as `out` with 3 terms; the luma term adds a difference of levels (1), 12 terms (11), the products
                go_c in_j (1), (L - 1) and the luma weight (2), the branch sum (1): K_dimage = K_coord + 40.
                S_dimage[j] = sum_c |go_c| sum_8 |grids[4c + j]| + gw_j (L - 1) sum_k |go_c in_j| sum_8 |grids[k]|.
  dgrids        a term is w go_c in_j: the weight (K_coord + 3), two products (2), and the sum over the n pixels that reach the node.
                A sum in two levels of sqrt n terms each has depth 2 sqrt n; nothing here asks for less (a running binary32 sum, as
                torch's CPU backward keeps, meets it in practice though not in the worst case): K_dgrids = K_coord + 8 + 2 ceil(sqrt n),
                per node.  S_dgrids = sum over those pixels of |go_c in_j|, unweighted for the reason above.  A pixel whose fz lies
                within FRAGILE of an integer counts for the levels on both sides (binary32 may put it in either cell, with a weight of
                rounding size), so "no pixel reaches the node" (S = 0, gradient exactly 0) holds for any correct rounding.
  tv            value: a difference, a square (2), a sum of n terms in a tree or in blocks (2 ceil(log2 n)), the division and the
                three-term sum (4): K_tv = 6 + 2 ceil(log2 n), S = the value itself (every term is positive).
                gradient: 2 / count (2), times upstream (1), a difference and a product per term (2), six terms (5): K_tvgrad = 10,
                S = |upstream| sum over the element's up to six differences of 2 / count |difference|.

FRAGILE PIXELS.  dimage's luma term jumps where fz is an integer and where the luma crosses 0 or 1; a pixel within FRAGILE = 1e-4 of
either (in binary64) is left out of the dimage comparison when L > 1.  out and dgrids are continuous there and keep it.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
FRAGILE = 1e-4
GRAY = (0.299, 0.587, 0.114)
SHAPES = ((37, 53, 8, 16, 16), (70, 130, 2, 3, 4), (9, 11, 1, 1, 1), (1, 1, 8, 16, 16), (17, 1921, 8, 16, 16), (270, 480, 8, 16, 16))
TV_SHAPES = ((3, 8, 16, 16), (1, 1, 1, 1), (2, 2, 3, 4))
N_IMAGES, IDX = 3, 1


def make_inputs(H, W, L, Gy, Gx, seed=0):
    """grids [3,12,L,Gy,Gx] = identity + 0.3 randn, image [3,H,W] = rand 1.3 - 0.1 (lumas clamp on either side: 0.4 % below 0, 2 % above 1),
    upstream [3,H,W] = randn; float32 CPU tensors."""
    g = torch.Generator().manual_seed(1000 + seed)
    eye = torch.eye(4)[:3].reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * torch.randn(N_IMAGES, 12, L, Gy, Gx, generator=g)).contiguous()
    image = torch.rand(3, H, W, generator=g) * 1.3 - 0.1
    go = torch.randn(3, H, W, generator=g)
    return grids, image, go


def make_tv_grids(N, L, Gy, Gx, seed=0):
    g = torch.Generator().manual_seed(2000 + seed)
    return (torch.eye(4)[:3].reshape(1, 12, 1, 1, 1) + 0.3 * torch.randn(N, 12, L, Gy, Gx, generator=g)).contiguous()


def slice_apply64(grids, image, idx):
    """The rule on float64 tensors."""
    _, H, W = image.shape
    x = ((torch.arange(W, dtype=torch.float64) + 0.5) / W).view(1, W).expand(H, W)
    y = ((torch.arange(H, dtype=torch.float64) + 0.5) / H).view(H, 1).expand(H, W)
    gray = GRAY[0] * image[0] + GRAY[1] * image[1] + GRAY[2] * image[2]
    coords = torch.stack((x, y, gray), -1) * 2.0 - 1.0
    A = F.grid_sample(grids[idx][None], coords[None, None], mode="bilinear", padding_mode="border", align_corners=True)
    A = A.view(3, 4, H, W)
    return (A[:, :3] * image[None]).sum(1) + A[:, 3]


def tv64(grids):
    tv = grids.reshape(-1)[:0].sum()                      # zero, and a function of grids whatever their shape
    for dim in (4, 3, 2):
        if grids.shape[dim] > 1:
            tv = tv + torch.diff(grids, dim=dim).square().mean()
    return tv


def k_coord(L, Gy, Gx):
    return 3 * (Gx - 1) + 3 * (Gy - 1) + 8 * (L - 1)


class Reference:
    """out, dgrids (all N rows), dimage in float64 and the S / K arrays of the error rule, for one seeded case."""

    def __init__(self, H, W, L, Gy, Gx, seed=0, tensors=None):
        """tensors: (grids, image, upstream) float32 CPU tensors of that shape instead of the seeded ones."""
        self.shape = (H, W, L, Gy, Gx)
        self.grids, self.image, self.go = make_inputs(H, W, L, Gy, Gx, seed) if tensors is None else tensors
        g64 = self.grids.double().requires_grad_(True)
        i64 = self.image.double().requires_grad_(True)
        out = slice_apply64(g64, i64, IDX)
        out.backward(self.go.double())
        self.out, self.dgrids, self.dimage = out.detach().numpy(), g64.grad.numpy(), i64.grad.numpy()
        # ---- taps in float64
        img, go, grid = self.image.double().numpy(), self.go.double().numpy(), self.grids[IDX].double().numpy()
        fx = np.broadcast_to(((np.arange(W) + 0.5) / W * (Gx - 1))[None, :], (H, W))
        fy = np.broadcast_to(((np.arange(H) + 0.5) / H * (Gy - 1))[:, None], (H, W))
        gray = GRAY[0] * img[0] + GRAY[1] * img[1] + GRAY[2] * img[2]
        fz = np.clip(gray, 0.0, 1.0) * (L - 1)

        def nodes(f, G):
            i0 = np.clip(np.floor(f), 0, G - 1).astype(np.int64)
            return i0, np.minimum(i0 + 1, G - 1)
        (x0, x1), (y0, y1), (z0, z1) = nodes(fx, Gx), nodes(fy, Gy), nodes(fz, L)
        absg = np.abs(grid)
        G8 = np.zeros((12, H, W))
        for zz in (z0, z1):
            for yy in (y0, y1):
                for xx in (x0, x1):
                    G8 += absg[:, zz, yy, xx]
        in4 = np.concatenate((np.abs(img), np.ones((1, H, W))), 0)
        G8 = G8.reshape(3, 4, H, W)
        self.S_out = (G8 * in4[None]).sum(1)
        term = np.abs(go)[:, None] * in4[None]                                             # |go_c in_j|  [3,4,H,W]
        luma = (G8 * term).sum((0, 1)) * (L - 1)
        self.S_dimage = (G8[:, :3] * np.abs(go)[:, None]).sum(0) + np.asarray(GRAY)[:, None, None] * luma[None]
        self.K_out, self.K_dimage = k_coord(L, Gy, Gx) + 16, k_coord(L, Gy, Gx) + 40
        near = (np.abs(fz - np.round(fz)) < FRAGILE) & (gray > 0.0) & (gray < 1.0)      # (a clamped luma sits ON a level, with no luma term)
        self.fragile = (near | (np.abs(gray) < FRAGILE) | (np.abs(gray - 1.0) < FRAGILE)) if L > 1 else np.zeros((H, W), bool)
        # ---- S and n of dgrids: the pixels that reach a node (levels on both sides of a near-integer fz)
        zlo = np.clip(np.floor(fz - FRAGILE), 0, L - 1).astype(np.int64)
        zhi = np.minimum(np.clip(np.floor(fz + FRAGILE), 0, L - 1).astype(np.int64) + 1, L - 1)
        lev = np.arange(L)[:, None, None]
        member = ((lev >= zlo[None]) & (lev <= zhi[None])).reshape(L, H * W).T.astype(np.float64)      # [HW, L]
        t12 = torch.from_numpy(np.ascontiguousarray(term.reshape(12, H * W).T))                       # [HW, 12]
        vals = torch.cat((torch.from_numpy(member)[:, :, None] * t12[:, None, :], torch.from_numpy(member)[:, :, None]), 2)      # [HW, L, 13]
        acc = torch.zeros(Gy * Gx, L, 13, dtype=torch.float64)
        for yy, ydup in ((y0, None), (y1, y1 == y0)):
            for xx, xdup in ((x0, None), (x1, x1 == x0)):
                keep = np.ones((H, W), bool)
                for dup in (ydup, xdup):
                    if dup is not None:
                        keep &= ~dup
                idx = torch.from_numpy((yy * Gx + xx).reshape(-1))
                acc.index_add_(0, idx, vals * torch.from_numpy(keep.reshape(-1, 1, 1).astype(np.float64)))
        acc = acc.numpy().reshape(Gy, Gx, L, 13)
        self.S_dgrids = np.ascontiguousarray(acc[..., :12].transpose(3, 2, 0, 1))               # [12, L, Gy, Gx]
        self.n_dgrids = np.ascontiguousarray(np.broadcast_to(acc[..., 12].transpose(2, 0, 1)[None], (12, L, Gy, Gx)))
        self.K_dgrids = k_coord(L, Gy, Gx) + 8 + 2 * np.ceil(np.sqrt(self.n_dgrids))
        self.untouched = self.n_dgrids == 0


_cache = {}


def reference(shape, seed=0) -> Reference:
    """Computed once per case and shared by the tests; nothing writes to it."""
    key = (tuple(shape), seed)
    if key not in _cache:
        _cache[key] = Reference(*shape, seed=seed)
    return _cache[key]


def worst(got, ref, S, K, mask=None):
    """max |got - ref| / (K u S) over the elements (of `mask`); where S is 0, got must equal ref exactly (counted as 0 or inf)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    S, K = np.broadcast_to(S, ref.shape), np.broadcast_to(np.asarray(K, np.float64), ref.shape)
    err, bound = np.abs(got - ref), K * U * S
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    if mask is not None:
        ratio = ratio[np.broadcast_to(mask, ratio.shape)]
    return float(ratio.max()) if ratio.size else 0.0


def check_slice(ref: Reference, out, dgrids_idx, dimage, label):
    """Holds the three outputs of one case to the rule; prints and returns the worst error in units of the bound."""
    w = {}
    if out is not None:
        w["out"] = worst(out, ref.out, ref.S_out, ref.K_out)
    if dgrids_idx is not None:
        w["dgrids"] = worst(dgrids_idx, ref.dgrids[IDX], ref.S_dgrids, ref.K_dgrids)
        assert not np.asarray(dgrids_idx)[ref.untouched].any(), f"{label}: a node no pixel reaches has a gradient"
    if dimage is not None:
        keep = ~ref.fragile
        share = 1.0 - keep.mean()
        assert share <= 0.01, f"{label}: {share:.2%} of the pixels are fragile"
        w["dimage"] = worst(dimage, ref.dimage, ref.S_dimage, ref.K_dimage, keep[None])
    print(f"{label}: worst error x the bound: " + ", ".join(f"{k} {v:.3f}" for k, v in w.items()))
    for k, v in w.items():
        assert v <= 1.0, f"{label}: {k} misses its bound by a factor of {v:.3f}"
    return w


class TvReference:
    def __init__(self, N, L, Gy, Gx, upstream=3.7, seed=0):
        self.grids, self.upstream = make_tv_grids(N, L, Gy, Gx, seed), upstream
        g64 = self.grids.double().requires_grad_(True)
        tv = tv64(g64)
        (tv * upstream).backward()
        self.value, self.grad = float(tv.detach()), g64.grad.numpy()
        n = self.grids.numel()
        self.K_value, self.S_value = 6 + 2 * math.ceil(math.log2(max(n, 2))), self.value
        S = np.zeros(self.grids.shape)
        g = self.grids.double().numpy()
        for dim in (4, 3, 2):
            if g.shape[dim] > 1:
                d = np.abs(np.diff(g, axis=dim)) * (2.0 / (g.size // g.shape[dim] * (g.shape[dim] - 1)))
                lo = [slice(None)] * 5
                hi = [slice(None)] * 5
                lo[dim], hi[dim] = slice(0, -1), slice(1, None)
                S[tuple(lo)] += d
                S[tuple(hi)] += d
        self.K_grad, self.S_grad = 10, S * abs(upstream)


def tv_reference(shape, seed=0) -> TvReference:
    key = ("tv", tuple(shape), seed)
    if key not in _cache:
        _cache[key] = TvReference(*shape, seed=seed)
    return _cache[key]


def check_tv(ref: TvReference, value, grad, label):
    wv = worst(np.array([value]), np.array([ref.value]), np.array([ref.S_value]), ref.K_value)
    wg = worst(grad, ref.grad, ref.S_grad, ref.K_grad)
    print(f"{label}: worst error x the bound: value {wv:.3f}, gradient {wg:.3f}")
    assert wv <= 1.0 and wg <= 1.0, f"{label}: value {wv:.3f}, gradient {wg:.3f} x the bound"
    return wv, wg
