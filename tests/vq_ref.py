"""Float64 numpy reference of the vector-quantisation kernels (csrc/gsr_vq.hip, diff_gaussian_rasterization/vq.py), the fixtures of
their tests and the rules those tests hold them to.  DESIGN.md section 18 derives the bounds.

B(p) = (D + 4) 2^-24 (|x_p| + max_k |c_k|)^2 bounds the binary32 evaluation |x|^2 + (|c|^2 - 2 x.c) of one squared distance: the
three D-term fmaf chains (dot product and the two norms) err by at most D 2^-24 (2 |x||c| + |c|^2 + |x|^2) together, every partial
sum of a chain being bounded by the product of the norms, and the two combining operations by 2^-24 (|x| + |c|)^2 each: (D + 2)
roundings' worth, with 2 to spare for the second-order terms.
"""
import numpy as np

U = 2.0 ** -24


def fixture(P, K, D):
    """x [P,D] and codebook [K,D]: i.i.d. standard normal from default_rng(1000 D + K), rounded to float32."""
    rng = np.random.default_rng(1000 * D + K)
    return rng.standard_normal((P, D)).astype(np.float32), rng.standard_normal((K, D)).astype(np.float32)


def blobs(K=16, n=50, D=3, spread=0.01, seed=7):
    """K blobs of n points with the given spread around the points of a unit-spaced 4 x ... grid, shuffled -> (x float32 [K n, D],
    label [K n], init [K]: the first point of every blob)."""
    rng = np.random.default_rng(seed)
    centres = np.stack([(np.arange(K) // 4 ** a) % 4 for a in range(D)], 1).astype(np.float64)
    assert len({tuple(c) for c in centres}) == K
    label = rng.permutation(np.repeat(np.arange(K), n))
    x = (centres[label] + spread * rng.standard_normal((K * n, D))).astype(np.float32)
    init = np.array([int(np.flatnonzero(label == k)[0]) for k in range(K)])
    return x, label, init


def sqdist(x, c):
    """Row-wise |x_p - c_p|^2 in float64, from the differences."""
    d = x.astype(np.float64) - c.astype(np.float64)
    return (d * d).sum(1)


def bound(x, cb):
    """B(p), float64 [P]."""
    D = x.shape[1]
    xn = np.sqrt((x.astype(np.float64) ** 2).sum(1))
    cmax = np.sqrt((cb.astype(np.float64) ** 2).sum(1)).max()
    return (D + 4) * U * (xn + cmax) ** 2


class Assign:
    """Brute force over all (point, code) pairs in float64: idx (argmin at the lowest index), dmin, gap (second best - best; inf
    for K == 1) and B.  The P x K distances are the expansion |x|^2 + |c|^2 - 2 x.c evaluated in float64, whose own error is 2^-29
    of B; dmin is recomputed from the differences."""

    def __init__(self, x, cb):
        self.x, self.cb = x, cb
        x64, c64 = x.astype(np.float64), cb.astype(np.float64)
        P, K = x.shape[0], cb.shape[0]
        cn = (c64 * c64).sum(1)
        self.idx = np.zeros(P, np.int64)
        self.gap = np.full(P, np.inf)
        for b in range(0, P, 4096):
            xs = x64[b:b + 4096]
            d = (xs * xs).sum(1)[:, None] + cn[None] - 2.0 * xs @ c64.T
            j = d.argmin(1)
            self.idx[b:b + 4096] = j
            if K > 1:
                best = d[np.arange(len(j)), j].copy()
                d[np.arange(len(j)), j] = np.inf
                self.gap[b:b + 4096] = d.min(1) - best
        self.dmin = sqdist(x, cb[self.idx]) if P else np.zeros(0)
        self.B = bound(x, cb) if P else np.zeros(0)

    def check(self, idx, dist2, index_rule=True):
        """The distance rule for every point, the index rule where the float64 gap exceeds 4 B -> the fraction of points the index
        rule leaves out."""
        idx, dist2 = np.asarray(idx), np.asarray(dist2, np.float64)
        P, K = self.x.shape[0], self.cb.shape[0]
        assert idx.shape == (P,) and dist2.shape == (P,)
        if P == 0:
            return 0.0
        assert idx.min() >= 0 and idx.max() < K
        dj = sqdist(self.x, self.cb[idx])
        worst = ((dj - self.dmin) / self.B).max()
        assert (dj <= self.dmin + 2 * self.B).all(), f"chosen code is {worst:.2f} B above the minimum"
        err = np.abs(dist2 - dj) / self.B
        assert (err <= 1).all(), f"dist2 is {err.max():.2f} B from the distance to the chosen code"
        assert (dist2 >= 0).all()
        if not index_rule:
            return 0.0
        clear = self.gap > 4 * self.B
        assert (idx[clear] == self.idx[clear]).all(), f"{int((idx[clear] != self.idx[clear]).sum())} clear points got another code"
        left_out = 1.0 - clear.mean()
        print(f"P={P} K={K} D={self.x.shape[1]}: chosen code at most {worst:.3f} B above the minimum, dist2 within {err.max():.3f} B, "
              f"index rule leaves out {100 * left_out:.3f} %")
        assert left_out <= 0.01
        return left_out


def means(x, idx, cb):
    """-> (codebook float64 [K,D]: per-code means, previous row where empty; counts int64 [K]; bound float64 [K,D]:
    n_j 2^-23 max over the members of |x_i| per column: n_j - 1 adds in any fixed order and the division, each within 2^-24 of a
    value no larger than the column's maximum, with a factor 2 to spare)."""
    K, D = cb.shape
    idx = np.asarray(idx, np.int64)
    counts = np.bincount(idx, minlength=K)
    sums = np.zeros((K, D))
    np.add.at(sums, idx, x.astype(np.float64))
    amax = np.zeros((K, D))
    np.maximum.at(amax, idx, np.abs(x.astype(np.float64)))
    out = np.where(counts[:, None] > 0, sums / np.maximum(counts, 1)[:, None], cb.astype(np.float64))
    return out, counts, counts[:, None] * 2.0 ** -23 * amax


def check_update(x, idx, cb, new_cb, counts):
    want, n, tol = means(x, idx, cb)
    new_cb, counts = np.asarray(new_cb), np.asarray(counts)
    assert counts.dtype == np.int32 and np.array_equal(counts, n)
    assert new_cb.dtype == np.float32 and new_cb.shape == cb.shape
    empty = n == 0
    assert np.array_equal(new_cb[empty].view(np.uint32), cb[empty].view(np.uint32)), "an empty code's row changed"
    err = np.abs(new_cb.astype(np.float64) - want)
    assert (err <= tol).all(), f"mean off by {np.max(err / np.maximum(tol, 1e-300)):.2f} bounds"


def objective(x, cb, idx):
    return float(sqdist(x, cb[np.asarray(idx, np.int64)]).sum())
