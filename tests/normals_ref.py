"""Binary64 restatement of the normal-map ops (diff_gaussian_rasterization/normals.py, csrc/gsr_normals_math.h),
in an independent form, and their error rule.

Values.  depth normals: every pixel is back-projected, P = (px z / fx, py z / fy, z); central differences of P, an explicit cross
product dP/dy x dP/dx and a normalise; the gradients are binary64 autograd's.  Gaussians: numpy's argmin (first of equals), the whole
rotation matrix of the normalised quaternion in binary64, its column, the facing test and the view rotation.  Every decision that is
piecewise constant - validity (alpha >= alpha_min, depth > 0), the argmin and its ties - is taken on the binary32 input values
themselves (alpha_min as the binary32 number the kernels compare with), so no pixel and no axis choice is fragile.  The facing test
can differ in binary32: the Gaussians whose |<n_w, mean - campos>| is within the rounding bound of that very dot product are reported
as fragile and compared up to sign.

Error rule.  A first-order running error analysis of the kernel as written: `Tracked` carries a binary64 value and a bound of the
absolute error its binary32 counterpart has, and every operation of csrc/gsr_normals_math.h is replayed on it in the kernel's order.
An add, subtract or multiply adds u |result| (u = 2^-24, one rounding); a division or square root adds 2 u |result| (one ulp: covers
an implementation that is faithfully but not correctly rounded); a product with a power of two, a negation and a selection add
nothing; incoming errors propagate with the operation's first derivatives.  A fused multiply-add has one rounding where the pair
counted here has two, so contraction only tightens.  The inputs are exact.  Nothing here comes from what the code under test gives.
"""
import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
ALPHA_MIN = float(np.float32(1.0 / 255.0))
LOSS_MAX_BLOCKS = 1024        # csrc/gsr_normals.hip kNrmMaxBlocks: the loss forward's blocks, each walking ceil(tiles / 1024) tiles of 64 x 16


def loss_adds(H, W):
    """Additions a pixel's term passes through in binary32 (csrc/gsr_normals.hip): 4 per tile a thread walks, 6 wave levels, 4 waves."""
    tiles = -(-W // 64) * -(-H // 16)
    return 4 * max(1, -(-tiles // LOSS_MAX_BLOCKS)) + 6 + 4


class Tracked:
    """A binary64 value `v` and a first-order bound `e` of the absolute error of its binary32 counterpart."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64)

    @staticmethod
    def of(x):
        return x if isinstance(x, Tracked) else Tracked(x)

    @staticmethod
    def _rounded(v, e, roundings=1):
        return Tracked(v, e + roundings * U * v.abs())

    def __add__(self, o):
        o = Tracked.of(o)
        return Tracked._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Tracked.of(o)
        return Tracked._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Tracked.of(o)
        return Tracked._rounded(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e)

    def __truediv__(self, o):
        o = Tracked.of(o)
        return Tracked._rounded(self.v / o.v, self.e / o.v.abs() + self.v.abs() * o.e / o.v.square(), 2)

    def __neg__(self):
        return Tracked(-self.v, self.e)

    def sqrt(self):
        r = self.v.sqrt()
        return Tracked._rounded(r, self.e / (2 * r), 2)

    def pow2(self, c):
        """Times a power of two: exact."""
        return Tracked(self.v * c, self.e * abs(c))

    def where(self, mask, other):
        other = Tracked.of(other)
        return Tracked(torch.where(mask, self.v, other.v), torch.where(mask, self.e, other.e))

    def __getitem__(self, idx):
        return Tracked(self.v[idx], self.e[idx])


def _pad(t, H, W):
    """An interior [..., H-2, W-2] array inside zeros [..., H, W]."""
    if isinstance(t, Tracked):
        return Tracked(_pad(t.v, H, W), _pad(t.e, H, W))
    return torch.nn.functional.pad(t, (1, 1, 1, 1))


def _shift(t, dy, dx):
    """out[y, x] = t[y + dy, x + dx], zero where that is outside."""
    if isinstance(t, Tracked):
        return Tracked(_shift(t.v, dy, dx), _shift(t.e, dy, dx))
    H, W = t.shape
    out = torch.zeros_like(t)
    ys, yd = (slice(dy, H), slice(0, H - dy)) if dy >= 0 else (slice(0, H + dy), slice(-dy, H))
    xs, xd = (slice(dx, W), slice(0, W - dx)) if dx >= 0 else (slice(0, W + dx), slice(-dx, W))
    out[yd, xd] = t[ys, xs]
    return out


# ---- depth normals -------------------------------------------------------------------------------------------------------------------

def valid_mask(depth32, alpha32, alpha_min=ALPHA_MIN):
    """On the binary32 values themselves."""
    return (alpha32 >= np.float32(alpha_min)) & (depth32 > np.float32(0))


def normal_mask(valid):
    """The pixels that have a depth normal: interior, four valid axis neighbours."""
    H, W = valid.shape
    ok = np.zeros((H, W), bool)
    if H >= 3 and W >= 3:
        ok[1:-1, 1:-1] = valid[1:-1, :-2] & valid[1:-1, 2:] & valid[:-2, 1:-1] & valid[2:, 1:-1]
    return ok


def depth_to_normal_ref(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN, valid=None):
    """depth, alpha: binary64 tensors [H,W] (leaves, for autograd) holding binary32 values -> n [3,H,W], by back-projection, central
    differences, a cross product and a normalise."""
    H, W = depth.shape
    if valid is None:
        valid = valid_mask(depth.detach().numpy().astype(np.float32), alpha.detach().numpy().astype(np.float32), alpha_min)
    ok = torch.from_numpy(normal_mask(valid))
    validt = torch.from_numpy(valid)
    if H < 3 or W < 3:
        return torch.zeros(3, H, W, dtype=F64) + 0 * (depth.sum() + alpha.sum())
    one = torch.ones_like(depth)
    z = torch.where(validt, depth, one) / torch.where(validt, alpha, one)
    fx, fy = W / (2.0 * tanfovx), H / (2.0 * tanfovy)
    xs = (torch.arange(W, dtype=F64) + 0.5 - W / 2).view(1, W)
    ys = (torch.arange(H, dtype=F64) + 0.5 - H / 2).view(H, 1)
    P = torch.stack((xs * z / fx, ys * z / fy, z))
    dPdx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dPdy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    c = torch.cross(dPdy, dPdx, dim=0)
    n = c / c.norm(dim=0, keepdim=True)
    return _pad(torch.where(ok[1:-1, 1:-1][None], n, torch.zeros_like(n)), H, W)


def normal_consistency_ref(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN):
    """The composed form: depth_to_normal_ref and the plain loss, alpha detached as a factor."""
    n = depth_to_normal_ref(depth, alpha, tanfovx, tanfovy, alpha_min)
    return (1 - alpha.detach() * (normal_map * n).sum(0)).mean()


def closed_form(depth, alpha, tanfovx, tanfovy, alpha_min=ALPHA_MIN):
    """The kernel's closed form in binary64 (the values of the tracked replay): held to the cross product in tests/test_normals_ref.py."""
    return depth_normal_tracked(depth, alpha, tanfovx, tanfovy, alpha_min)["n"].v


def depth_normal_tracked(depth32, alpha32, tanfovx, tanfovy, alpha_min=ALPHA_MIN, grad_n=None, normal_map=None, grad_loss=None):
    """The replay of the kernels on [H,W] arrays of binary32 values: {"n": Tracked [3,H,W]} and, with grad_n [3,H,W] (depth_to_normal's
    backward) or with normal_map and grad_loss (the loss: also "loss", "dN"), {"ddepth", "dalpha"}: Tracked [H,W].  The bound is `.e`;
    where a result must be zero, value and bound are zero."""
    d = torch.as_tensor(np.asarray(depth32), dtype=F64)
    a = torch.as_tensor(np.asarray(alpha32), dtype=F64)
    H, W = d.shape
    valid = valid_mask(d.numpy().astype(np.float32), a.numpy().astype(np.float32), alpha_min)
    validt, ok = torch.from_numpy(valid), torch.from_numpy(normal_mask(valid))
    zero = Tracked(torch.zeros(H, W, dtype=F64))
    out = {}
    if H < 3 or W < 3:
        out["n"] = Tracked(torch.zeros(3, H, W, dtype=F64))
        if grad_n is not None or normal_map is not None:
            out["ddepth"], out["dalpha"] = zero, zero
        if normal_map is not None:
            out["dN"] = Tracked(torch.zeros(3, H, W, dtype=F64))
            out["loss"] = Tracked(torch.ones((), dtype=F64), torch.as_tensor((loss_adds(H, W) + 2) * U, dtype=F64)) if H * W else None
        return out
    one = torch.ones_like(d)
    z = Tracked(torch.where(validt, d, one)) / Tracked(torch.where(validt, a, one))
    fx = Tracked(float(W)) / Tracked(2.0 * tanfovx)              # (float)W / (2.f * tanfovx): the product with 2 is exact
    fy = Tracked(float(H)) / Tracked(2.0 * tanfovy)
    px = Tracked((torch.arange(1, W - 1, dtype=F64) + 0.5 - 0.5 * W).view(1, W - 2))
    py = Tracked((torch.arange(1, H - 1, dtype=F64) + 0.5 - 0.5 * H).view(H - 2, 1))
    zl, zr, zu, zd = z[1:-1, :-2], z[1:-1, 2:], z[:-2, 1:-1], z[2:, 1:-1]
    Dx, Sx, Dy, Sy = zr - zl, zr + zl, zd - zu, zd + zu
    # nrm_normal_one
    pa, pb = Sy * Dx, Sx * Dy
    m0, m1, m2 = fx * pa, fy * pb, -(Sx * Sy + px * pa + py * pb)
    inv = Tracked(1.0) / (m0 * m0 + m1 * m1 + m2 * m2).sqrt()
    n = [m0 * inv, m1 * inv, m2 * inv]
    oki = ok[1:-1, 1:-1]
    out["n"] = Tracked(torch.stack([_pad(torch.where(oki, c.v, 0 * c.v), H, W) for c in n]),
                       torch.stack([_pad(torch.where(oki, c.e, 0 * c.e), H, W) for c in n]))
    if grad_n is None and normal_map is None:
        return out
    ai = Tracked(a[1:-1, 1:-1])
    if normal_map is not None:
        Nm = torch.as_tensor(np.asarray(normal_map), dtype=F64)[:, 1:-1, 1:-1]
        inv_hw = Tracked(1.0 / (H * W), U / (H * W))           # (float)(1.0 / (H W))
        scale = -(Tracked(float(grad_loss)) * inv_hw)
        s = ai * scale
        g = [Tracked(Nm[c]) * s for c in range(3)]
        dN = [s * n[c] for c in range(3)]
        out["dN"] = Tracked(torch.stack([_pad(torch.where(oki, c.v, 0 * c.v), H, W) for c in dN]),
                            torch.stack([_pad(torch.where(oki, c.e, 0 * c.e), H, W) for c in dN]))
        # the forward: per-pixel terms, loss_adds binary32 additions each, the blocks' sums in binary64, two roundings at the end
        dot = Tracked(Nm[0]) * n[0] + Tracked(Nm[1]) * n[1] + Tracked(Nm[2]) * n[2]
        term = Tracked(1.0) - ai * dot
        tv = _pad(torch.where(oki, term.v, one[1:-1, 1:-1]), H, W)
        tv[~ok] = 1.0
        te = _pad(torch.where(oki, term.e, 0 * term.e), H, W)
        loss = tv.sum() / (H * W)
        out["terms"] = Tracked(tv, te)
        out["loss"] = Tracked(loss, (te.sum() + loss_adds(H, W) * U * tv.abs().sum()) / (H * W) + 2 * U * loss.abs())
    else:
        gn = torch.as_tensor(np.asarray(grad_n), dtype=F64)[:, 1:-1, 1:-1]
        g = [Tracked(gn[c]) for c in range(3)]
    # nrm_normal_backward_one
    dot = n[0] * g[0] + n[1] * g[1] + n[2] * g[2]
    gm0, gm1, gm2 = (g[0] - n[0] * dot) * inv, (g[1] - n[1] * dot) * inv, (g[2] - n[2] * dot) * inv
    gDx, gDy = Sy * (gm0 * fx - gm2 * px), Sx * (gm1 * fy - gm2 * py)
    gSx = gm1 * fy * Dy - gm2 * (Sy + py * Dy)
    gSy = gm0 * fx * Dx - gm2 * (Sx + px * Dx)
    takes = [gSx - gDx, gSx + gDx, gSy - gDy, gSy + gDy]                     # of (left, right, up, down)
    takes = [_pad(t.where(oki, 0.0), H, W) for t in takes]
    # nrm_gather: the left neighbour's take of its right depth, the right's of its left, the upper's of its lower, the lower's of its upper
    gz = Tracked(torch.zeros(H, W, dtype=F64))
    for t, dy, dx in ((takes[1], 0, -1), (takes[0], 0, 1), (takes[3], -1, 0), (takes[2], 1, 0)):
        gz = gz + _shift(t, dy, dx)
    # nrm_chain
    zt, at = z, Tracked(torch.where(validt, a, one))
    gd = gz / at
    ga = Tracked(0.0) - (gz * zt) / at
    out["ddepth"], out["dalpha"] = gd.where(validt, 0.0), ga.where(validt, 0.0)
    return out


# ---- Gaussians -----------------------------------------------------------------------------------------------------------------------

def rotation_matrix(q):
    """upstream's build_rotation of q / |q|, [P,3,3], in q's dtype."""
    u = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = u.unbind(1)
    return torch.stack((1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)), 1).view(-1, 3, 3)


def gaussian_normals_ref(scales32, rotations, means32, viewmatrix32, campos32):
    """scales32 / means32 / viewmatrix32 / campos32: numpy binary32; rotations: a binary64 tensor [P,4] (a leaf, for autograd) ->
    (normals [P,3] binary64, k [P], flipped [P] bool)."""
    P = scales32.shape[0]
    k = torch.from_numpy(np.argmin(scales32, axis=1).astype(np.int64)) if P else torch.zeros(0, dtype=torch.int64)
    R = rotation_matrix(rotations)
    n_w = R[torch.arange(P), :, k]
    d = torch.as_tensor(means32.astype(np.float64) - campos32.astype(np.float64).reshape(1, 3))
    flipped = (n_w.detach() * d).sum(1) > 0
    n_w = torch.where(flipped[:, None], -n_w, n_w)
    V = torch.as_tensor(viewmatrix32.astype(np.float64))
    return n_w @ V[:3, :3], k, flipped


def _column(u, k):
    """nrm_rotation_column on Tracked components."""
    r, x, y, z = u
    one = Tracked(1.0)
    if k == 0:
        return [one - (y * y + z * z).pow2(2), (x * y + r * z).pow2(2), (x * z - r * y).pow2(2)]
    if k == 1:
        return [(x * y - r * z).pow2(2), one - (x * x + z * z).pow2(2), (y * z + r * x).pow2(2)]
    return [(x * z + r * y).pow2(2), (y * z - r * x).pow2(2), one - (x * x + y * y).pow2(2)]


def _column_backward(u, k, gc):
    """nrm_rotation_column_backward on Tracked components."""
    r, x, y, z = u
    if k == 0:
        return [(z * gc[1] - y * gc[2]).pow2(2), (y * gc[1] + z * gc[2]).pow2(2),
                (x * gc[1] - r * gc[2]).pow2(2) - y.pow2(4) * gc[0], (r * gc[1] + x * gc[2]).pow2(2) - z.pow2(4) * gc[0]]
    if k == 1:
        return [(x * gc[2] - z * gc[0]).pow2(2), (y * gc[0] + r * gc[2]).pow2(2) - x.pow2(4) * gc[1],
                (x * gc[0] + z * gc[2]).pow2(2), (y * gc[2] - r * gc[0]).pow2(2) - z.pow2(4) * gc[1]]
    return [(y * gc[0] - x * gc[1]).pow2(2), (z * gc[0] - r * gc[1]).pow2(2) - x.pow2(4) * gc[2],
            (r * gc[0] + z * gc[1]).pow2(2) - y.pow2(4) * gc[2], (x * gc[0] + y * gc[1]).pow2(2)]


def gaussian_normals_tracked(scales32, rotations32, means32, viewmatrix32, campos32, grad_out32=None):
    """The replay of nrm_gaussian_forward_one / _backward_one: {"out": Tracked [P,3], "fragile": bool [P]} and, with grad_out32,
    {"dq": Tracked [P,4]}.  fragile: |<n_w, mean - campos>| in binary64 is within the bound of the binary32 dot product."""
    P = scales32.shape[0]
    k = torch.from_numpy(np.argmin(scales32, axis=1).astype(np.int64)) if P else torch.zeros(0, dtype=torch.int64)
    q = [Tracked(torch.as_tensor(rotations32[:, i].astype(np.float64))) for i in range(4)]
    inv_len = Tracked(1.0) / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]).sqrt()
    u = [c * inv_len for c in q]
    cols = [_column(u, j) for j in range(3)]
    nw = [cols[0][i].where(k == 0, cols[1][i].where(k == 1, cols[2][i])) for i in range(3)]
    mean = [Tracked(torch.as_tensor(means32[:, i].astype(np.float64))) for i in range(3)]
    cam = [float(c) for c in campos32.reshape(3)]
    dot = nw[0] * (mean[0] - cam[0]) + nw[1] * (mean[1] - cam[1]) + nw[2] * (mean[2] - cam[2])
    sign = torch.where(dot.v > 0, -1.0, 1.0).to(F64)
    nw = [Tracked(c.v * sign, c.e) for c in nw]
    V = viewmatrix32.astype(np.float64)
    out = [nw[0] * float(V[0, j]) + nw[1] * float(V[1, j]) + nw[2] * float(V[2, j]) for j in range(3)]
    res = {"out": Tracked(torch.stack([c.v for c in out], 1), torch.stack([c.e for c in out], 1)),
           "fragile": dot.v.abs() <= dot.e, "k": k, "sign": sign}
    if grad_out32 is None:
        return res
    g = [Tracked(torch.as_tensor(grad_out32[:, j].astype(np.float64))) for j in range(3)]
    gc = [Tracked(sign) * (g[0] * float(V[i, 0]) + g[1] * float(V[i, 1]) + g[2] * float(V[i, 2])) for i in range(3)]
    gus = [_column_backward(u, j, gc) for j in range(3)]
    gu = [gus[0][i].where(k == 0, gus[1][i].where(k == 1, gus[2][i])) for i in range(4)]
    d2 = u[0] * gu[0] + u[1] * gu[1] + u[2] * gu[2] + u[3] * gu[3]
    dq = [(gu[i] - u[i] * d2) * inv_len for i in range(4)]
    res["dq"] = Tracked(torch.stack([c.v for c in dq], 1), torch.stack([c.e for c in dq], 1))
    return res


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

TANFOV = (float(np.float32(0.8)), float(np.float32(0.45)))
MAP_SIZES = ((1, 1), (2, 2), (2, 5), (3, 3), (5, 5), (17, 33), (37, 70), (64, 256))          # H x W
MAP_FORMS = ("smooth", "holes", "step")


def make_maps(H, W, form, seed=0):
    """(depth, alpha) binary32 [H,W].  smooth: a curved surface under a varying alpha; holes: alpha under alpha_min at isolated pixels,
    in a 2 x 2 block, along a whole row and in the second and second-to-last columns, one pixel at alpha_min exactly (valid) and one
    at depth 0 (invalid); step: a depth step down the middle."""
    rng = np.random.default_rng(1000 * H + W + 7 * seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    z = 3.0 + 0.5 * np.sin(0.31 * x + 0.1) + 0.4 * np.cos(0.23 * y) + 0.01 * x + 0.05 * rng.random((H, W))
    if form == "step":
        z = z + 2.0 * (x >= W // 2)
    alpha = (0.6 + 0.3 * np.sin(0.17 * x + 0.4 * y) + 0.05 * rng.random((H, W))).astype(np.float32)
    hole = np.float32(0.5 * ALPHA_MIN)
    depth = None
    if form == "holes":
        for _ in range(max(1, H * W // 40)):
            alpha[rng.integers(H), rng.integers(W)] = hole
        if H >= 6 and W >= 6:
            alpha[H // 3:H // 3 + 2, W // 3:W // 3 + 2] = hole
            alpha[H // 2 + 1, :] = hole
        if W >= 7:
            alpha[:, 1] = hole
            alpha[:, W - 2] = hole
        if H >= 5 and W >= 5:
            alpha[H - 2, W // 2] = np.float32(ALPHA_MIN)            # exactly the cut-off: valid
    depth = (z.astype(np.float32) * alpha).astype(np.float32)
    if form == "holes" and H >= 5 and W >= 5:
        depth[1, W // 2] = 0.0                                          # depth 0: invalid
    return depth, alpha


def make_upstream(H, W, seed=1):
    """(grad_n, normal_map) binary32 [3,H,W], components of both signs."""
    rng = np.random.default_rng(77 * H + W + seed)
    return rng.standard_normal((3, H, W)).astype(np.float32), (0.8 * rng.standard_normal((3, H, W))).astype(np.float32)


GAUSSIAN_SIZES = (0, 1, 63, 64, 65, 1000)
GAUSSIAN_SEED = 5


def make_camera(seed=GAUSSIAN_SEED):
    """(viewmatrix [4,4], campos [3]) binary32: a posed camera, row-vector convention."""
    rng = np.random.default_rng(seed)
    q = rng.standard_normal(4)
    R = rotation_matrix(torch.as_tensor(q[None]))[0].numpy()
    campos = rng.standard_normal(3) * 2.0
    V = np.eye(4)
    V[:3, :3] = R
    V[3, :3] = -campos @ R
    return V.astype(np.float32), campos.astype(np.float32)


def make_gaussians(P, log_scales=False, unit=False, seed=GAUSSIAN_SEED):
    """(scales, rotations, means, grad_out) binary32: random Gaussians around the origin, on both sides of facing; rows 0 .. 5 (where
    there are that many) carry two- and three-way ties of the scales."""
    rng = np.random.default_rng(seed + 13 * P)
    s = np.exp(rng.uniform(-4.0, 0.0, (P, 3)))
    ties = ((0, 1), (1, 2), (0, 2), (0, 1, 2), (1, 2), (0, 1))
    for i, t in enumerate(ties[:P]):
        s[i, list(t)] = s[i].min() * (1.0 if i % 2 == 0 else 0.5)
        if i % 2 == 0:
            others = [j for j in range(3) if j not in t]
            s[i, others] = s[i, list(t)][0] * 2.0
    s = s.astype(np.float32)
    if log_scales:
        s = np.log(s).astype(np.float32)
        for i, t in enumerate(ties[:P]):                                 # the logarithm's rounding must not undo a tie
            s[i, list(t)] = s[i, t[0]]
    q = rng.standard_normal((P, 4)) * np.exp(rng.uniform(-1.0, 1.0, (P, 1)))
    if unit:
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
    means = rng.standard_normal((P, 3)) * 3.0
    g = rng.standard_normal((P, 3))
    return s, q.astype(np.float32), means.astype(np.float32), g.astype(np.float32)


def exact_gaussians():
    """Small-integer cases whose every operation is exact in binary32: the identity quaternion (R = I), integer means and camera.
    -> (scales, rotations, means, viewmatrix, campos, expected normals).  Row 0: the dot is exactly 0 (no flip); row 1: positive
    (flips); row 2: negative (stays); rows 3, 4: a two-way and a three-way tie take the lowest axis."""
    scales = np.array([[1, 2, 3], [3, 1, 2], [2, 3, 1], [2, 1, 1], [1, 1, 1]], np.float32)
    rot = np.tile(np.array([[1, 0, 0, 0]], np.float32), (5, 1))
    campos = np.array([1, 2, 3], np.float32)
    means = np.array([[1, 5, 7], [4, 5, 0], [0, 0, 1], [0, 2, 9], [1, 0, 0]], np.float32)
    V = np.eye(4, dtype=np.float32)
    V[:3, :3] = np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float32)
    V[3, :3] = -campos @ V[:3, :3]
    # k = 0, 1, 2, 1, 0; n_w = e_k; dots: 0, 3, -2, 0, 0
    n_w = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float32)
    return scales, rot, means, V, campos, n_w @ V[:3, :3]
