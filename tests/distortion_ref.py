"""Binary64 restatement of the depth-distortion ops (diff_gaussian_rasterization/distortion.py, csrc/gsr_distortion_math.h; DESIGN
section 29), in an independent form, and their error rule.

Values.  The distortion of one pixel is the explicit double sum over ordered pairs of its list of (w, m),
    D = 1/2 sum_i sum_j w_i w_j (m_i - m_j)^2                                                              (pair_sum)
and tests/test_distortion_ref.py holds A M2 - M1^2 to it on random lists.  For maps - whose inputs are the three sums, not the lists -
the reference evaluates A M2 - M1 M1 on the binary32 inputs in binary64 with two products and a difference (no fused operation), and
the gradients are binary64 autograd's.  The depth value is restated as m = far / (far - near) (1 - near / z), not the kernel's
quotient of two products, with z a plain dot product; its gradient is autograd's.  near and far enter as the binary32 numbers the
kernel is handed; far - near and far near are exact here and rounded once in the replay.

Error rule (tests/normals_ref.py's, whose Tracked is used here).  The kernels' binary32 operations are replayed on pairs (value, bound)
in the kernel's order: u = 2^-24 per add, subtract and multiply, 2 u per division, ONE rounding for an fma as written (the view
depth's three and D = fma(A, M2, -(M1 M1))); a product with a power of two, a negation and 0 - x add nothing.  The inputs are exact.

The loss.  k_distortion_fwd<true> gives every thread four consecutive pixels, and a pixel's term passes through
    3 adds in the thread ((D0 + D1) + D2) + D3, 6 levels of the wave's butterfly, 3 adds of the four waves' sums by thread 0
= LOSS_ADDS32 = 12 binary32 additions before it rests in partials[block].  Each level rounds every partial sum it forms once, and
the partial sums of one level are sums over disjoint sets of pixels, so to first order a level adds at most u sum|term|; 12 levels
add 12 u sum|term|.  k_distortion_sum then adds the partials in binary64: ceil(blocks / 256) - 1 adds in a thread, 6 butterfly levels,
3 adds of the waves' sums, the product with 1 / N (itself rounded), all at 2^-53, and ONE binary32 rounding for the final cast.
Nothing here comes from what the code under test gives.
"""
import numpy as np
import torch

from normals_ref import F64, U, Tracked, make_camera

U64 = 2.0 ** -53
BLOCK_PX = 1024           # csrc/gsr_distortion.hip kDstBlockPx: pixels of one block, one partial each
SUM_BLOCK = 256           # kDstSumBlock: partials per trip of the second stage
LOSS_ADDS32 = 3 + 6 + 3
NEAR, FAR = float(np.float32(0.2)), float(np.float32(100.0))


def loss_blocks(n):
    return -(-n // BLOCK_PX)


def loss_adds64(n):
    """Binary64 operations a partial passes through in k_distortion_sum, the product with the rounded 1 / N included."""
    return max(0, -(-loss_blocks(n) // SUM_BLOCK) - 1) + 6 + 3 + 2


def fma(a, b, c, fused=True):
    """a b + c on Tracked values: one rounding (fused) or the pair's two."""
    a, b, c = Tracked.of(a), Tracked.of(b), Tracked.of(c)
    if not fused:
        return a * b + c
    v = a.v * b.v + c.v
    return Tracked(v, a.v.abs() * b.e + b.v.abs() * a.e + c.e + U * v.abs())


# ---- the pair sum ----------------------------------------------------------------------------------------------------------------------

def pair_sum(w, m):
    """1/2 sum_i sum_j w_i w_j (m_i - m_j)^2 over ordered pairs of one pixel's list, binary64, two explicit loops."""
    w, m = np.asarray(w, np.float64), np.asarray(m, np.float64)
    total = 0.0
    for i in range(len(w)):
        for j in range(len(w)):
            total += w[i] * w[j] * (m[i] - m[j]) ** 2
    return 0.5 * total


def sums_of(w, m):
    w, m = np.asarray(w, np.float64), np.asarray(m, np.float64)
    return float(w.sum()), float((w * m).sum()), float((w * m * m).sum())


# ---- maps ------------------------------------------------------------------------------------------------------------------------------

def distortion_map_ref(moments, alpha):
    """moments [3,H,W], alpha [H,W]: binary64 tensors (leaves, for autograd) holding binary32 values -> D [H,W]."""
    return alpha * moments[1] - moments[0] * moments[0]


def distortion_loss_ref(moments, alpha):
    return distortion_map_ref(moments, alpha).mean()


def distortion_tracked(moments32, alpha32, grad_map=None, grad_loss=None, fused=True):
    """The replay of k_distortion_fwd / _bwd on binary32 arrays: {"D": Tracked [H,W]} and, with grad_map [H,W] (the map's backward) or
    grad_loss (the loss: also "loss"), {"dmoments": Tracked [3,H,W], "dalpha": Tracked [H,W]}.  fused=False counts the twin's
    operations instead: the product and the difference of A M2 - M1 M1 rounded separately, the mean's order free (see the test)."""
    M = torch.as_tensor(np.asarray(moments32), dtype=F64)
    A = Tracked(torch.as_tensor(np.asarray(alpha32), dtype=F64).reshape(M.shape[1:]))
    M1, M2 = Tracked(M[0]), Tracked(M[1])
    D = fma(A, M2, -(M1 * M1), fused)
    out = {"D": D}
    n = M[0].numel()
    if grad_loss is not None:
        loss = D.v.sum() / n
        absD = D.v.abs().sum()
        out["loss"] = Tracked(loss, (D.e.sum() + LOSS_ADDS32 * U * absD + loss_adds64(n) * U64 * absD) / n + U * loss.abs())
        g = Tracked(float(grad_loss)) * Tracked(1.0 / n, U / n)                     # grad_loss * (float)(1.0 / N)
        g = Tracked(g.v.expand(M[0].shape).clone(), g.e.expand(M[0].shape).clone())
    elif grad_map is not None:
        g = Tracked(torch.as_tensor(np.asarray(grad_map), dtype=F64).reshape(M[0].shape))
    else:
        return out
    dA, dM1, dM2 = g * M2, -((g * M1).pow2(2.0)), g * A
    zero = torch.zeros_like(M[0])
    out["dmoments"] = Tracked(torch.stack((dM1.v, dM2.v, zero)), torch.stack((dM1.e, dM2.e, zero)))
    out["dalpha"] = dA
    return out


# ---- Gaussians -------------------------------------------------------------------------------------------------------------------------

def depth_moments_ref(means, viewmatrix32, near=NEAR, far=FAR, mapping="ndc"):
    """means: a binary64 tensor [P,3] (a leaf, for autograd) holding binary32 values -> ([P,3] binary64, in_front [P] bool)."""
    V = torch.as_tensor(np.asarray(viewmatrix32).astype(np.float64))
    z = means @ V[:3, 2] + V[3, 2]
    front = z.detach() > (near if mapping == "ndc" else 0.0)
    zs = torch.where(front, z, torch.ones_like(z))
    m = far / (far - near) * (1.0 - near / zs) if mapping == "ndc" else zs
    m = torch.where(front, m, torch.zeros_like(m))
    return torch.stack((m, m * m, torch.zeros_like(m)), 1), front


def depth_moments_tracked(means32, viewmatrix32, near=NEAR, far=FAR, mapping="ndc", grad_out32=None, fused=True):
    """The replay of dst_moments_one / dst_moments_backward_one: {"out": Tracked [P,3], "fragile": bool [P]} and, with grad_out32,
    {"dmeans": Tracked [P,3]}.  fragile: z is within its own bound of the plane that culls it.  fused=False: the twin's view depth
    (three products and three sums, each rounded)."""
    P = means32.shape[0]
    V = np.asarray(viewmatrix32).astype(np.float64)
    p = [Tracked(torch.as_tensor(means32[:, i].astype(np.float64))) for i in range(3)]
    if fused:
        z = fma(p[0], float(V[0, 2]), fma(p[1], float(V[1, 2]), fma(p[2], float(V[2, 2]), float(V[3, 2]))))
    else:
        z = p[0] * float(V[0, 2]) + p[1] * float(V[1, 2]) + p[2] * float(V[2, 2]) + float(V[3, 2])
    plane = near if mapping == "ndc" else 0.0
    front = z.v > plane
    fragile = (z.v - plane).abs() <= z.e
    one = torch.ones(P, dtype=F64)
    zs = Tracked(torch.where(front, z.v, one), torch.where(front, z.e, 0 * one))
    if mapping == "ndc":
        den = (Tracked(far) - Tracked(near)) * zs
        m = (Tracked(far) * (zs - near)) / den
    else:
        m = zs
    m = m.where(front, 0.0)
    m2 = m * m
    zero = torch.zeros(P, dtype=F64)
    res = {"out": Tracked(torch.stack((m.v, m2.v, zero), 1), torch.stack((m.e, m2.e, zero), 1)), "fragile": fragile, "front": front}
    if grad_out32 is None:
        return res
    g = [Tracked(torch.as_tensor(grad_out32[:, j].astype(np.float64))) for j in range(2)]
    gz = g[0] + m.pow2(2.0) * g[1]
    if mapping == "ndc":
        gz = gz * ((Tracked(far) * Tracked(near)) / (den * zs))
    gz = gz.where(front, 0.0)
    d = [gz * float(V[k, 2]) for k in range(3)]
    res["dmeans"] = Tracked(torch.stack([c.v for c in d], 1), torch.stack([c.e for c in d], 1))
    return res


# ---- fixtures --------------------------------------------------------------------------------------------------------------------------

MAP_CASES = ((1, 1, "ndc"), (17, 33, "ndc"), (17, 33, "holes"), (17, 33, "linear"))          # H, W, form
GAUSSIAN_SIZES = (1, 257, 5000)


def make_lists(H, W, form, K=5, seed=0):
    """Per pixel a list of K splats: (w [H,W,K], m [H,W,K]) binary64, w_i = alpha_i T_i of random opacities; m in [0, 1) (ndc, holes) or
    a view depth in [0.5, 8) (linear).  holes: every fifth pixel, a 3 x 3 block and the last row are empty (all w = 0)."""
    rng = np.random.default_rng(31 * H + W + 1000 * seed + len(form))
    a = rng.uniform(0.02, 0.7, (H, W, K))
    T = np.cumprod(np.concatenate([np.ones((H, W, 1)), 1.0 - a[..., :-1]], -1), -1)
    w = a * T
    m = np.sort(rng.uniform(0.0, 1.0, (H, W, K)) if form != "linear" else rng.uniform(0.5, 8.0, (H, W, K)), -1)
    if form == "holes":
        hole = np.zeros((H, W), bool)
        hole.reshape(-1)[::5] = True
        hole[H // 2:H // 2 + 3, W // 2:W // 2 + 3] = True
        hole[-1, :] = True
        w[hole] = 0.0
    return w, m


def make_maps(H, W, form, seed=0):
    """(moments [3,H,W], alpha [H,W]) binary32, the sums of make_lists' lists rounded once; plane 2 holds a value that must not be read."""
    w, m = make_lists(H, W, form, seed=seed)
    A, M1, M2 = w.sum(-1), (w * m).sum(-1), (w * m * m).sum(-1)
    return np.stack((M1, M2, np.full_like(M1, 7.0))).astype(np.float32), A.astype(np.float32)


def make_upstream(H, W, seed=1):
    """grad_map [H,W] binary32, both signs."""
    return np.random.default_rng(91 * H + W + seed).standard_normal((H, W)).astype(np.float32)


def make_gaussians(P, seed=3):
    """(means [P,3], viewmatrix [4,4], grad_out [P,3]) binary32: a posed camera (normals_ref.make_camera) and means whose view depths lie
    on both sides of both cull planes: most between 0.5 and 9 in front, a sixth behind the camera, a sixth between it and `near`."""
    rng = np.random.default_rng(seed + 17 * P)
    V, _ = make_camera(seed)
    R, t = V[:3, :3].astype(np.float64), V[3, :3].astype(np.float64)
    view = np.stack((rng.uniform(-3, 3, P), rng.uniform(-3, 3, P), rng.uniform(0.5, 9.0, P)), 1)
    kind = np.arange(P) % 6
    view[kind == 4, 2] = rng.uniform(-5.0, -0.05, int((kind == 4).sum()))
    view[kind == 5, 2] = rng.uniform(0.02, 0.18, int((kind == 5).sum()))
    means = (view - t) @ R.T                                                         # p_view = p R + t
    return means.astype(np.float32), V, rng.standard_normal((P, 3)).astype(np.float32)
