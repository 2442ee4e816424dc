"""GPU tests of the kernels between the rasterizer's gradients and the next frame's parameters, element by element against the float64
restatements of tests/training_ref.py:

  csrc/gsr_optim.hip        k_adam_multi (gsr_adam_step_multi, and with one tensor gsr_adam_step and gsr_adam_step_split), k_densify_stats
  csrc/gsr_activations.hip  k_act_fwd, k_act_bwd
  csrc/gsr_knn.hip          the 3-NN chain, against the oracle's float64 brute force

Every float bound is |got - ref64| <= K u S per element (u = 2^-24, S the scale training_ref derives for that element), Adam's parameter
u |p'| + K u U.  Adam is compared over ONE step from a seeded mid-training state: multi-step float32 trajectories with eps = 1e-15 and
v ~ 0 diverge for reasons that are no defect.  K = ceil(2 x measured worst ratio), never above the ceiling counted from the kernel's
expression (training_ref.CEIL); each test prints the ratios it measures.

Worst ratios measured on an MI355X (gfx950; gsr_optim.o built with -ffp-contract=fast, gsr_activations.o with the default contraction),
in units of u S:

  quantity            kernel, case                                      measured   2 x, rounded up   ceiling   asserted K
  m'                  67 M floats (grid wrap)                              1.795          4              3          3
                      4 195 331 floats / 155 401 rows of 27 (one tensor)   1.784 / 1.771
                      item edges / split rows / eight tensors              1.742 / 1.712 / 1.765
  v'                  67 M floats                                          1.983          4              4          4
                      4 195 331 floats / 155 401 rows of 27                1.976 / 1.968
                      item edges / split rows / eight tensors              1.907 / 1.924 / 1.819
  p' beyond u |p'|    4 195 331 floats                                     3.626          8             12          8
                      67 M floats / 155 401 rows of 27                     3.574 / 2.469
                      item edges / split rows / eight tensors              2.754 / 2.539 / 2.294
  activations forward k_act_fwd, P = 2 098 179 (1000: 2.142)               3.113          7              8          7
  d_scaling           k_act_bwd, P = 2 098 179 (1000: 0.982)               0.999          2              1          1
  d_opacity           k_act_bwd, P = 2 098 179 (1000: 2.361)               2.819          6              3          3
  d_rotation          k_act_bwd, P = 2 098 179 (1000: 4.262)               8.960         18             16         16
  xyz_gradient_accum  k_densify_stats, P = 1000 (255 .. 257: 1.5)          1.814          4              3          3

No measured ratio is above its ceiling.  The three Adam entry points run one kernel, whose rule (csrc/gsr_math.h adam_update) spells every
multiply-add as an fmaf: the one-tensor calls measure what gsr_adam_step_multi measures on the same case, and tests/test_training_ref.py gets
the same ratios from the rule compiled for the host.  v' = fma((1 - b2) g, g, v b2) has three roundings of the four counted.
"""
import numpy as np
import pytest
import torch

import oracle
import training_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B1, B2 = R.ADAM_BETAS
EPS = R.ADAM_EPS
GUARD = 64                             # floats of sentinel on either side of every small Adam tensor
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def N():
    from diff_gaussian_rasterization import _native
    return _native


def _guarded(t):
    """t on the device inside a buffer whose margins must keep their sentinel (a kernel that writes past a tail shows here)."""
    buf = torch.full((t.numel() + 2 * GUARD,), SENTINEL, device=DEV)
    view = buf[GUARD:GUARD + t.numel()]
    view.copy_(t.reshape(-1))
    return view, buf


def _guards_intact(buf):
    return bool((buf[:GUARD] == SENTINEL).all()) and bool((buf[-GUARD:] == SENTINEL).all())


def _launch(N, entry, items):
    """items: [(p, g, m, v, lr, lr_tail, step, row_len, split)], flat device tensors."""
    if entry == "multi":
        N.adam_step_multi(items, B1, B2, EPS)
        return
    for p, g, m, v, lr, lr_tail, step, row_len, split in items:
        if entry == "single":
            assert row_len == 0
            N.adam_step(p, g, m, v, lr, B1, B2, EPS, step)
        else:
            N.adam_step_split(p.view(-1, row_len), g, m, v, split, lr, lr_tail, B1, B2, EPS, step)


def _adam_check(N, entry, cases, top):
    """Run every case of `cases` (one launch for "multi") and hold each to its float64 step; the worst ratios go to `top`."""
    host, dev = [], []
    for n, row_len, split, step, lr, lr_tail, seed in cases:
        host.append(R.adam_state(n, seed))
        dev.append([_guarded(t) for t in host[-1]])
    items = [tuple(view for view, _ in d) + (lr, lr_tail, step, row_len, split) for d, (n, row_len, split, step, lr, lr_tail, seed) in zip(dev, cases)]
    _launch(N, entry, items)
    torch.cuda.synchronize()
    for (n, row_len, split, step, lr, lr_tail, seed), (p, g, m, v), d in zip(cases, host, dev):
        what = (entry, n, row_len, split, step)
        assert all(_guards_intact(buf) for _, buf in d), what
        assert R.bits_equal(d[1][0].cpu(), g), what                                     # the gradient is only read
        if n == 0:
            continue
        ref, scl = R.adam_step64(p, g, m, v, lr, lr_tail, step, row_len, split, B1, B2, EPS)
        got = [d[i][0].cpu() for i in (0, 2, 3)]
        assert all(bool(torch.isfinite(t).all()) for t in got), what
        for key, r in (("adam_m", R.worst(got[1], ref[1], scl[0])), ("adam_v", R.worst(got[2], ref[2], scl[1])),
                       ("adam_p", R.worst_p(got[0], ref[0], scl[2]))):
            top[key] = max(top.get(key, 0.0), r)
            assert r <= R.K[key], (what, key, r)
        for i in R.adam_planted(n):                                                     # g = m = v = 0: p keeps its bits
            assert R.bits_equal(got[0][i:i + 1], p[i:i + 1]), (what, i)
        if lr == 0.0 and lr_tail == 0.0:
            assert R.bits_equal(got[0], p), what
            assert not torch.equal(got[1], m) and not torch.equal(got[2], v), what


def _report(name, top):
    print(f"\nMEASURED {name}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(top.items())))


PLAIN = [c for c in R.adam_cases() if c[1] == 0]
SPLIT = [c for c in R.adam_cases() if c[1] != 0]


@pytest.mark.parametrize("entry", ("multi", "single"))
def test_adam_one_learning_rate_at_every_item_edge(N, entry):
    """n around the 4-float vector and the 4096-float work item (a tail-only item at 4097 and 4098), steps 1, 2, 7 and 10^6."""
    top = {}
    for case in PLAIN:
        _adam_check(N, entry, [case], top)
    _report(f"adam plain {entry}", top)


@pytest.mark.parametrize("entry", ("multi", "split"))
def test_adam_split_rows_across_an_item_end(N, entry):
    """[rows, row_len] with the head / tail boundary at 0, 1, 3, row_len - 1 and row_len; rows of 5 and 27 floats put a float4 across a
    row's end."""
    top = {}
    for case in SPLIT:
        _adam_check(N, entry, [case], top)
    _report(f"adam split {entry}", top)


def test_adam_multi_eight_tensors_in_one_launch(N):
    """Eight tensors, one of them empty, each with its own step count and learning rates; tail-only items in the middle of the item list."""
    top = {}
    _adam_check(N, "multi", R.ADAM_EIGHT, top)
    _report("adam multi eight tensors", top)


@pytest.mark.parametrize("entry", ("multi", "single", "split"))
def test_adam_zero_learning_rate_moves_only_the_moments(N, entry):
    case = (153 * 27, 27, 3, 7, 0.0, 0.0, 9) if entry != "single" else (4098, 0, 0, 7, 0.0, 0.0, 9)
    _adam_check(N, entry, [case], {})


@pytest.mark.parametrize("entry", ("single", "split"))
def test_adam_one_tensor_kernels_wrap_their_grid(N, entry):
    """gsr_adam_step at 4 195 331 floats and gsr_adam_step_split at 155 401 rows of 27 (just past 4096 x 256 float4): k_adam_multi with one
    tensor of 1025 work items, the last one with 256 and 380 float4 and the three trailing floats."""
    rows, row_len = R.ADAM_WRAP_SPLIT
    case = (R.ADAM_WRAP_PLAIN, 0, 0, 7, 0.01, 0.01, 41) if entry == "single" else (rows * row_len, row_len, 3, 2, 0.0025, 0.000125, 42)
    assert case[0] // 4 > 4096 * 256 and case[0] % 4 == 3
    top = {}
    _adam_check(N, entry, [case], top)
    _report(f"adam wrap {entry}", top)


def _compare_on_device(top, got, before, g, args, lo, hi, what):
    """[lo, hi) of one tensor of the big state against its float64 step, computed on the device in chunks of 8 M elements."""
    lr, lr_tail, step, row_len, split = args
    for c in range(lo, hi, 8 << 20):
        e = min(hi, c + (8 << 20))
        ref, scl = R.adam_step64(before[0][c:e], g[c:e], before[1][c:e], before[2][c:e], lr, lr_tail, step, row_len, split, B1, B2, EPS, index0=c - lo)
        for key, r in (("adam_m", R.worst(got[1][c:e], ref[1], scl[0])), ("adam_v", R.worst(got[2][c:e], ref[2], scl[1])),
                       ("adam_p", R.worst_p(got[0][c:e], ref[0], scl[2]))):
            top[key] = max(top.get(key, 0.0), r)
            assert r <= R.K[key], (what, c, key, r)


def test_adam_multi_wraps_its_grid(N):
    """16 385 x 4096 + 3 floats are 16 386 work items for 16 384 blocks: blocks 0 and 1 take a second trip, block 1's being the tail-only item.
    A second launch steps the same memory as two tensors (rows of 27 with a split, then a short one) whose boundary lies beyond item 16 384,
    so the search for an item's tensor is taken on a second trip too.  The floats between the two tensors keep their bits."""
    n = 16385 * R.ADAM_ITEM + 3
    gen = torch.Generator(device=DEV).manual_seed(77)
    p, g = torch.randn(n, device=DEV, generator=gen), torch.randn(n, device=DEV, generator=gen)
    m, v = 0.1 * torch.randn(n, device=DEV, generator=gen), (0.03 * torch.randn(n, device=DEV, generator=gen)) ** 2
    for base in (0, 16384 * R.ADAM_ITEM, n - 3):                    # the planted triple at the start, in the second-trip item and in the tail
        g[base] = m[base] = v[base] = 0.0
        g[base + 1] = v[base + 1] = 0.0
        g[base + 2] = 1e3
    g0 = g.clone()
    top = {}
    before = [t.clone() for t in (p, m, v)]
    N.adam_step_multi([(p, g, m, v, 0.01, 0.01, 7, 0, 0)], B1, B2, EPS)
    _compare_on_device(top, (p, m, v), before, g, (0.01, 0.01, 7, 0, 0), 0, n, "one tensor")
    for base in (0, 16384 * R.ADAM_ITEM, n - 3):
        assert R.bits_equal(p[base:base + 1], before[0][base:base + 1])
    n_a = 27 * 2_485_514                                             # 16 384 x 4096 + 14 floats: 16 385 items, the last one with the 2-float tail
    off_b = (n_a + 3) // 4 * 4
    assert n_a > 16384 * R.ADAM_ITEM and n_a % 4 == 2 and n - off_b > 4 and (n - off_b) % 4 == 3
    for dst, src in zip(before, (p, m, v)):
        dst.copy_(src)
    args_a, args_b = (0.0025, 0.000125, 2, 27, 3), (0.05, 0.05, 1000, 0, 0)
    N.adam_step_multi([(p[:n_a], g[:n_a], m[:n_a], v[:n_a]) + args_a, (p[off_b:], g[off_b:], m[off_b:], v[off_b:]) + args_b], B1, B2, EPS)
    _compare_on_device(top, (p, m, v), before, g, args_a, 0, n_a, "rows of 27")
    _compare_on_device(top, [t[off_b:] for t in (p, m, v)], [t[off_b:] for t in before], g[off_b:], args_b, 0, n - off_b, "short tensor")
    for now, was in zip((p, m, v), before):
        assert R.bits_equal(now[n_a:off_b], was[n_a:off_b])
    assert R.bits_equal(g, g0) and bool(torch.isfinite(p).all())
    _report("adam multi wrap", top)


# ---- activations -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.ACT_SIZES)
def test_activations_against_float64(N, P):
    """Forward and backward per element.  2 098 179 Gaussians is the smallest size class at which the scale, opacity and quaternion block
    ranges all take a second trip, with a 3-float opacity tail and a 1-float scale tail."""
    (sc, ro, op), grads = R.activation_inputs(P, P)
    dev = [t.to(DEV) for t in (sc, ro, op)]
    got = N.activations_forward(*dev)
    vals, scl = R.activations64(sc, ro, op)
    top = {}
    for name, a, b, s in zip(("scales", "rotations", "opacities"), got, vals, scl):
        assert a.shape == b.shape
        r = R.worst(a.cpu(), b, s)
        top["act_fwd"] = max(top.get("act_fwd", 0.0), r)
        assert r <= R.K["act_fwd"], (name, r)
    dgrads = [t.to(DEV) for t in grads]
    d = N.activations_backward(got[0], dev[1], got[2], *dgrads)
    want, dscl = R.activations_backward64(got[0].cpu(), ro, got[2].cpu(), *grads)            # on the forward values the kernel reads
    for name, mine, b, s in zip(("d_scaling", "d_rotation", "d_opacity"), d, want, dscl):
        assert mine.shape == b.shape and bool(torch.isfinite(mine).all()), name
        r = R.worst(mine.cpu(), b, s)
        top[name] = r
        assert r <= R.K[name], (name, r)
    # a None gradient skips that tensor
    d2 = N.activations_backward(got[0], dev[1], got[2], dgrads[0], None, dgrads[2])
    assert d2[1] is None and torch.equal(d2[0], d[0]) and torch.equal(d2[2], d[2])
    for a, b in zip(dev, (sc, ro, op)):
        assert R.bits_equal(a.cpu(), b)                                                       # inputs are only read
    _report(f"activations P={P}", top)


# ---- densification statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", R.DENSIFY_SIZES)
def test_densify_stats_against_float64(N, P):
    """Negative, zero and positive radii and 2^24 + 1 (which float32 rounds to 2^24); NaN in every hidden row's gradient and in column 2
    of every row; non-trivial prior contents, which a hidden row keeps bit for bit."""
    radii, grad, mr, acc, den = R.densify_inputs(P, P)
    (mr1, acc1, den1), s = R.densify_stats64(radii, grad, mr, acc, den)
    d_mr, d_acc, d_den = mr.to(DEV), acc.to(DEV), den.to(DEV)
    N.densify_stats(radii.to(DEV), grad.to(DEV), d_mr, d_acc, d_den)
    torch.cuda.synchronize()
    hidden = radii <= 0
    for now, was in ((d_mr.cpu(), mr), (d_acc.cpu(), acc), (d_den.cpu(), den)):
        assert R.bits_equal(now[hidden], was[hidden])
    assert torch.equal(d_mr.cpu().double(), mr1) and torch.equal(d_den.cpu().double().reshape(-1), den1)
    assert float(d_mr[P - 1]) == 2.0 ** 24
    r = R.worst(d_acc.cpu(), acc1, s)
    assert r <= R.K["densify_accum"], r
    _report(f"densify P={P}", {"densify_accum": r})


# ---- 3-NN --------------------------------------------------------------------------------------------------------------------------
def _clouds():
    g = torch.Generator().manual_seed(2024)
    rn = lambda *s: torch.randn(*s, generator=g)
    c = {f"random {P}": rn(P, 3) * torch.tensor([1.0, 0.3, 2.0]) for P in (4, 7, 8, 511, 512, 513, 1025)}
    c["identical 4099"] = torch.tensor([0.3, -1.7, 2.9]).repeat(4099, 1)
    c["planar"] = torch.cat([rn(2000, 2), torch.full((2000, 1), 0.7)], 1)
    c["collinear"] = rn(2000, 1) * torch.tensor([[1.0, 2.0, -1.0]]) + torch.tensor([0.5, 0.0, -3.0])
    # each cluster collapses to a Morton cell (1 / 1023 of the extent is a thousand cluster widths), so its points keep their input order:
    # the +-3 seeds are arbitrary points of the cluster, and the box of points 512..1023 spans both clusters
    c["two clusters"] = torch.cat([rn(1000, 3) * 1e-3, rn(1000, 3) * 1e-3 + torch.tensor([1e3, 1e3, 1e3])])
    c["offset"] = rn(3000, 3) * 1e-2 + torch.tensor([1000.0, -1000.0, 1000.0])
    c["negative octant"] = -rn(1500, 3).abs() - 1.0
    t = torch.arange(16, dtype=torch.float32) * 0.1
    c["grid 16^3"] = torch.stack(torch.meshgrid(t, t, t, indexing="ij"), -1).reshape(-1, 3)
    # two slabs 2e-3 apart in x, the most significant Morton axis: every point's nearest neighbours lie in the other slab too, 300 places
    # away in Morton order, and the second slab straddles the boundary between the boxes of points 0..511 and 512..599
    yz = torch.rand(600, 2, generator=g)
    c["two slabs"] = torch.cat([torch.where(torch.arange(600) % 2 == 0, -1e-3, 1e-3)[:, None], yz], 1)
    return c


CLOUDS = _clouds()


@pytest.mark.parametrize("name", list(CLOUDS))
def test_dist2_knn3_on_clouds_that_stress_the_morton_boxes(N, name):
    pts = CLOUDS[name]
    want = oracle.dist2_knn3(pts.numpy())
    got = N.dist2_knn3(pts.to(DEV)).cpu().numpy()
    if name.startswith("identical"):
        assert not got.any() and not want.any()
    if name == "two slabs":                                       # the cloud is what it claims: most points have one of their 3 in the other slab
        d = torch.cdist(pts.double(), pts.double()).fill_diagonal_(float("inf"))
        lo = pts[:, 0] < 0
        assert float((lo[d.topk(3, largest=False).indices] != lo[:, None]).any(1).float().mean()) > 0.8
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=2e-5, atol=1e-9)
