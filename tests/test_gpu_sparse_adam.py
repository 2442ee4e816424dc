"""k_adam_sparse_multi on the GPU, held BITWISE to the dense kernel (k_adam_multi; both in csrc/gsr_optim.hip): a visible row of a
sparse step is the dense step's row, a hidden row is what it was.  Shapes: the model's five tensors [P,3] [P,M,3] [P,1] [P,3]
[P,4] in one launch, the SH table with its two learning rates (head_cols = 1, tail) for M in {1, 4, 9, 16}, i.e. every width the
kernel specialises (1, 3, 4, 12, 27, 48); P in {1, 3, 257, 1366, 4099}: P = 1366 makes a width-3 tensor of 4098 floats = one full
work item of 1024 float4 (the sparse kernel's item is the dense one's), a row across its end and a 2-float tail."""
from dataclasses import replace

import pytest
import torch

import scene_synth as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = (1, 3, 257, 1366, 4099)
MASKS = ("none", "all", "first", "last", "alternating", "random10", "random50", "second_half", "first_half", "run")


def _mask(kind, P, gen):
    m = torch.zeros(P, dtype=torch.bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[P - 1] = True
    elif kind == "alternating":
        m[::2] = True
    elif kind == "random10":
        m = torch.rand(P, generator=gen) < 0.1
    elif kind == "random50":
        m = torch.rand(P, generator=gen) < 0.5
    elif kind == "second_half":                                  # a skipped work item beside a worked one
        m[P // 2:] = True
    elif kind == "first_half":
        m[:P // 2] = True
    elif kind == "run":                                          # both ends odd: inside a float4 of a width-1 and of a width-3 tensor
        a = min(P - 1, (P // 3) | 1)
        m[a:max(a + 1, min(P, (2 * P // 3) | 1))] = True
    return m


def _as_radii(mask):
    """int32 radii: positive where visible, zero and negative entries (both hidden) elsewhere."""
    i = torch.arange(mask.shape[0])
    return torch.where(mask, 1 + i % 9, -(i % 2) * 7).to(torch.int32)


def _groups(ps):
    return [{"params": [ps[0]], "lr": 0.00016, "name": "xyz"},
            {"params": [ps[1]], "lr": 0.0025, "name": "f_dc", "head_cols": 1, "tail": "f_rest"},
            {"params": [], "lr": 0.000125, "name": "f_rest"},
            {"params": [ps[2]], "lr": 0.05, "name": "opacity"}, {"params": [ps[3]], "lr": 0.005, "name": "scaling"},
            {"params": [ps[4]], "lr": 0.001, "name": "rotation"}]


def _seeded(P, M, gen, steps=(3, 1, 7, 2, 5)):
    """A state in mid-training: parameters, both moments (second one >= 0) and a step count of its own per tensor."""
    out = []
    for shape, k in zip(((P, 3), (P, M, 3), (P, 1), (P, 3), (P, 4)), steps):
        r = lambda s=1.0: (torch.randn(shape, generator=gen) * s).to(DEV)
        out.append((r(), r(0.1), r(0.03) ** 2, k))
    return out


def _optimizer(cls, state, views=None, **kw):
    """cls over clones of `state` (or over `views`: [(p, m, v)] tensors to step in place), moments and step counts installed."""
    ps = [(p.clone() if views is None else views[i][0]).requires_grad_(True) for i, (p, _, _, _) in enumerate(state)]
    opt = cls(_groups(ps), lr=0.0, eps=1e-15, **kw)
    for i, (p, (_, m, v, k)) in enumerate(zip(ps, state)):
        opt.state[p] = {"step": torch.tensor(float(k)), "exp_avg": m.clone() if views is None else views[i][1],
                        "exp_avg_sq": v.clone() if views is None else views[i][2]}
    return ps, opt


def _current(ps, opt):
    return [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone(), int(opt.state[p]["step"])) for p in ps]


def _sparse_vs_dense(ps, sparse, mask, as_radii, gen, poison=False, **kw):
    """One step of `sparse` under `mask` against FusedAdam.step() on clones of its state: torch.where(visible rows, dense, before)."""
    from fused_adam import FusedAdam
    before = _current(ps, sparse)
    qs, dense = _optimizer(FusedAdam, before)
    vis = mask.to(DEV)
    for p, q in zip(ps, qs):
        q.grad = torch.randn(p.shape, generator=gen).to(DEV)
        p.grad = q.grad.clone()
        if poison:                                               # a hidden row's gradient is not used, whatever it holds
            bad = torch.tensor([float("nan"), float("inf"), float("-inf")], device=DEV)[torch.arange(p.numel(), device=DEV) % 3].view(p.shape)
            p.grad = torch.where(vis.view(-1, *([1] * (p.dim() - 1))), p.grad, bad)
    grads = [p.grad.clone() for p in ps]
    versions = [p._version for p in ps]
    dense.step()
    sparse.step(visibility=_as_radii(mask).to(DEV) if as_radii else vis)
    for i, (p, q, (p0, m0, v0, k0)) in enumerate(zip(ps, qs, before)):
        rows = vis.view(-1, *([1] * (p.dim() - 1)))
        st, sq = sparse.state[p], dense.state[q]
        for name, got, want_seen, was in (("param", p.detach(), q.detach(), p0), ("exp_avg", st["exp_avg"], sq["exp_avg"], m0),
                                          ("exp_avg_sq", st["exp_avg_sq"], sq["exp_avg_sq"], v0)):
            want = torch.where(rows, want_seen, was)
            assert torch.equal(got, want), (i, name, kw, int((got != want).sum()))
        assert int(st["step"]) == k0 + 1 == int(sq["step"])              # seen or not, the call counts
        assert torch.isfinite(p.detach()).all() and torch.isfinite(st["exp_avg"]).all() and torch.isfinite(st["exp_avg_sq"]).all()
        assert torch.equal(p.grad.view(torch.int32), grads[i].view(torch.int32))         # the gradient is only read (bits: it may hold NaN)
        assert p._version > versions[i] or not mask.any()                # autograd is told about the raw-pointer write


@pytest.mark.parametrize("M", (1, 4, 9, 16))
@pytest.mark.parametrize("P", SIZES)
def test_stepwise_bitwise_against_the_dense_kernel(P, M):
    """Consecutive steps of one SparseFusedAdam with a changing mask, every mask once as bool and once as int32 radii; each step is
    compared with the dense kernel's step from the same state."""
    from fused_adam import SparseFusedAdam
    gen = torch.Generator().manual_seed(100 * P + M)
    ps, sparse = _optimizer(SparseFusedAdam, _seeded(P, M, gen))
    for n, kind in enumerate(MASKS + MASKS):
        _sparse_vs_dense(ps, sparse, _mask(kind, P, gen), as_radii=(n >= len(MASKS)) != (n % 2 == 1), gen=gen, P=P, M=M, kind=kind, n=n)


@pytest.mark.parametrize("P", SIZES)
def test_hidden_gradients_are_not_used(P):
    from fused_adam import SparseFusedAdam
    gen = torch.Generator().manual_seed(7 * P)
    ps, sparse = _optimizer(SparseFusedAdam, _seeded(P, 16, gen))
    for n, kind in enumerate(("random50", "alternating", "run", "first", "none", "random10")):
        _sparse_vs_dense(ps, sparse, _mask(kind, P, gen), as_radii=n % 2 == 1, gen=gen, poison=True, P=P, kind=kind)


@pytest.mark.parametrize("P", SIZES)
def test_no_write_outside_the_tensors(P):
    """param, exp_avg and exp_avg_sq are views into the middle of larger buffers of a sentinel: 64 floats on each side are intact
    after the steps (a width-3 tensor of 4098 floats ends 2 floats into a float4), and the gradient buffers are as they were."""
    from fused_adam import SparseFusedAdam
    gen = torch.Generator().manual_seed(13 * P)
    state = _seeded(P, 16, gen)
    SENT, PAD = 12345.0, 64
    bufs, views = [], []
    for p, m, v, _ in state:
        three = []
        for t in (p, m, v):
            buf = torch.full((PAD + t.numel() + PAD,), SENT, device=DEV)
            buf[PAD:PAD + t.numel()] = t.reshape(-1)
            bufs.append(buf)
            three.append(buf[PAD:PAD + t.numel()].view(t.shape))
        views.append(tuple(three))
    ps, sparse = _optimizer(SparseFusedAdam, state, views=views)
    gbufs = []
    for p in ps:
        gb = torch.full((PAD + p.numel() + PAD,), SENT, device=DEV)
        gb[PAD:PAD + p.numel()] = torch.randn(p.numel(), generator=gen).to(DEV)
        gbufs.append(gb)
        p.grad = gb[PAD:PAD + p.numel()].view(p.shape)
    gclones = [g.clone() for g in gbufs]
    for n, kind in enumerate(("all", "last", "random50", "run", "second_half")):
        mask = _mask(kind, P, gen)
        sparse.step(visibility=_as_radii(mask).to(DEV) if n % 2 else mask.to(DEV))
    torch.cuda.synchronize()
    for buf, (p, m, v, _) in zip(bufs[0::3], state):
        assert not torch.equal(buf[PAD:-PAD].view(p.shape), p)                     # it did step
    for buf in bufs:
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())
    for g, c in zip(gbufs, gclones):
        assert torch.equal(g, c)


def test_same_inputs_twice_give_the_same_bits_and_no_mask_is_the_dense_step():
    from fused_adam import FusedAdam, SparseFusedAdam
    P = 4099
    gen = torch.Generator().manual_seed(21)
    state = _seeded(P, 16, gen)
    grads = [torch.randn(p.shape, generator=gen).to(DEV) for p, _, _, _ in state]
    mask = _mask("random50", P, gen).to(DEV)
    results = []
    for cls, vis in ((SparseFusedAdam, mask), (SparseFusedAdam, mask), (SparseFusedAdam, None), (FusedAdam, None)):
        ps, opt = _optimizer(cls, state)
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        opt.step(vis) if cls is SparseFusedAdam else opt.step()
        results.append(_current(ps, opt))
    for a, b in ((results[0], results[1]), (results[2], results[3])):
        for x, y in zip(a, b):
            assert all(torch.equal(s, t) for s, t in zip(x[:3], y[:3])) and x[3] == y[3]


def test_one_launch_of_its_own_name_per_step():
    from diff_gaussian_rasterization import _native as N
    from fused_adam import SparseFusedAdam
    gen = torch.Generator().manual_seed(5)
    ps, sparse = _optimizer(SparseFusedAdam, _seeded(257, 16, gen))
    N.profile_enable(True)
    try:
        for n in range(3):
            for p in ps:
                p.grad = torch.randn(p.shape, generator=gen).to(DEV)
            sparse.step(visibility=_mask(("random50", "none", "all")[n], 257, gen).to(DEV))
        torch.cuda.synchronize()
        prof = N.profile_read()
    finally:
        N.profile_enable(False)
    assert prof["adam_sparse"][1] == 3 and "adam" not in prof, prof


def test_uncorrected_step_is_the_rule_without_bias_corrections():
    """bias_correction=False (upstream's arithmetic: step size lr, second moment as it is) against float64 over three steps with
    changing masks, under the conditions and the bounds the project holds FusedAdam to (test_fused_adam_matches_torch_adam: fresh
    moments, N(0,1) gradients, |p - p64| <= 2e-6 max(1, max |p|), |v - v64| <= 1e-6)."""
    from fused_adam import SparseFusedAdam
    P = 1366
    gen = torch.Generator().manual_seed(8)
    state = [(p, torch.zeros_like(m), torch.zeros_like(v), 0) for p, m, v, _ in _seeded(P, 16, gen)]
    ps, sparse = _optimizer(SparseFusedAdam, state, bias_correction=False)
    lrs = ((0.00016, 0.00016), (0.0025, 0.000125), (0.05, 0.05), (0.005, 0.005), (0.001, 0.001))
    ref = [[t.double().cpu() for t in (p0, m0, v0)] for p0, m0, v0, _ in state]
    # the rule's coefficients as the C ABI receives them: beta1, beta2 are floats, and 1 - beta is formed in float (the uncorrected step
    # has no 1 / (1 - beta2^t) in front of v that would divide the rounding of 1 - beta2 out again)
    f32 = lambda x: torch.tensor(x, dtype=torch.float32)
    b2, one_minus_b1, one_minus_b2 = float(f32(0.999)), float(1 - f32(0.9)), float(1 - f32(0.999))
    for kind in ("random50", "alternating", "random10"):
        mask = _mask(kind, P, gen)
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(DEV)
        sparse.step(visibility=mask.to(DEV))
        for p, (p64, m64, v64), (lr_head, lr_tail) in zip(ps, ref, lrs):
            g = p.grad.double().cpu()
            lr = torch.full(p64.shape, lr_head, dtype=torch.float64)
            if p64.dim() == 3:
                lr[:, 1:] = lr_tail
            m64[mask] = m64[mask] + (g[mask] - m64[mask]) * one_minus_b1
            v64[mask] = v64[mask] * b2 + one_minus_b2 * g[mask] * g[mask]
            p64[mask] = p64[mask] - lr[mask] * (m64[mask] / (v64[mask].sqrt() + 1e-15))
    for p, (p64, m64, v64) in zip(ps, ref):
        ep = float((p.detach().double().cpu() - p64).abs().max())
        ev = float((sparse.state[p]["exp_avg_sq"].double().cpu() - v64).abs().max())
        print(f"uncorrected, shape {tuple(p.shape)}: |p - p64| = {ep:.3e}, |v - v64| = {ev:.3e}")
        assert ep <= 2e-6 * max(1.0, float(p64.abs().max())) and ev <= 1e-6
        assert int(sparse.state[p]["step"]) == 3


def test_through_the_training_loop():
    """Two GaussianModels from one seeded scene of 4 000 Gaussians at 160 x 112, one with the default optimizer and one with
    optimizer_type = "sparse_adam", under a camera with half the field of view the scene was laid out for (tan(fovy / 2) = 0.3 against
    1.1 x 0.5: the CPU oracle gives radii > 0 for 1 715 of the 4 000, 42.9 %).  After one iteration of train(): a row the frame saw
    is bitwise the same in both models, on every leaf and both moments; a row it did not see is, in the sparse model, what it was.
    Then 30 iterations of the sparse model lower the loss."""
    from fused_adam import FusedAdam, SparseFusedAdam
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    W, H, P = 160, 112, 4000
    scene = S.make_scene(P, W, H, 2, 30, scale_lo=0.01, scale_hi=0.08)
    cam, bg = S.make_camera(W, H, tanfovy=0.3).to(DEV), torch.zeros(3, device=DEV)
    truth = GaussianModel(2); truth.adopt_scene(scene, device=DEV)
    # the models start off the truth: dimmer colours, lower opacities (the same places and shapes: the same visible set)
    start = replace(scene, shs=scene.shs * 0.5, opacity_logits=scene.opacity_logits - 1.0)
    probe = GaussianModel(2); probe.adopt_scene(start, device=DEV)
    with torch.no_grad():
        target = render(cam, truth, Pipe(), bg)["render"].clone()
        seen = render(cam, probe, Pipe(), bg)["radii"] > 0
    assert 0 < int(seen.sum()) < P
    opt = replace(OptimizationDefaults(), densify_from_iter=10 ** 9, densify_until_iter=0)       # densification off
    models = []
    for kind, cls in (("default", FusedAdam), ("sparse_adam", SparseFusedAdam)):
        gm = GaussianModel(2); gm.adopt_scene(start, device=DEV)
        gm.training_setup(replace(opt, optimizer_type=kind))
        assert type(gm.optimizer) is cls
        before = {k: t.detach().clone() for k, t in gm._t.items()}
        train(gm, [cam], [target], replace(opt, optimizer_type=kind), Pipe(), bg, iterations=2)      # the step of iteration 1; the last one has none
        models.append((gm, before))
    (dense, _), (sparse, before) = models
    for k in dense._t:
        rows = seen.view(-1, *([1] * (dense._t[k].dim() - 1)))
        sd, ss = dense.optimizer.state[dense._t[k]], sparse.optimizer.state[sparse._t[k]]
        assert int(sd["step"]) == int(ss["step"]) == 1
        for name, a, b, was in ((k, dense._t[k].detach(), sparse._t[k].detach(), before[k]),
                                (k + ".exp_avg", sd["exp_avg"], ss["exp_avg"], torch.zeros_like(before[k])),
                                (k + ".exp_avg_sq", sd["exp_avg_sq"], ss["exp_avg_sq"], torch.zeros_like(before[k]))):
            assert torch.equal(torch.where(rows, a, was), b), name
        assert not torch.equal(sparse._t[k].detach(), before[k]), k
    losses = []
    sparse.optimizer.zero_grad(set_to_none=True)                 # (the last iteration of a train() call neither steps nor clears)
    train(sparse, [cam], [target], replace(opt, optimizer_type="sparse_adam"), Pipe(), bg, iterations=31,
          on_iteration=lambda it, loss, g: losses.append(float(loss.detach())))
    assert len(losses) == 31 and all(l == l for l in losses)
    assert losses[-1] < losses[0] and sum(losses[-5:]) < sum(losses[:5]), (losses[:3], losses[-3:])
