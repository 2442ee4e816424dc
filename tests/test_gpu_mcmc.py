"""csrc/gsr_mcmc.hip on the GPU: the relocation rule, the row edit, the position noise and the regulariser gradient, every element
against the binary64 restatement (tests/mcmc_ref.py) under its error rules; what is a copy or must stay is compared bit for bit.
Then GaussianModel.mcmc_* on the device with the native path (the checks of tests/mcmc_checks.py, and the host path as a second
reference), and train() under densify_strategy = "mcmc" with both optimizers."""
import ctypes as C
from dataclasses import replace

import numpy as np
import pytest
import torch

import mcmc_checks as MC
import mcmc_ref as MR
import scene_synth as S
from diff_gaussian_rasterization import mcmc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a), dtype=dtype).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


# ---- the relocation rule ------------------------------------------------------------------------------------------------------------
def _sources(P, n, rng):
    """n draws from [0, P): row 5 sixty times (> 51), row 7 fifty-one times, row 8 fifty times (N = 51 exactly), row 9 twice, then
    distinct rows (taken once) and random ones (a few taken twice or three times), shuffled."""
    fixed = np.concatenate((np.full(60, 5), np.full(51, 7), np.full(50, 8), np.full(2, 9)))
    if n < fixed.size + 10:
        return fixed[:n].copy()
    rest = n - fixed.size
    once = rng.permutation(np.arange(10, P // 2))[:rest // 2]
    some = rng.integers(P // 2, P, rest - once.size)
    s = np.concatenate((fixed, once, some))
    rng.shuffle(s)
    return s


@pytest.mark.parametrize("n", (3000, 1, 0))
def test_relocation_rule_against_the_restatement(n):
    P = 4099
    x, ls = MR.relocation_inputs(P, 21)
    sampled = _sources(P, n, np.random.default_rng(n))
    out_o, out_s = mcmc.compute_relocation(dev(x), dev(ls), dev(sampled, torch.int64), 0.005)
    assert out_o.shape == (n,) and out_s.shape == (n, 3) and out_o.dtype == out_s.dtype == torch.float32
    if n == 0:
        # nothing is written: the raw call with outputs that hold a pattern
        from diff_gaussian_rasterization import _native
        keep_o, keep_s = torch.full((4,), 7.0, device=DEV), torch.full((4, 3), 7.0, device=DEV)
        ws = torch.zeros(4 * P, dtype=torch.uint8, device=DEV)
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = _native.load().gsr_mcmc_relocation(C.c_int64(P), C.c_int64(0), p(dev(x)), p(dev(ls)), None, C.c_float(0.005), p(ws), p(keep_o),
                                                p(keep_s), None)
        torch.cuda.synchronize()
        assert rc == 0 and bool((keep_o == 7).all()) and bool((keep_s == 7).all())
        return
    N = MR.multiplicity(sampled, P)
    if n == 3000:
        seen = set(N.tolist())
        assert {2, 3, 51, 52, 61} <= seen, sorted(seen)          # taken once, twice, 50 times (N = 51), 51 and 60 times (clamped)
    ref_o, ref_s = MR.relocation(x[sampled], ls[sampled], N, 0.005)
    worst = MR.check_relocation(host(out_o), host(out_s), ref_o, ref_s, f"relocation n={n}")
    print(f"relocation n={n}: worst error {worst:.3f} x the bound")
    again = mcmc.compute_relocation(dev(x), dev(ls), dev(sampled, torch.int64), 0.005)
    assert torch.equal(again[0], out_o) and torch.equal(again[1], out_s)


# ---- the row edit ---------------------------------------------------------------------------------------------------------------------
SHAPES = (("opacity", (1,), "opacity"), ("scaling", (3,), "scaling"), ("xyz", (3,), "copy"), ("rotation", (4,), "copy"),
          ("sh3", (16, 3), "copy"), ("sh0", (1, 3), "copy"), ("sh2", (9, 3), "copy"))       # widths 1 3 3 4 48 3 27


def _row_case(P, n, seed):
    rng = np.random.default_rng(seed)
    x, ls = MR.relocation_inputs(P, seed)
    perm = rng.permutation(P)
    dead, alive = perm[:n], perm[n:]
    sampled = alive[rng.integers(0, alive.size, n)]
    if n >= 60:
        sampled[:60] = alive[0]                                   # one source taken 60 times
    tensors = {}
    for name, shape, role in SHAPES:
        p = x if name == "opacity" else ls if name == "scaling" else rng.standard_normal((P,) + shape).astype(np.float32)
        tensors[name] = tuple(torch.from_numpy(np.ascontiguousarray(a)) for a in
                              (p, rng.standard_normal(p.shape).astype(np.float32), rng.random(p.shape).astype(np.float32) + 0.1))
    return tensors, torch.from_numpy(sampled), torch.from_numpy(dead)


def _run_rows(tensors, sampled, dead):
    on = {k: tuple(t.to(DEV) for t in v) for k, v in tensors.items()}
    s, d = sampled.to(DEV), None if dead is None else dead.to(DEV)
    new_o, new_s = mcmc.compute_relocation(on["opacity"][0], on["scaling"][0], s, 0.005)
    versions = {k: v[0]._version for k, v in on.items()}
    mcmc.relocate_rows([(on[name][0], on[name][1], on[name][2], role) for name, _, role in SHAPES], s, d, new_o, new_s)
    torch.cuda.synchronize()
    assert all(on[k][0]._version > versions[k] for k in ("opacity", "scaling"))
    return {k: tuple(t.cpu() for t in v) for k, v in on.items()}, new_o.cpu(), new_s.cpu()


@pytest.mark.parametrize("n", (1, 700))
@pytest.mark.parametrize("P", (1000, 4099))
def test_row_relocation_bit_for_bit(P, n):
    tensors, sampled, dead = _row_case(P, n, 100 * n + P)
    out, new_o, new_s = _run_rows(tensors, sampled, dead)
    is_src = torch.zeros(P, dtype=torch.bool); is_src[sampled] = True
    is_dead = torch.zeros(P, dtype=torch.bool); is_dead[dead] = True
    assert torch.equal(out["opacity"][0][sampled].reshape(-1), new_o) and torch.equal(out["scaling"][0][sampled], new_s)
    for name, _, role in SHAPES:
        p, m, v = out[name]
        p0, m0, v0 = tensors[name]
        assert torch.equal(p[dead], p[sampled]), name              # copied rows equal their sources
        if role == "copy":
            assert torch.equal(p[~is_dead], p0[~is_dead]), name    # ... which, for a copied tensor, did not move
        else:
            assert torch.equal(p[~(is_dead | is_src)], p0[~(is_dead | is_src)]), name
        for a, a0 in ((m, m0), (v, v0)):
            assert not a[is_src].any(), (name, "a source kept a moment")
            assert torch.equal(a[~is_src], a0[~is_src]), (name, "a moment outside the sources moved")
    again, _, _ = _run_rows(tensors, sampled, dead)
    for name in out:
        assert all(torch.equal(a, b) for a, b in zip(out[name], again[name])), name
    # dead = NULL: the new values only, every moment left alone
    grow, new_o2, new_s2 = _run_rows(tensors, sampled, None)
    assert torch.equal(new_o2, new_o) and torch.equal(new_s2, new_s)
    for name, _, role in SHAPES:
        p, m, v = grow[name]
        p0, m0, v0 = tensors[name]
        assert torch.equal(m, m0) and torch.equal(v, v0), name
        assert torch.equal(p[~is_src], p0[~is_src]), name
        assert torch.equal(p[is_src], out[name][0][is_src]), name


# ---- the position noise -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", (1e-3, 80.0))
@pytest.mark.parametrize("P", (1, 63, 64, 65, 1000, 4099))
def test_noise_against_the_restatement(P, c):
    xyz, ls, q, x, xi = MR.noise_inputs(P, 31 + P)
    run = []
    for _ in range(2):
        t = dev(xyz).requires_grad_(True)
        v0 = t._version
        mcmc.inject_position_noise(t, dev(ls), dev(q), dev(x), dev(xi), c)
        assert t._version > v0
        run.append(host(t))
    assert np.array_equal(run[0], run[1])
    worst = MR.check_noise(run[0], xyz, ls, q, x, xi, c, f"noise P={P} c={c}")
    print(f"noise P={P} c={c}: worst error {worst:.3f} x the bound")
    saturated = x.reshape(-1) >= 3.0                               # o >= 0.95: the exponential overflows, g = 0
    assert np.array_equal(run[0][saturated], xyz[saturated])
    if P >= 63:
        assert saturated.sum() > P // 8 and (run[0] != xyz).any()


# ---- the regulariser gradient ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", (1, 1000, 4099))
def test_reg_grads_against_the_restatement(P):
    _, ls, _, x, _ = MR.noise_inputs(P, 41 + P)
    rng = np.random.default_rng(P)
    g_o, g_s = (rng.standard_normal((P, 1)) * 1e-5).astype(np.float32), (rng.standard_normal((P, 3)) * 1e-5).astype(np.float32)
    go, gs = dev(g_o), dev(g_s)
    mcmc.add_regularizer_grads(dev(x), dev(ls), 0.01, 0.02, go, gs)
    ref_o, ref_s = MR.reg_delta(x, ls, 0.01, 0.02)
    w = max(MR.check_reg(host(go).astype(np.float64) - g_o, ref_o, g_o, f"reg opacity P={P}"),
            MR.check_reg(host(gs).astype(np.float64) - g_s, ref_s, g_s, f"reg scaling P={P}"))
    print(f"reg P={P}: worst error {w:.3f} x the bound")
    only_s, only_o = dev(g_s), dev(g_o)
    mcmc.add_regularizer_grads(None, dev(ls), 0.01, 0.02, None, only_s)          # a NULL side: the other is what it was
    mcmc.add_regularizer_grads(dev(x), None, 0.01, 0.02, only_o, None)
    assert torch.equal(only_s, gs) and torch.equal(only_o, go)


# ---- the model on the device ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 0))
def test_model_relocate_native(D):
    gm = MC.make_model(500, D, DEV)
    torch.manual_seed(5)
    sampled, N, worst, (old, new) = MC.check_relocate(gm, list(range(3, 500, 7)))
    print(f"model relocate D={D}: worst error {worst:.3f} x the bound, multiplicities up to {N.max()}")
    # the host path on the same old values and the same sources
    ref_o, ref_s = mcmc.compute_relocation(old["opacity"], old["scaling"], sampled, MC.MIN_OPACITY, native=False)
    MR.check_relocation(new["opacity"][sampled].numpy(), new["scaling"][sampled].numpy(), ref_o.numpy(), ref_s.numpy(), "against the host path")
    before, mom = MC.snapshot(gm)
    assert gm.mcmc_relocate(MC.MIN_OPACITY) == 0                   # no dead row: nothing happens
    after, mom2 = MC.snapshot(gm)
    for k in before:
        assert torch.equal(before[k], after[k]) and all(torch.equal(a, b) for a, b in zip(mom[k], mom2[k]))


@pytest.mark.parametrize("D", (3, 0))
def test_model_relocate_all_dead_but_one_native(D):
    torch.manual_seed(6)
    MC.all_but_one(MC.make_model(500, D, DEV), 123)


@pytest.mark.parametrize("D", (3, 0))
def test_model_grow_native(D):
    gm = MC.make_model(500, D, DEV)
    torch.manual_seed(8)
    counts = [500]
    assert MC.check_grow(gm, 600) == 25
    counts.append(gm._xyz.shape[0])
    MC.check_capture_restore(gm)
    for _ in range(4):
        MC.check_grow(gm, 600, detailed=False)
        counts.append(gm._xyz.shape[0])
    assert counts == [500, 525, 551, 578, 600, 600]
    assert gm.max_radii2D.is_cuda and gm.denom.is_cuda


def test_model_noise_and_regularizer_native():
    gm = MC.make_model(1001, 2, DEV)
    xyz0, v0 = gm._xyz.detach().clone(), gm._xyz._version
    noise = torch.randn(1001, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    s_before = gm.get_scaling                                      # an evaluation the cache holds
    gm.mcmc_inject_noise(80.0, noise=noise)
    assert gm._xyz._version > v0 and gm.get_scaling is s_before   # xyz is not an input of the activations: the cache stays
    MR.check_noise(host(gm._xyz), host(xyz0), host(gm._scaling), host(gm._rotation), host(gm._opacity), host(noise), 80.0, "model noise")
    gm.mcmc_inject_noise(1.0)
    assert torch.isfinite(gm._xyz).all()
    gm.mcmc_add_regularizer_grads(0.01, 0.02)
    ref_o, ref_s = MR.reg_delta(host(gm._opacity), host(gm._scaling), 0.01, 0.02)
    MR.check_reg(host(gm._opacity.grad), ref_o, np.zeros(1001), "model reg opacity")
    MR.check_reg(host(gm._scaling.grad), ref_s, np.zeros(3003), "model reg scaling")
    # the activation cache sees a relocation
    MC.kill(gm, [4, 5])
    gm.mcmc_relocate(MC.MIN_OPACITY)
    assert float(gm.get_opacity.detach().min()) >= MC.MIN_OPACITY * (1 - 1e-6)


# ---- the training loop ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optimizer_type", ("default", "sparse_adam"))
def test_training_loop_under_the_mcmc_strategy(optimizer_type):
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    torch.manual_seed(0)
    W, H = 160, 112
    cams = [c.to(DEV) for c in S.arc_cameras(W, H, 4)]
    scene = S.make_scene(4000, W, H, 2, 30, scale_lo=0.01, scale_hi=0.08)
    truth = GaussianModel(2); truth.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    gm = GaussianModel(2); gm.adopt_scene(scene, device=DEV)
    with torch.no_grad():                                          # a start away from the truth, with some rows dead
        gm._xyz.add_(0.01 * torch.randn_like(gm._xyz))
        gm._opacity[::50] = -7.0
    opt = replace(OptimizationDefaults(), densify_strategy="mcmc", mcmc_cap_max=5000, densify_from_iter=10, densification_interval=10,
                  optimizer_type=optimizer_type)
    gm.training_setup(opt)
    counts, floor, losses = [], [], []

    def on_iteration(it, loss, g):
        counts.append(g._xyz.shape[0])
        losses.append(float(loss.detach()))
        if 10 < it < 80 and it % 10 == 0:                          # right after a refinement
            floor.append(float(torch.sigmoid(g._opacity.detach()).min()))
    train(gm, cams, targets, opt, Pipe(), bg, iterations=80, scene_extent=3.0, on_iteration=on_iteration)
    want, P = [], 4000
    for it in range(1, 81):
        if 10 < it < 80 and it % 10 == 0:
            P = min(5000, int(1.05 * P))
        want.append(P)
    assert counts == want and 5000 not in counts[:59] and counts[59] == counts[-1] == 5000
    assert len(floor) == 6 and min(floor) >= opt.mcmc_min_opacity * (1 - 1e-6), floor
    assert all(np.isfinite(losses))
    for k, t in gm._t.items():
        st = gm.optimizer.state[t]
        assert t.shape[0] == st["exp_avg"].shape[0] == st["exp_avg_sq"].shape[0] == 5000, k
        assert torch.isfinite(t).all() and torch.isfinite(st["exp_avg"]).all() and torch.isfinite(st["exp_avg_sq"]).all(), k
    assert gm.max_radii2D.shape[0] == gm.xyz_gradient_accum.shape[0] == gm.denom.shape[0] == 5000
