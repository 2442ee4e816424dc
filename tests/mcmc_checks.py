"""Checks of GaussianModel.mcmc_relocate / mcmc_grow that tests/test_mcmc_ref.py runs on the host path and tests/test_gpu_mcmc.py on
the device with the native path: one statement of what the two edits must leave behind."""
from dataclasses import replace

import numpy as np
import torch

import mcmc_ref as MR
import scene_synth as S
from scene import GaussianModel, OptimizationDefaults
from scene.gaussian_model import TABLE

MIN_OPACITY = 0.005


def make_model(P, D, device, steps=2, seed=11):
    """A model of P Gaussians with SH degree D under the "mcmc" strategy, after `steps` optimizer steps on random gradients (so
    that both moments are non-zero everywhere)."""
    gm = GaussianModel(D)
    gm.adopt_scene(S.make_scene(P, 64, 64, D, 7), device=device)
    gm.training_setup(replace(OptimizationDefaults(), densify_strategy="mcmc"))
    gen = torch.Generator().manual_seed(seed)
    for _ in range(steps):
        for k in TABLE:
            gm._t[k].grad = torch.randn(gm._t[k].shape, generator=gen).to(device)
        gm.optimizer.step()
    gm.optimizer.zero_grad(set_to_none=True)
    return gm


def kill(gm, rows):
    with torch.no_grad():
        gm._opacity[torch.as_tensor(rows, device=gm.device)] = -8.0          # sigmoid(-8) = 3.4e-4 < 0.005


def snapshot(gm):
    """({name: param}, {name: (exp_avg, exp_avg_sq)}) as host copies."""
    params = {k: gm._t[k].detach().cpu().clone() for k in TABLE}
    moments = {}
    for k in TABLE:
        st = gm.optimizer.state.get(gm._t[k]) if gm.optimizer is not None else None
        if st:
            moments[k] = (st["exp_avg"].cpu().clone(), st["exp_avg_sq"].cpu().clone())
    return params, moments


def sources_of(rows, xyz_new, xyz_old):
    """For every row in `rows`: the old row whose xyz it now holds bit for bit (the scene's means are distinct)."""
    index = {xyz_old[i].numpy().tobytes(): i for i in range(xyz_old.shape[0])}
    return torch.tensor([index[xyz_new[int(r)].numpy().tobytes()] for r in rows], dtype=torch.int64)


def check_sources(params_old, params_new, sampled, what):
    """The sources carry the restatement's values computed from the OLD ones; their copied leaves keep their bits."""
    P = params_old["xyz"].shape[0]
    N = MR.multiplicity(sampled.numpy(), P)
    ref_o, ref_s = MR.relocation(params_old["opacity"][sampled].numpy(), params_old["scaling"][sampled].numpy(), N, MIN_OPACITY)
    worst = MR.check_relocation(params_new["opacity"][sampled].numpy(), params_new["scaling"][sampled].numpy(), ref_o, ref_s, what)
    for k in ("xyz", "features", "rotation"):
        assert torch.equal(params_new[k][sampled], params_old[k][sampled]), (what, k)
    return worst, N


def check_relocate(gm, dead_rows, generator=None, native=None, what="relocate"):
    P = gm._xyz.shape[0]
    kill(gm, dead_rows)
    old, mom_old = snapshot(gm)
    n = gm.mcmc_relocate(MIN_OPACITY, generator=generator, native=native)
    new, mom_new = snapshot(gm)
    dead = torch.nonzero(torch.sigmoid(old["opacity"]).reshape(-1) <= MIN_OPACITY).reshape(-1)       # the killed rows and any the scene had
    assert set(dead_rows) <= set(dead.tolist()) and n == dead.numel() and gm._xyz.shape[0] == P
    sampled = sources_of(dead, new["xyz"], old["xyz"])
    is_dead = torch.zeros(P, dtype=torch.bool); is_dead[dead] = True
    is_src = torch.zeros(P, dtype=torch.bool); is_src[sampled] = True
    assert not (is_dead & is_src).any(), "a dead row was sampled as a source"
    for k in TABLE:                                               # dead rows equal their (updated) sources in all five leaves
        assert torch.equal(new[k][dead], new[k][sampled]), (what, k)
        untouched = ~(is_dead | is_src)
        assert torch.equal(new[k][untouched], old[k][untouched]), (what, k, "an untouched row moved")
    worst, N = check_sources(old, new, sampled, what)
    assert set(mom_new) == set(mom_old) == set(TABLE)
    for k in TABLE:
        for a, b in zip(mom_new[k], mom_old[k]):
            assert not a[is_src].any(), (what, k, "a source kept a moment")
            assert torch.equal(a[~is_src], b[~is_src]), (what, k, "a moment outside the sources moved")
    return sampled, N, worst, (old, new)


def check_grow(gm, cap_max, generator=None, native=None, what="grow", detailed=True):
    """detailed = False (a model that grew before holds equal means, so sources cannot be told from earlier copies): the count and
    the shapes only."""
    P = gm._xyz.shape[0]
    old, mom_old = snapshot(gm)
    want = max(0, min(cap_max, int(1.05 * P)) - P)
    n = gm.mcmc_grow(cap_max, MIN_OPACITY, generator=generator, native=native)
    assert n == want and gm._xyz.shape[0] == P + want <= max(cap_max, P), (what, n, want)
    new, mom_new = snapshot(gm)
    assert gm.max_radii2D.shape[0] == gm.xyz_gradient_accum.shape[0] == gm.denom.shape[0] == P + n
    if n == 0:
        for k in TABLE:
            assert torch.equal(new[k], old[k]), (what, k)
        return 0
    if not detailed:
        return n
    added = torch.arange(P, P + n)
    sampled = sources_of(added, new["xyz"], old["xyz"])
    for k in TABLE:                                               # appended rows equal the updated sources
        assert torch.equal(new[k][added], new[k][sampled]), (what, k)
        is_src = torch.zeros(P, dtype=torch.bool); is_src[sampled] = True
        assert torch.equal(new[k][:P][~is_src], old[k][~is_src]), (what, k, "a row that was not sampled moved")
    check_sources(old, {k: v[:P] for k, v in new.items()}, sampled, what)
    for k in TABLE:
        for a, b in zip(mom_new[k], mom_old[k]):
            assert torch.equal(a[:P], b), (what, k, "a source lost its moment")
            assert not a[P:].any(), (what, k, "an appended row has a moment")
    return n


def check_capture_restore(gm):
    gm2 = GaussianModel(gm.max_sh_degree)
    gm2.restore(gm.capture(), replace(OptimizationDefaults(), densify_strategy="mcmc"))
    a, ma = snapshot(gm)
    b, mb = snapshot(gm2)
    for k in TABLE:
        assert torch.equal(a[k], b[k]), k
        for x, y in zip(ma[k], mb[k]):
            assert torch.equal(x, y), k
    assert gm2.densify_strategy == "mcmc" and gm2.max_radii2D.shape[0] == gm._xyz.shape[0]


def all_but_one(gm, keep, generator=None, native=None):
    """All rows dead but `keep`: every row becomes that source at N = 51."""
    P = gm._xyz.shape[0]
    rows = [i for i in range(P) if i != keep]
    kill(gm, rows)
    with torch.no_grad():
        gm._opacity[keep] = 1.0
    old, _ = snapshot(gm)
    assert gm.mcmc_relocate(MIN_OPACITY, generator=generator, native=native) == P - 1
    new, _ = snapshot(gm)
    ref_o, ref_s = MR.relocation(old["opacity"][keep:keep + 1].numpy(), old["scaling"][keep:keep + 1].numpy(), np.array([MR.MAX_RATIO]),
                                 MIN_OPACITY)
    MR.check_relocation(new["opacity"][keep:keep + 1].numpy(), new["scaling"][keep:keep + 1].numpy(), ref_o, ref_s, "all but one")
    for k in TABLE:
        assert torch.equal(new[k], new[k][keep:keep + 1].expand_as(new[k])), k
