"""CPU checks of sparse Adam (fused_adam.SparseFusedAdam, gsr_adam_step_sparse_multi): the C ABI's refusals without a GPU, the
per-row rule on host tensors against a float64 loop written out here, hidden rows keep their bits, an all-true mask is FusedAdam's
step, and the model's optimizer_type switch with its parameter-store surgery."""
import copy
import ctypes as C
import math
import os
import re
from dataclasses import replace

import pytest
import torch

import scene_synth as S
from fused_adam import FusedAdam, SparseFusedAdam
from scene import GaussianModel, OptimizationDefaults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = lambda P: [(P, 3), (P, 16, 3), (P, 1), (P, 4)]
SIZES = (1, 3, 257, 1366, 4099)


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


def test_abi_symbol_and_refusals_without_gpu(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    assert re.search(r"^int gsr_adam_step_sparse_multi\(int32_t count, const gsr_adam_tensor \*tensors, int64_t rows,\s*"
                     r"const void \*visible, int32_t visible_elem_bytes,\s*float beta1, float beta2, float eps, void \*stream\);", hdr, re.M)
    lib = native.load()
    assert hasattr(lib, "gsr_adam_step_sparse_multi") and "gsr_adam_step_sparse_multi" in native.EXPORTS
    assert lib.gsr_version() == 12
    fake = C.c_void_p(256)                                       # never dereferenced: every refusal comes before any launch

    def call(n=30, rows=10, visible=fake, elem_bytes=1, step=1, row_len=0, split=0, count=1):
        t = (native.AdamTensor * 1)()
        t[0].param = t[0].grad = t[0].exp_avg = t[0].exp_avg_sq = 256
        t[0].n, t[0].lr, t[0].lr_tail, t[0].step, t[0].row_len, t[0].split = n, 0.01, 0.01, step, row_len, split
        rc = lib.gsr_adam_step_sparse_multi(C.c_int32(count), t, C.c_int64(rows), visible, C.c_int32(elem_bytes), C.c_float(0.9),
                                            C.c_float(0.999), C.c_float(1e-15), None)
        return rc, lib.gsr_last_error()
    rc, msg = call(n=31)
    assert rc == -1 and b"n % rows != 0" in msg
    for b in (0, 2, 8):
        rc, msg = call(elem_bytes=b)
        assert rc == -1 and b"visible_elem_bytes" in msg
    rc, msg = call(visible=None)
    assert rc == -1 and b"visible is NULL" in msg
    for s in (0, -3):
        rc, msg = call(step=s)
        assert rc == -1 and b"step >= 1" in msg
    rc, msg = call(row_len=4, split=1)                           # the width is 3
    assert rc == -1 and b"row_len" in msg
    rc, msg = call(count=native.ADAM_MAX_TENSORS + 1)
    assert rc == -1 and b"tensors" in msg
    # nothing to do is not an error, and launches nothing: no tensors; no rows
    assert call(count=0)[0] == 0
    assert call(n=0, rows=0, visible=None)[0] == 0


def _groups(ps):
    return [{"params": [p], "lr": 0.01 * (i + 1), "name": str(i)} for i, p in enumerate(ps)]


def _random_mask(P, fraction, gen):
    if fraction == 0.0:
        return torch.zeros(P, dtype=torch.bool)
    if fraction == 1.0:
        return torch.ones(P, dtype=torch.bool)
    return torch.rand(P, generator=gen) < fraction


@pytest.mark.parametrize("bias_correction", (True, False))
@pytest.mark.parametrize("P", SIZES)
def test_rule_against_float64(P, bias_correction):
    """The conditions of test_fused_adam_matches_torch_adam (6 steps, N(0,1) gradients, the 4th all zero, lr 0.01 (i + 1), eps = 1e-15)
    with a fresh random mask per step, against the per-row rule in float64 with the GLOBAL step count in the bias corrections."""
    b1, b2, eps = 0.9, 0.999, 1e-15
    for fraction in (0.0, 0.1, 0.5, 1.0):
        gen = torch.Generator().manual_seed(1000 * P + int(10 * fraction))
        ps = [torch.randn(*s, generator=gen).requires_grad_(True) for s in SHAPES(P)]
        opt = SparseFusedAdam(_groups(ps), lr=0.0, eps=eps, native=False, bias_correction=bias_correction)
        p64 = [p.detach().double().clone() for p in ps]
        m64, v64 = [torch.zeros_like(p) for p in p64], [torch.zeros_like(p) for p in p64]
        for it in range(6):
            mask = _random_mask(P, fraction, gen)
            for p in ps:
                p.grad = torch.randn(p.shape, generator=gen) * (0.0 if it == 3 else 1.0)
            for i, p in enumerate(ps):
                step, lr, g = it + 1, 0.01 * (i + 1), p.grad.double()
                bc1, bc2 = (1 - b1 ** step, 1 - b2 ** step) if bias_correction else (1.0, 1.0)
                r = mask                                             # the rule, on the visible rows only
                m64[i][r] = m64[i][r] + (g[r] - m64[i][r]) * (1 - b1)
                v64[i][r] = v64[i][r] * b2 + (1 - b2) * g[r] * g[r]
                p64[i][r] = p64[i][r] - (lr / bc1) * (m64[i][r] / (v64[i][r].sqrt() / math.sqrt(bc2) + eps))
            opt.step(visibility=(mask, mask.to(torch.uint8), mask.to(torch.int32) * 5 - 2 * (~mask).to(torch.int32))[it % 3])
        for i, p in enumerate(ps):
            ep = float((p.detach().double() - p64[i]).abs().max())
            ev = float((opt.state[p]["exp_avg_sq"].double() - v64[i]).abs().max()) if opt.state[p] else 0.0
            print(f"P={P} fraction={fraction} bias_correction={bias_correction} shape={tuple(p.shape)}: |p - p64| = {ep:.3e}, |v - v64| = {ev:.3e}")
            assert ep <= 2e-6 * max(1.0, float(p.detach().abs().max())), (fraction, i, ep)
            assert ev <= 1e-6, (fraction, i, ev)
            assert float(opt.state[p]["step"]) == 6.0


@pytest.mark.parametrize("P", SIZES)
def test_hidden_rows_keep_their_bits_and_the_step_advances(P):
    gen = torch.Generator().manual_seed(P)
    ps = [torch.randn(*s, generator=gen).requires_grad_(True) for s in SHAPES(P)]
    opt = SparseFusedAdam(_groups(ps), lr=0.0, eps=1e-15, native=False)
    for it in range(3):
        mask = torch.rand(P, generator=gen) < 0.5
        if it == 2:
            mask[:] = False
        before = [(p.detach().clone(), opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) if opt.state[p]
                  else (p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen)
            p.grad[~mask] = float("nan")                         # a hidden row's gradient is not used
        opt.step(visibility=mask)
        for p, (p0, m0, v0) in zip(ps, before):
            st = opt.state[p]
            assert torch.equal(p.detach()[~mask], p0[~mask]) and torch.equal(st["exp_avg"][~mask], m0[~mask])
            assert torch.equal(st["exp_avg_sq"][~mask], v0[~mask])
            assert torch.isfinite(p.detach()).all() and float(st["step"]) == it + 1
            if mask.any():
                assert not torch.equal(p.detach()[mask], p0[mask])


def _split_groups(ps):
    """The model's layout: the SH table steps column 0 with its own lr and the others with the (parameter-less) group "f_rest"'s."""
    return [{"params": [ps[0]], "lr": 0.00016, "name": "xyz"},
            {"params": [ps[1]], "lr": 0.0025, "name": "f_dc", "head_cols": 1, "tail": "f_rest"},
            {"params": [], "lr": 0.000125, "name": "f_rest"},
            {"params": [ps[2]], "lr": 0.05, "name": "opacity"}, {"params": [ps[3]], "lr": 0.001, "name": "rotation"}]


@pytest.mark.parametrize("how", ("all_true_bool", "all_positive_radii", "none"))
def test_all_true_mask_and_no_mask_are_the_dense_step(how):
    P = 257
    gen = torch.Generator().manual_seed(11)
    ps = [torch.randn(*s, generator=gen).requires_grad_(True) for s in SHAPES(P)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]
    sparse, dense = SparseFusedAdam(_split_groups(ps), lr=0.0, eps=1e-15, native=False), FusedAdam(_split_groups(qs), lr=0.0, eps=1e-15, native=False)
    mask = {"all_true_bool": torch.ones(P, dtype=torch.bool), "all_positive_radii": torch.arange(1, P + 1, dtype=torch.int32), "none": None}[how]
    for it in range(3):
        for p, q in zip(ps, qs):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad = p.grad.clone()
        sparse.step(visibility=mask) if it else sparse.step(mask)
        dense.step()
        for p, q in zip(ps, qs):
            assert torch.equal(p.detach(), q.detach())
            for k in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(sparse.state[p][k], dense.state[q][k]), k
    assert sparse.state_dict()["state"].keys() == dense.state_dict()["state"].keys()
    dense.load_state_dict(sparse.state_dict())                   # same layout


def test_native_refuses_host_tensors_and_bad_masks():
    p = torch.randn(10, 3, requires_grad=True)
    p.grad = torch.randn(10, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        SparseFusedAdam([p], native=True).step(visibility=torch.ones(10, dtype=torch.bool))
    with pytest.raises(TypeError, match="bool, uint8 or int32"):
        SparseFusedAdam([p], native=False).step(visibility=torch.ones(10))


def _model(P=500, D=3, **opt):
    gm = GaussianModel(D)
    gm.adopt_scene(S.make_scene(P, 64, 64, D, 7), device="cpu")
    gm.training_setup(replace(OptimizationDefaults(), **opt))
    return gm


def _set_grads(gm, gen):
    for g in gm.optimizer.param_groups:
        for p in g["params"]:
            p.grad = torch.randn(p.shape, generator=gen)


def test_model_builds_the_optimizer_its_arguments_name():
    assert OptimizationDefaults().optimizer_type == "default"
    gm = _model(optimizer_type="sparse_adam")
    assert type(gm.optimizer) is SparseFusedAdam and gm.optimizer.bias_correction
    assert [g["name"] for g in gm.optimizer.param_groups] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    f_dc = gm.optimizer.param_groups[1]
    assert f_dc["params"][0] is gm._features and f_dc["head_cols"] == 1 and f_dc["tail"] == "f_rest" and not gm.optimizer.param_groups[2]["params"]
    assert type(_model().optimizer) is FusedAdam
    with pytest.raises(ValueError, match="optimizer_type"):
        _model(optimizer_type="sparse")


def test_model_surgery_keeps_sparse_moments_aligned_with_rows():
    gen = torch.Generator().manual_seed(5)
    gm = _model(optimizer_type="sparse_adam")
    P = 500
    _set_grads(gm, gen)
    mask = torch.zeros(P, dtype=torch.bool); mask[::2] = True
    xyz0 = gm._xyz.detach().clone()
    gm.optimizer.step(visibility=mask)
    m = {k: gm.optimizer.state[gm._t[k]]["exp_avg"].clone() for k in gm._t}
    assert all(float(m[k][~mask].abs().max()) == 0.0 and float(m[k][mask].abs().min()) > 0.0 for k in m)     # moments only where seen
    assert torch.equal(gm._xyz.detach()[~mask], xyz0[~mask])
    # densify-style edit: drop every third row, append 7 clones
    keep = torch.ones(P, dtype=torch.bool); keep[::3] = False
    extra = {k: gm._t[k].detach()[:7].clone() for k in gm._t}
    tables = {k: gm._t[k].detach().clone() for k in gm._t}
    gm._rebuild(keep=keep, extra=extra)
    n = int(keep.sum())
    for k in gm._t:
        st = gm.optimizer.state[gm._t[k]]
        assert gm._t[k].shape[0] == n + 7 and st["exp_avg"].shape == gm._t[k].shape == st["exp_avg_sq"].shape
        assert torch.equal(gm._t[k].detach()[:n], tables[k][keep]) and torch.equal(st["exp_avg"][:n], m[k][keep])
        assert float(st["exp_avg"][n:].abs().max()) == 0.0 and float(st["step"]) == 1.0
    # right after the edit no leaf has a gradient: the frame's mask (old size) steps nothing and is no error
    before = {k: gm._t[k].detach().clone() for k in gm._t}
    gm.optimizer.step(visibility=mask)
    assert all(torch.equal(gm._t[k].detach(), before[k]) and float(gm.optimizer.state[gm._t[k]]["step"]) == 1.0 for k in gm._t)
    # with gradients, a mask of another length names the group it fails on
    _set_grads(gm, gen)
    with pytest.raises(ValueError, match=r"group 'xyz'.*500 rows"):
        gm.optimizer.step(visibility=mask)
    new_mask = torch.rand(n + 7, generator=gen) < 0.5
    gm.optimizer.step(visibility=(new_mask.to(torch.int32) * 3))           # radii-style
    st = gm.optimizer.state[gm._xyz]
    assert float(st["step"]) == 2.0 and torch.equal(st["exp_avg"][:n][~new_mask[:n]], m["xyz"][keep][~new_mask[:n]])


def test_model_capture_restore_round_trips_with_sparse_adam():
    gen = torch.Generator().manual_seed(6)
    opt = replace(OptimizationDefaults(), optimizer_type="sparse_adam")
    gm = _model(200, optimizer_type="sparse_adam")
    _set_grads(gm, gen)
    mask = torch.rand(200, generator=gen) < 0.5
    gm.optimizer.step(visibility=mask)
    snap = gm.capture()
    file = lambda: snap[:10] + (copy.deepcopy(snap[10]),) + snap[11:]      # as a checkpoint file read twice would: the live state_dict
                                                                           # shares its tensors (the step counters) with whoever loads it
    assert [g["name"] for g in snap[10]["param_groups"]] == ["xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation"]
    gm2 = GaussianModel(3)
    gm2.restore(file(), opt)
    assert type(gm2.optimizer) is SparseFusedAdam
    gm3 = GaussianModel(3)
    gm3.restore(file(), OptimizationDefaults())                   # the state is FusedAdam's: the other optimizer reads it too
    assert type(gm3.optimizer) is FusedAdam
    for k in gm._t:
        for other in (gm2, gm3):
            assert torch.equal(other._t[k].detach(), gm._t[k].detach())
            for s in ("step", "exp_avg", "exp_avg_sq"):
                assert torch.equal(other.optimizer.state[other._t[k]][s], gm.optimizer.state[gm._t[k]][s]), (k, s)
    # both restored models continue alike under an all-true mask / the dense step
    for other in (gm, gm2, gm3):
        _set_grads(other, torch.Generator().manual_seed(9))
    gm.optimizer.step(visibility=torch.ones(200, dtype=torch.bool)); gm2.optimizer.step(visibility=torch.ones(200, dtype=torch.uint8)); gm3.optimizer.step()
    for k in gm._t:
        assert torch.equal(gm2._t[k].detach(), gm._t[k].detach()) and torch.equal(gm3._t[k].detach(), gm._t[k].detach())
