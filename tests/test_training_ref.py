"""CPU checks of tests/training_ref.py, the float64 reference that tests/test_gpu_training_kernels.py holds the Adam, activation and
densification kernels to: it equals torch.optim.Adam and autograd in float64; correct float32 implementations (FusedAdam(native=False),
torch's float32 getters and autograd, a float32 restatement of the kernels' expressions) stay inside its ceilings on the very inputs the
GPU tests use; planted defects miss the bound by orders of magnitude; and the C entry points refuse bad arguments before any launch."""
import ctypes as C
import os

import pytest
import torch

import training_ref as R
from fused_adam import FusedAdam

B1, B2 = R.ADAM_BETAS
EPS = R.ADAM_EPS
LRS = (0.0025, 0.000125)


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


# ---- the reference is right --------------------------------------------------------------------------------------------------------
def _torch_adam64(tensors_lrs, step, b1, b2, eps):
    """One step of torch.optim.Adam in float64 from an installed state with step count `step`: [(p, g, m, v, lr)] -> [(p', m', v')]."""
    ps = [p.double().clone().requires_grad_(True) for p, *_ in tensors_lrs]
    opt = torch.optim.Adam([{"params": [q], "lr": lr} for q, (*_, lr) in zip(ps, tensors_lrs)], lr=0.0, betas=(b1, b2), eps=eps, foreach=False)
    for q, (_, g, m, v, _) in zip(ps, tensors_lrs):
        q.grad = g.double().clone()
        opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
    opt.step()
    return [(q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]) for q in ps]


def _rel(a, b):
    return float(((a - b).abs() / b.abs().clamp_min(R.TINY)).max())


@pytest.mark.parametrize("step", (1, 2, 1000))
def test_adam_step64_equals_torch_adam_in_float64(step):
    """torch.optim.Adam keeps lr / bc1 and sqrt(bc2) in float64, so the comparison is made with round_derived=False and the float32-rounded
    beta, eps and lr on both sides; the two roundings the kernels add on top move the step size and 1 / sqrt(bc2) by at most u each."""
    b1, b2, eps = R.f32(B1), R.f32(B2), R.f32(EPS)
    p, g, m, v = R.adam_state(4131, 100 + step)
    (p1, m1, v1), _ = R.adam_step64(p, g, m, v, LRS[0], LRS[0], step, 0, 0, B1, B2, EPS, round_derived=False)
    (tp, tm, tv), = _torch_adam64([(p, g, m, v, R.f32(LRS[0]))], step, b1, b2, eps)
    worst = max(_rel(p1, tp), _rel(m1, tm), _rel(v1, tv))
    print(f"step {step}: plain worst relative difference {worst:.2e}")
    assert worst <= 1e-12
    # the split form against Adam on the two column ranges
    for row_len, split in ((27, 3), (27, 0), (27, 27), (5, 4), (4, 1)):
        rows = R.adam_split_rows(row_len)
        p, g, m, v = (t.reshape(rows, row_len) for t in R.adam_state(rows * row_len, 200 + row_len + split))
        (p1, m1, v1), _ = R.adam_step64(p, g, m, v, LRS[0], LRS[1], step, row_len, split, B1, B2, EPS, round_derived=False)
        parts = [(tuple(t[:, :split] for t in (p, g, m, v)) + (R.f32(LRS[0]),)), (tuple(t[:, split:] for t in (p, g, m, v)) + (R.f32(LRS[1]),))]
        out = _torch_adam64(parts, step, b1, b2, eps)
        for got, k in ((p1, 0), (m1, 1), (v1, 2)):
            want = torch.cat([out[0][k], out[1][k]], dim=1).reshape(-1)
            assert _rel(got, want) <= 1e-12, (row_len, split, k)
    s64, s32 = R.adam_scalars(LRS[0], LRS[1], step, B1, B2, EPS, False), R.adam_scalars(LRS[0], LRS[1], step, B1, B2, EPS, True)
    for name in ("head", "tail", "inv"):
        assert abs(getattr(s32, name) / getattr(s64, name) - 1.0) <= R.U, name
    assert (s32.omb1, s32.omb2) == (1.0 - R.f32(B1), 1.0 - R.f32(B2))          # 1.f - beta is exact


def test_activations64_equal_float64_autograd():
    (sc, ro, op), grads = R.activation_inputs(1000, 1000)
    leaves = [t.double().requires_grad_(True) for t in (sc, ro, op)]
    want = (torch.exp(leaves[0]), torch.nn.functional.normalize(leaves[1], eps=R.NORMALIZE_EPS), torch.sigmoid(leaves[2]))
    vals, _ = R.activations64(sc, ro, op)
    for a, b in zip(vals, want):
        assert _rel(a, b.detach()) <= 1e-12
    torch.autograd.backward(want, [g.double() for g in grads])
    d, _ = R.activations_backward64(want[0], ro, want[2], *grads)
    n = ro.double().norm(dim=-1)
    assert float(n[0]) == 0.0 and 0.0 < float(n[1]) < R.NORMALIZE_EPS < float(n[2]) < 4 * R.NORMALIZE_EPS      # the three rows around eps
    for name, mine, leaf in zip(("scaling", "rotation", "opacity"), d, leaves):
        # relative to the largest term of the row: the two terms of the quaternion's gradient cancel
        scale = leaf.grad.abs().amax(-1, keepdim=True).clamp_min(R.TINY)
        err = float(((mine - leaf.grad).abs() / scale).max())
        print(f"{name}: worst difference {err:.2e} of the row's largest gradient")
        assert err <= 1e-12, name


def test_densify_stats64_equals_masked_torch_ops():
    for P in R.DENSIFY_SIZES:
        radii, grad, mr, acc, den = R.densify_inputs(P, P)
        (mr1, acc1, den1), _ = R.densify_stats64(radii, grad, mr, acc, den)
        vis = radii > 0
        wm, wa, wd = mr.double().clone(), acc.double().clone(), den.double().clone()
        wm[vis] = torch.max(wm[vis], radii[vis].float().double())
        wa[vis] += torch.norm(grad.double()[vis, :2], dim=-1, keepdim=True)
        wd[vis] += 1
        assert torch.equal(mr1, wm) and torch.equal(den1, wd.reshape(-1)) and _rel(acc1, wa.reshape(-1)) <= 1e-15
        assert bool(vis.any()) and (P < 4 or bool((~vis).any())) and torch.isfinite(acc1).all()
    assert float(torch.tensor([2 ** 24 + 1], dtype=torch.int32).float()) == 2.0 ** 24


# ---- correct float32 implementations stay inside the ceilings, on the inputs the GPU tests use ------------------------------------------
def _adam32(p, g, m, v, lr, lr_tail, step, row_len, split, mutate=None):
    """The kernels' expressions in float32 torch ops (no contraction).  `mutate` plants a defect."""
    s = R.adam_scalars(lr, lr_tail, step + (1 if mutate == "step_off_by_one" else 0), B1, B2, EPS)
    p, g, m, v = (t.reshape(-1).clone() for t in (p, g, m, v))
    m1 = m + (g - m) * s.omb1
    v1 = v * s.b2 + s.omb2 * g * g
    st = torch.full_like(p, s.head)
    if row_len:
        i = torch.arange(p.numel())
        col = i % row_len
        if mutate == "no_row_wrap":                                   # a float4's columns counted on from its first, past the row's end
            body = i < p.numel() // 4 * 4
            col = torch.where(body, (i // 4 * 4) % row_len + i % 4, col)
        head, tail = (s.tail, s.head) if mutate == "lr_swapped" else (s.head, s.tail)
        st = torch.where(col <= split if mutate == "le_split" else col < split, torch.tensor(head, dtype=torch.float32),
                         torch.tensor(tail, dtype=torch.float32))
    return p - st * (m1 / (v1.sqrt() * s.inv + s.eps)), m1, v1


def _fused_adam_cpu(p, g, m, v, lr, lr_tail, step, row_len, split):
    """FusedAdam(native=False) from an installed state; the split through its own head_cols group."""
    b = (R.f32(B1), R.f32(B2))
    if row_len and 0 < split < row_len:
        q = p.reshape(-1, row_len).clone().requires_grad_(True)
        opt = FusedAdam([{"params": [q], "lr": R.f32(lr), "name": "h", "head_cols": split, "tail": "t"}, {"params": [], "lr": R.f32(lr_tail), "name": "t"}],
                        lr=0.0, betas=b, eps=R.f32(EPS), native=False)
    else:
        q = p.reshape(-1).clone().requires_grad_(True)
        opt = FusedAdam([{"params": [q], "lr": R.f32(lr if (not row_len or split == row_len) else lr_tail)}], lr=0.0, betas=b, eps=R.f32(EPS), native=False)
    q.grad = g.reshape(q.shape).clone()
    opt.state[q] = {"step": torch.tensor(float(step - 1)), "exp_avg": m.reshape(q.shape).clone(), "exp_avg_sq": v.reshape(q.shape).clone()}
    opt.step()
    return q.detach(), opt.state[q]["exp_avg"], opt.state[q]["exp_avg_sq"]


def _adam_ratios(out, ref, scl):
    return {"adam_m": R.worst(out[1], ref[1], scl[0]), "adam_v": R.worst(out[2], ref[2], scl[1]), "adam_p": R.worst_p(out[0], ref[0], scl[2])}


def test_correct_float32_adam_stays_inside_the_ceilings():
    top = {impl: {"adam_m": 0.0, "adam_v": 0.0, "adam_p": 0.0} for impl in ("restatement", "FusedAdam(native=False)")}
    big = [(R.ADAM_WRAP_PLAIN, 0, 0, 7, 0.01, 0.01, 41), (R.ADAM_WRAP_SPLIT[0] * R.ADAM_WRAP_SPLIT[1], R.ADAM_WRAP_SPLIT[1], 3, 2, LRS[0], LRS[1], 42)]
    for n, row_len, split, step, lr, lr_tail, seed in R.adam_cases() + big:
        p, g, m, v = R.adam_state(n, seed)
        ref, scl = R.adam_step64(p, g, m, v, lr, lr_tail, step, row_len, split, B1, B2, EPS)
        for impl, out in (("restatement", _adam32(p, g, m, v, lr, lr_tail, step, row_len, split)),
                          ("FusedAdam(native=False)", _fused_adam_cpu(p, g, m, v, lr, lr_tail, step, row_len, split))):
            assert all(bool(torch.isfinite(t).all()) for t in out), (impl, n, row_len, split, step)
            for k, r in _adam_ratios(out, ref, scl).items():
                assert r <= R.CEIL[k], (impl, k, r, n, row_len, split, step)
                top[impl][k] = max(top[impl][k], r)
            for i in R.adam_planted(n):                                # g = m = v = 0: p keeps its bits
                assert R.bits_equal(out[0].reshape(-1)[i:i + 1], p[i:i + 1])
    for impl, t in top.items():
        print(f"{impl}: worst ratios m' {t['adam_m']:.2f} u S_m, v' {t['adam_v']:.2f} u S_v, p' beyond u |p'|: {t['adam_p']:.2f} u U")


def test_the_kernels_own_adam_rule_stays_inside_the_asserted_bounds(tmp_path):
    """csrc/gsr_math.h adam_update and adam_step_size, the functions every path of k_adam_multi and k_adam_sparse_multi calls, compiled for
    the host without contraction (tests/host_harness.cpp hh_adam_step): every multiply-add of the rule is an explicit fmaf, so this is the
    arithmetic of the device, held to the bounds the GPU tests assert (R.K, not the looser R.CEIL) on their inputs."""
    import binning_ref
    hh = binning_ref.build_harness(str(tmp_path))
    ptr, f = (lambda t: C.c_void_p(t.data_ptr())), C.c_float
    top = dict.fromkeys(("adam_m", "adam_v", "adam_p"), 0.0)
    for n, row_len, split, step, lr, lr_tail, seed in R.adam_cases() + R.ADAM_EIGHT:
        p, g, m, v = R.adam_state(n, seed)
        s = R.adam_scalars(lr, lr_tail, step, B1, B2, EPS)
        out = [t.clone() for t in (p, m, v)]
        hh.hh_adam_step(C.c_int64(n), ptr(out[0]), ptr(g), ptr(out[1]), ptr(out[2]), f(s.omb1), f(s.b2), f(s.omb2), f(s.eps), f(s.head), f(s.tail),
                        f(s.inv), C.c_int32(row_len), C.c_int32(split))
        if n == 0:
            continue
        ref, scl = R.adam_step64(p, g, m, v, lr, lr_tail, step, row_len, split, B1, B2, EPS)
        assert all(bool(torch.isfinite(t).all()) for t in out), (n, row_len, split, step)
        for k, r in _adam_ratios(out, ref, scl).items():
            assert r <= R.K[k], (k, r, n, row_len, split, step)
            top[k] = max(top[k], r)
        for i in R.adam_planted(n):                                    # g = m = v = 0: p keeps its bits
            assert R.bits_equal(out[0][i:i + 1], p[i:i + 1]), (n, i)
    print(f"adam_update on the host: worst ratios m' {top['adam_m']:.3f} u S_m, v' {top['adam_v']:.3f} u S_v, p' beyond u |p'|: {top['adam_p']:.3f} u U")


def _normalize_bwd32(q, g, mutate=None):
    """k_act_bwd's quaternion branch in float32 torch ops."""
    eps = torch.tensor(R.NORMALIZE_EPS, dtype=torch.float32)
    n = (q * q).sum(-1, keepdim=True).sqrt()
    inv = 1.0 / torch.maximum(n, eps)
    live = (n < eps) if mutate == "branch_inverted" else (n >= eps)
    k = torch.where(live, (q * g).sum(-1, keepdim=True) * inv * inv / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
    return g * inv - q * k


def test_correct_float32_activations_stay_inside_the_ceilings():
    top = dict.fromkeys(("act_fwd", "d_scaling", "d_opacity", "d_rotation", "d_rotation restated"), 0.0)
    for P in R.ACT_SIZES:
        (sc, ro, op), grads = R.activation_inputs(P, P)
        leaves = [t.clone().requires_grad_(True) for t in (sc, ro, op)]
        got = (torch.exp(leaves[0]), torch.nn.functional.normalize(leaves[1]), torch.sigmoid(leaves[2]))
        vals, scl = R.activations64(sc, ro, op)
        for a, b, s in zip(got, vals, scl):
            top["act_fwd"] = max(top["act_fwd"], R.worst(a, b, s))
        # backward on the float32 forward values, as the kernel reads them.  autograd's exp and sigmoid backward use the saved
        # outputs, so they are the kernel's expressions; its normalize backward goes through norm -> clamp -> div
        torch.autograd.backward(got, grads)
        d, dscl = R.activations_backward64(got[0], ro, got[2], *grads)
        for name, leaf, b, s in zip(("d_scaling", "d_rotation", "d_opacity"), leaves, d, dscl):
            top[name] = max(top[name], R.worst(leaf.grad, b, s))
        top["d_rotation restated"] = max(top["d_rotation restated"], R.worst(_normalize_bwd32(ro, grads[1]), d[1], dscl[1]))
    for name, r in top.items():
        print(f"{name}: worst ratio {r:.2f} u S")
        assert r <= R.CEIL[name.split()[0]], (name, r)


def test_correct_float32_densify_stats_stay_inside_the_ceiling():
    top = 0.0
    for P in R.DENSIFY_SIZES:
        radii, grad, mr, acc, den = R.densify_inputs(P, P)
        (mr1, acc1, den1), s = R.densify_stats64(radii, grad, mr, acc, den)
        vis = radii > 0
        m32, a32, d32 = mr.clone(), acc.clone(), den.clone()
        m32[vis] = torch.max(m32[vis], radii[vis].float())
        a32[vis] += (grad[vis, 0] * grad[vis, 0] + grad[vis, 1] * grad[vis, 1]).sqrt()[:, None]
        d32[vis] += 1
        assert torch.equal(m32.double(), mr1) and torch.equal(d32.double().reshape(-1), den1)
        top = max(top, R.worst(a32, acc1, s))
    print(f"xyz_gradient_accum: worst ratio {top:.2f} u S")
    assert top <= R.CEIL["densify_accum"]


# ---- the bounds have teeth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate", ("lr_swapped", "le_split", "step_off_by_one", "no_row_wrap"))
def test_a_planted_adam_defect_misses_the_bound_widely(mutate):
    row_len, split, step = 27, 3, 7
    n = R.adam_split_rows(row_len) * row_len
    p, g, m, v = R.adam_state(n, 5)
    ref, scl = R.adam_step64(p, g, m, v, LRS[0], LRS[1], step, row_len, split, B1, B2, EPS)
    good = _adam_ratios(_adam32(p, g, m, v, LRS[0], LRS[1], step, row_len, split), ref, scl)
    bad = _adam_ratios(_adam32(p, g, m, v, LRS[0], LRS[1], step, row_len, split, mutate), ref, scl)
    print(f"{mutate}: p' beyond u |p'| is {bad['adam_p']:.3g} u U (ceiling {R.CEIL['adam_p']}, unmutated {good['adam_p']:.2f})")
    assert good["adam_p"] <= R.CEIL["adam_p"]
    assert bad["adam_p"] >= 1000 * R.CEIL["adam_p"]


def test_an_inverted_normalize_branch_misses_the_bound_widely():
    (_, ro, _), grads = R.activation_inputs(1000, 1000)
    z = torch.zeros(1000, 1)
    d, scl = R.activations_backward64(torch.zeros(1000, 3), ro, z, torch.zeros(1000, 3), grads[1], z)
    good, bad = R.worst(_normalize_bwd32(ro, grads[1]), d[1], scl[1]), R.worst(_normalize_bwd32(ro, grads[1], "branch_inverted"), d[1], scl[1])
    print(f"branch_inverted: d_rotation {bad:.3g} u S (ceiling {R.CEIL['d_rotation']}, unmutated {good:.2f})")
    assert good <= R.CEIL["d_rotation"] and bad >= 1000 * R.CEIL["d_rotation"]


def test_asserted_bounds_do_not_exceed_their_ceilings():
    assert R.K.keys() == R.CEIL.keys()
    for name in R.K:
        assert 1 <= R.K[name] <= R.CEIL[name] and R.K[name] == int(R.K[name]), name


# ---- refusals that come before any launch (fake non-null pointers, no GPU) -----------------------------------------------------------
def test_training_entry_points_refuse_bad_arguments_without_gpu(native):
    lib = native.load()
    fake, odd, f = C.c_void_p(256), C.c_void_p(264), C.c_float
    err = lambda: lib.gsr_last_error()
    hyper = (f(0.9), f(0.999), f(1e-15))

    def adam(n=8, step=1, ptr=fake):
        return lib.gsr_adam_step(C.c_int64(n), ptr, fake, fake, fake, f(0.01), *hyper, C.c_int64(step), None)
    for step in (0, -1):
        assert adam(step=step) == -1 and b"gsr_adam_step: bad argument" in err()
    assert adam(ptr=None) == -1 and b"gsr_adam_step: bad argument" in err()
    assert adam(n=0) == 0 and adam(n=0, ptr=None) == 0

    def split(rows=4, row_len=4, split=1, step=1):
        return lib.gsr_adam_step_split(C.c_int64(rows), C.c_int32(row_len), C.c_int32(split), fake, fake, fake, fake, f(0.01), f(0.001), *hyper,
                                       C.c_int64(step), None)
    for kw in (dict(row_len=0), dict(row_len=3), dict(split=-1), dict(row_len=4, split=5), dict(step=0)):
        assert split(**kw) == -1 and b"gsr_adam_step_split: bad argument" in err(), kw
    assert split(rows=0) == 0

    def multi(count=1, n=30, row_len=0, split=0, step=1):
        t = (native.AdamTensor * max(count, 1))()
        for a in t:
            a.param = a.grad = a.exp_avg = a.exp_avg_sq = 256
            a.n, a.lr, a.lr_tail, a.step, a.row_len, a.split = n, 0.01, 0.01, step, row_len, split
        return lib.gsr_adam_step_multi(C.c_int32(count), t, *hyper, None)
    assert native.ADAM_MAX_TENSORS == 8
    assert multi(count=9) == -1 and b"0 .. 8 tensors" in err()
    for kw in (dict(n=30, row_len=4), dict(n=30, row_len=3), dict(step=0), dict(n=32, row_len=4, split=5)):
        assert multi(**kw) == -1 and b"bad tensor 0" in err(), kw
    assert multi(count=0) == 0 and multi(n=0) == 0

    def fwd(P=4, ins=(fake, fake, fake), outs=(fake, fake, fake)):
        return lib.gsr_activations_forward(C.c_int64(P), *ins, *outs, None)
    assert fwd(outs=(None, fake, fake)) == -1 and b"every input needs its output" in err()
    assert fwd(ins=(fake, None, fake)) == -1 and b"every input needs its output" in err()
    assert fwd(ins=(odd, fake, fake)) == -1 and b"16-byte aligned" in err()
    assert fwd(outs=(fake, fake, odd)) == -1 and b"16-byte aligned" in err()
    assert fwd(P=-1) == -1
    assert fwd(P=0) == 0 and fwd(P=0, ins=(None, fake, None), outs=(None, fake, None)) == 0

    def bwd(P=4, saved=(fake, fake, fake), gin=(fake, fake, fake), gout=(fake, fake, fake)):
        return lib.gsr_activations_backward(C.c_int64(P), *saved, *gin, *gout, None)
    assert bwd(saved=(None, fake, fake)) == -1 and b"a wanted gradient needs" in err()
    assert bwd(gin=(fake, None, fake)) == -1 and b"a wanted gradient needs" in err()
    assert bwd(gin=(fake, fake, odd)) == -1 and b"16-byte aligned" in err()
    assert bwd(gout=(odd, fake, fake)) == -1 and b"16-byte aligned" in err()
    assert bwd(P=-1) == -1
    assert bwd(P=0) == 0 and bwd(P=0, gin=(fake, None, fake), gout=(fake, None, fake)) == 0

    def densify(P=4, radii=fake, out=fake):
        return lib.gsr_densify_stats(C.c_int32(P), radii, fake, out, fake, fake, None)
    assert densify(radii=None) == -1 and b"gsr_densify_stats: bad argument" in err()
    assert densify(out=None) == -1 and b"gsr_densify_stats: bad argument" in err()
    assert densify(P=-1) == -1 and b"gsr_densify_stats: bad argument" in err()
    assert densify(P=0, radii=None) == 0

    size = C.c_size_t(0)
    assert lib.gsr_dist2_workspace_size(C.c_int32(-1), C.byref(size)) == -1 and b"gsr_dist2_workspace_size: bad argument" in err()
    assert lib.gsr_dist2_workspace_size(C.c_int32(10), None) == -1 and b"gsr_dist2_workspace_size: bad argument" in err()
    assert lib.gsr_dist2_workspace_size(C.c_int32(10), C.byref(size)) == 0 and size.value > 0
    assert lib.gsr_dist2_knn3(C.c_int32(-1), fake, fake, fake, None) == -1 and b"gsr_dist2_knn3: bad argument" in err()
    for args in ((None, fake, fake), (fake, None, fake), (fake, fake, None)):
        assert lib.gsr_dist2_knn3(C.c_int32(10), *args, None) == -1 and b"gsr_dist2_knn3: bad argument" in err()
    assert lib.gsr_dist2_knn3(C.c_int32(0), None, None, None, None) == 0
