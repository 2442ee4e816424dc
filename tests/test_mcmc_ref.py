"""CPU checks of the MCMC densification strategy: the C ABI is additive (five new symbols declared and exported, the version
unchanged) and refuses bad arguments without touching a GPU; the binary64 restatement (tests/mcmc_ref.py) holds its closed forms and
stays within 1e-12 of a 50-digit evaluation; the kernels' own per-Gaussian functions (csrc/gsr_math.h mcmc_relocation_one,
mcmc_noise_one, mcmc_reg_one, compiled with g++: tests/mcmc_host.cpp) and the package's torch path agree with the restatement under
its error rules; the model's relocate / grow on the host path leave behind what tests/mcmc_checks.py states; training_setup refuses
what the strategy does not support."""
import ctypes as C
import math
import os
import re
import subprocess
from dataclasses import replace
from decimal import Decimal, getcontext

import numpy as np
import pytest
import torch

import mcmc_checks as MC
import mcmc_ref as MR
from diff_gaussian_rasterization import mcmc
from scene import GaussianModel, OptimizationDefaults

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ("gsr_mcmc_relocation_workspace_size", "gsr_mcmc_relocation", "gsr_mcmc_relocate_rows", "gsr_mcmc_inject_noise",
                 "gsr_mcmc_reg_grads")
RATIOS = (1, 2, 5, 20, 51, 60)


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_functions_are_declared_and_exported_and_the_version_stays(native):
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"^\s*(?:int|const char \*)\s*\**(gsr_[a-z0-9_]+)\s*\(", hdr, re.M))
    lib = native.load()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported by libgsrast.so"
        assert name in native.EXPORTS
    assert lib.gsr_version() == 12 and "#define GSR_VERSION 12" in hdr
    consts = open(os.path.join(ROOT, "include", "gsr_constants.h")).read()
    assert int(re.search(r"#define\s+GSR_MCMC_MAX_RATIO\s+(\d+)", consts).group(1)) == MR.MAX_RATIO == mcmc.MAX_RATIO == 51
    assert native.MCMC_MAX_TENSORS == int(re.search(r"#define\s+GSR_MCMC_MAX_TENSORS\s+(\d+)", hdr).group(1))
    for role, value in native.MCMC_ROLES.items():
        assert int(re.search(rf"#define\s+GSR_MCMC_ROLE_{role.upper()}\s+(\d+)", hdr).group(1)) == value


def test_argument_validation_without_gpu(native):
    """Every refusal comes before anything touches the device: the pointers here are never dereferenced."""
    lib = native.load()
    f = C.c_void_p(256)
    size = C.c_size_t(0)
    assert lib.gsr_mcmc_relocation_workspace_size(C.c_int64(1000), C.byref(size)) == 0 and size.value >= 4000
    assert lib.gsr_mcmc_relocation_workspace_size(C.c_int64(-1), C.byref(size)) == -1
    assert lib.gsr_mcmc_relocation_workspace_size(C.c_int64(10), None) == -1

    def reloc(P=10, n=4, op=f, sc=f, sampled=f, min_opacity=0.005, ws=f, out_o=f, out_s=f):
        rc = lib.gsr_mcmc_relocation(C.c_int64(P), C.c_int64(n), op, sc, sampled, C.c_float(min_opacity), ws, out_o, out_s, None)
        return rc, lib.gsr_last_error()
    for kw in (dict(P=-1), dict(n=-2)):
        rc, msg = reloc(**kw)
        assert rc == -1 and b"gsr_mcmc_relocation" in msg
    for m in (0.0, 1.0, -0.1, 1.5, float("nan")):
        rc, msg = reloc(min_opacity=m)
        assert rc == -1 and b"min_opacity" in msg
    for name in ("op", "sc", "sampled", "ws", "out_o", "out_s"):
        rc, msg = reloc(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
    assert reloc(P=0)[0] == 0 and reloc(n=0, sampled=None, out_o=None, out_s=None)[0] == 0

    def rows(count=1, width=3, role=0, m=256, v=256, param=256, P=10, n=4, sampled=f, dead=f, new_o=f, new_s=f):
        t = (native.McmcTensor * 1)()
        t[0].param, t[0].exp_avg, t[0].exp_avg_sq, t[0].width, t[0].role = param, m, v, width, role
        rc = lib.gsr_mcmc_relocate_rows(C.c_int32(count), t, C.c_int64(P), C.c_int64(n), sampled, dead, new_o, new_s, None)
        return rc, lib.gsr_last_error()
    rc, msg = rows(width=0)
    assert rc == -1 and b"width >= 1" in msg
    rc, msg = rows(role=3)
    assert rc == -1 and b"role" in msg
    rc, msg = rows(role=1, width=3)
    assert rc == -1 and b"does not fit its role" in msg
    rc, msg = rows(role=2, width=1)
    assert rc == -1 and b"does not fit its role" in msg
    rc, msg = rows(m=256, v=None)
    assert rc == -1 and b"both" in msg
    rc, msg = rows(param=None)
    assert rc == -1 and b"param is NULL" in msg
    rc, msg = rows(count=native.MCMC_MAX_TENSORS + 1)
    assert rc == -1 and b"tensors" in msg
    for kw in (dict(P=-1), dict(n=-1)):
        assert rows(**kw)[0] == -1
    for name in ("sampled", "new_o", "new_s"):
        rc, msg = rows(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
    assert rows(count=0)[0] == 0 and rows(n=0)[0] == 0 and rows(P=0)[0] == 0

    def noise(P=10, xyz=f, sc=f, rot=f, op=f, xi=f):
        rc = lib.gsr_mcmc_inject_noise(C.c_int64(P), xyz, sc, rot, op, xi, C.c_float(1.0), None)
        return rc, lib.gsr_last_error()
    assert noise(P=-1)[0] == -1
    for name in ("xyz", "sc", "rot", "op", "xi"):
        rc, msg = noise(**{name: None})
        assert rc == -1 and b"NULL" in msg, name
        rc, msg = noise(**{name: C.c_void_p(260)})
        assert rc == -1 and b"16-byte aligned" in msg, name
    assert noise(P=0, xyz=None)[0] == 0

    def reg(P=10, op=f, sc=f, go=f, gs=f):
        rc = lib.gsr_mcmc_reg_grads(C.c_int64(P), op, sc, C.c_float(0.01), C.c_float(0.01), go, gs, None)
        return rc, lib.gsr_last_error()
    assert reg(P=-1)[0] == -1
    rc, msg = reg(op=None)
    assert rc == -1 and b"needs its raw tensor" in msg
    rc, msg = reg(sc=None)
    assert rc == -1 and b"needs its raw tensor" in msg
    rc, msg = reg(gs=C.c_void_p(260))
    assert rc == -1 and b"16-byte aligned" in msg
    assert reg(P=0)[0] == 0 and reg(go=None, gs=None)[0] == 0


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_restatement_closed_forms():
    x, ls = MR.relocation_inputs(400, 1)
    x64, ls64 = x.astype(np.float64).reshape(-1), ls.astype(np.float64)
    # N = 1 returns its inputs exactly
    o1, s1 = MR.relocation(x, ls, 1, 0.005)
    assert np.array_equal(o1, x64) and np.array_equal(s1, ls64)
    # N = 2: D = 2 o' - o'^2 / sqrt 2
    o, om = MR.sigmoid(x64), MR.sigmoid(-x64)
    op = MR.relocated_opacity(om, 2)
    assert np.allclose(MR.denominator(op, 2), 2 * op - op * op / math.sqrt(2), rtol=1e-15, atol=0)
    _, s2 = MR.relocation(x, ls, 2, 0.005)
    assert np.abs(s2 - (ls64 + np.log(o / (2 * op - op * op / math.sqrt(2)))[:, None])).max() <= 1e-13
    # 1 - (1 - o')^N = o
    for N in RATIOS[1:-1]:
        op = MR.relocated_opacity(om, N)
        assert np.abs(1 - (1 - op) ** N - o).max() <= 1e-12, N
        # the opacity output is logit(o') where nothing clamps
        out_o, _ = MR.relocation(x, ls, N, 0.005)
        free = (op > 0.0051) & (op < 0.999)
        assert free.sum() > 100 and np.abs(MR.sigmoid(out_o[free]) - op[free]).max() <= 1e-14
        assert (MR.sigmoid(out_o) >= float(np.float32(0.005)) * (1 - 1e-12)).all()
    # N > 51 equals N = 51
    a, b = MR.relocation(x, ls, 60, 0.005), MR.relocation(x, ls, 51, 0.005)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # g(0.005) = 1/2, and the gate saturates on both sides
    assert MR.gate(0.005) == 0.5 and MR.gate(0.0) > 0.62 and MR.gate(1.0) < 1e-43
    assert np.array_equal(MR.multiplicity([3, 3, 5, 3, 0], 6), [4, 4, 2, 4, 2])


def test_binary64_is_enough_and_binary32_is_not():
    """The alternating sum against a 50-digit evaluation: binary64 stays within 1e-12 for o in [0.005, 0.99999] and N up to 51; the
    same sum in binary32 does not stay within 1e-6 (why the kernel runs the rule in binary64)."""
    getcontext().prec = 50
    worst64 = worst32 = 0.0
    for N in (2, 5, 20, 51):
        for o in (0.005, 0.05, 0.3, 0.7, 0.95, 0.999, 0.99999):
            op = float(MR.relocated_opacity(np.float64(1.0 - o), N))
            d, exact = Decimal(op), Decimal(0)
            for j in range(1, N + 1):
                exact += (-1) ** (j - 1) * math.comb(N, j) * d ** j / Decimal(j).sqrt()
            worst64 = max(worst64, abs(float((Decimal(float(MR.denominator(op, N))) - exact) / exact)))
            D32, c, pw = np.float32(0), np.float32(1), np.float32(1)
            for j in range(1, N + 1):
                c = np.float32(c * np.float32(N - j + 1) / np.float32(j))
                pw = np.float32(pw * np.float32(op))
                t = np.float32(c * pw / np.sqrt(np.float32(j)))
                D32 = np.float32(D32 + t) if j & 1 else np.float32(D32 - t)
            worst32 = max(worst32, abs(float((Decimal(float(D32)) - exact) / exact)))
    print(f"relative error of D: binary64 {worst64:.3e}, binary32 {worst32:.3e}")
    assert worst64 <= 1e-12 and worst32 > 1e-6


# ---- the kernels' per-Gaussian functions on the host ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mcmc_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("mcmc")
    exe = str(d / "mcmc_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "mcmc_host.cpp")])

    def run(kind, rows, width):
        rows = np.asarray(rows, np.float64)
        with open(d / "in.txt", "w") as fh:
            for r in rows:
                fh.write(f"{kind} " + " ".join(f"{np.float32(v):.9g}" for v in r) + "\n")
        subprocess.check_call([exe, str(d / "in.txt"), str(d / "out.txt")])
        out = np.loadtxt(d / "out.txt", dtype=np.float32, ndmin=2)
        assert out.shape == (rows.shape[0], width)
        return out
    return run


def test_host_relocation_against_the_restatement(mcmc_host):
    x, ls = MR.relocation_inputs(600, 2)
    N = np.resize(np.array(RATIOS), 600)
    out = mcmc_host(0, np.concatenate((x, ls, N[:, None], np.full((600, 1), 0.005)), 1), 4)
    ref_o, ref_s = MR.relocation(x, ls, N, 0.005)
    worst = MR.check_relocation(out[:, 0], out[:, 1:], ref_o, ref_s, "host relocation")
    print(f"host relocation: worst error {worst:.3f} x the bound")
    one = N == 1
    assert np.array_equal(out[one, 0], x[one, 0]) and np.array_equal(out[one, 1:], ls[one])      # the identity, bit for bit


@pytest.mark.parametrize("c", (1e-3, 80.0))
def test_host_noise_against_the_restatement(mcmc_host, c):
    xyz, ls, q, x, xi = MR.noise_inputs(1000, 3)
    delta = mcmc_host(1, np.concatenate((ls, q, x, xi, np.full((1000, 1), c)), 1), 3)
    assert np.isfinite(delta).all()
    worst = MR.check_noise(xyz + delta, xyz, ls, q, x, xi, c, f"host noise c={c}")
    print(f"host noise c={c}: worst error {worst:.3f} x the bound")
    saturated = x.reshape(-1) >= 3.0                               # o >= 0.95: exp(100 o - 0.5) overflows binary32, g = 0
    assert saturated.sum() > 100 and not delta[saturated].any()
    live = np.abs(x.reshape(-1) - math.log(0.005 / 0.995)) <= 1.0
    assert live.sum() >= 250 and (np.abs(delta[live]).max(1) > 0).mean() > 0.99


def test_host_reg_against_the_restatement(mcmc_host):
    _, ls, _, x, _ = MR.noise_inputs(1000, 4)
    k_o, k_s = 0.01 / 1000, 0.01 / 3000
    out = mcmc_host(2, np.concatenate((x, ls, np.full((1000, 1), k_o), np.full((1000, 1), k_s)), 1), 4)
    # the twin takes the two factors as binary32: the restatement is evaluated with those
    ref_o, ref_s = MR.reg_delta(x, ls, float(np.float32(k_o)) * 1000, float(np.float32(k_s)) * 3000)
    zero = np.zeros(1000)
    w = max(MR.check_reg(out[:, 0], ref_o, zero, "host reg opacity"), MR.check_reg(out[:, 1:], ref_s, np.zeros(3000), "host reg scaling"))
    print(f"host reg: worst error {w:.3f} x the bound")


# ---- the package's torch path -------------------------------------------------------------------------------------------------------
def test_torch_relocation_against_the_restatement():
    x, ls = MR.relocation_inputs(700, 5)
    rng = np.random.default_rng(5)
    sampled = np.concatenate((rng.integers(0, 700, 300), np.full(60, 17), np.full(2, 33), [44]))
    t = lambda a, dt=torch.float32: torch.as_tensor(np.asarray(a), dtype=dt)
    out_o, out_s = mcmc.compute_relocation(t(x), t(ls), t(sampled, torch.int64), 0.005, native=False)
    assert out_o.dtype == out_s.dtype == torch.float32 and out_o.shape == (363,) and out_s.shape == (363, 3)
    N = MR.multiplicity(sampled, 700)
    assert N.max() >= 61 and (N == 2).any()
    ref_o, ref_s = MR.relocation(x[sampled], ls[sampled], N, 0.005)
    MR.check_relocation(out_o.numpy(), out_s.numpy(), ref_o, ref_s, "torch relocation")
    a, b = mcmc.compute_relocation(t(x), t(ls), t(sampled, torch.int64), 0.005)           # host tensors: native=None takes the same path
    assert torch.equal(a, out_o) and torch.equal(b, out_s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        mcmc.compute_relocation(t(x), t(ls), t(sampled, torch.int64), 0.005, native=True)
    with pytest.raises(ValueError, match="min_opacity"):
        mcmc.compute_relocation(t(x), t(ls), t(sampled, torch.int64), 1.0)
    with pytest.raises(TypeError, match="int64"):
        mcmc.compute_relocation(t(x), t(ls), t(sampled, torch.int32), 0.005)


@pytest.mark.parametrize("c", (1e-3, 80.0))
def test_torch_noise_and_reg_against_the_restatement(c):
    xyz, ls, q, x, xi = MR.noise_inputs(1000, 6)
    t = torch.from_numpy
    out = t(xyz.copy()).requires_grad_(True)
    v0 = out._version
    mcmc.inject_position_noise(out, t(ls), t(q), t(x), t(xi), c)
    assert out._version > v0
    MR.check_noise(out.detach().numpy(), xyz, ls, q, x, xi, c, f"torch noise c={c}")
    saturated = x.reshape(-1) >= 3.0
    assert np.array_equal(out.detach().numpy()[saturated], xyz[saturated])
    rng = np.random.default_rng(6)
    g_o, g_s = rng.standard_normal((1000, 1)).astype(np.float32) * 1e-5, rng.standard_normal((1000, 3)).astype(np.float32) * 1e-5
    go, gs = t(g_o.copy()), t(g_s.copy())
    mcmc.add_regularizer_grads(t(x), t(ls), 0.01, 0.02, go, gs)
    ref_o, ref_s = MR.reg_delta(x, ls, 0.01, 0.02)
    MR.check_reg(go.numpy().astype(np.float64) - g_o, ref_o, g_o, "torch reg opacity")
    MR.check_reg(gs.numpy().astype(np.float64) - g_s, ref_s, g_s, "torch reg scaling")
    only = t(g_s.copy())
    mcmc.add_regularizer_grads(None, t(ls), 0.01, 0.02, None, only)                       # a None side is left alone
    assert torch.equal(only, gs)


# ---- the model's host path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", (3, 0))
def test_model_relocate_on_the_host_path(D):
    gm = MC.make_model(500, D, "cpu")
    assert gm._features.shape == (500, (D + 1) ** 2, 3)
    gen = torch.Generator().manual_seed(5)
    dead = list(range(3, 500, 7))
    sampled, N, worst, _ = MC.check_relocate(gm, dead, generator=gen, native=False)
    assert N.max() >= 3                                            # 71 draws from 429: some source is taken twice or more
    print(f"model relocate D={D}: worst error {worst:.3f} x the bound, multiplicities up to {N.max()}")
    # nothing happens when no row is dead
    old, mom = MC.snapshot(gm)
    assert gm.mcmc_relocate(MC.MIN_OPACITY, generator=gen) == 0
    new, mom2 = MC.snapshot(gm)
    for k in old:
        assert torch.equal(old[k], new[k]) and all(torch.equal(a, b) for a, b in zip(mom[k], mom2[k]))


@pytest.mark.parametrize("D", (3, 0))
def test_model_relocate_all_dead_but_one(D):
    MC.all_but_one(MC.make_model(500, D, "cpu"), 123, generator=torch.Generator().manual_seed(6), native=False)


def test_model_relocate_without_optimizer_moves_parameters_only():
    import scene_synth as S
    gm = GaussianModel(1)
    gm.adopt_scene(S.make_scene(200, 64, 64, 1, 7), device="cpu")
    MC.kill(gm, [1, 2, 3])
    n_dead = int((torch.sigmoid(gm._opacity.detach()) <= 0.005).sum())
    assert gm.mcmc_relocate(0.005, generator=torch.Generator().manual_seed(1)) == n_dead >= 3
    assert float(torch.sigmoid(gm._opacity.detach()).min()) >= 0.005 * (1 - 1e-6)
    fresh = MC.make_model(200, 1, "cpu", steps=0)                  # an optimizer that has not stepped: no moments yet
    MC.kill(fresh, [5])
    assert fresh.mcmc_relocate(0.005) >= 1


@pytest.mark.parametrize("D", (3, 0))
def test_model_grow_on_the_host_path(D):
    gm = MC.make_model(500, D, "cpu")
    gen = torch.Generator().manual_seed(8)
    counts = [500]
    assert MC.check_grow(gm, 600, generator=gen, native=False) == 25
    counts.append(gm._xyz.shape[0])
    MC.check_capture_restore(gm)
    for _ in range(4):
        MC.check_grow(gm, 600, generator=gen, native=False, detailed=False)
        counts.append(gm._xyz.shape[0])
    assert counts == [500, 525, 551, 578, 600, 600]
    for k, t in gm._t.items():
        st = gm.optimizer.state[t]
        assert t.shape[0] == st["exp_avg"].shape[0] == st["exp_avg_sq"].shape[0] == 600 and torch.isfinite(t).all(), k
    gm._t["xyz"].grad = torch.zeros_like(gm._xyz)                 # the optimizer still steps the grown table
    gm.optimizer.step()
    MC.check_capture_restore(gm)


def test_model_noise_and_regularizer_on_the_host_path():
    gm = MC.make_model(300, 2, "cpu")
    xyz0, v0 = gm._xyz.detach().clone(), gm._xyz._version
    noise = torch.randn(300, 3, generator=torch.Generator().manual_seed(2))
    gm.mcmc_inject_noise(80.0, noise=noise)
    assert gm._xyz._version > v0
    n = lambda t: t.detach().numpy()
    MR.check_noise(n(gm._xyz), n(xyz0), n(gm._scaling), n(gm._rotation), n(gm._opacity), n(noise), 80.0, "model noise")
    torch.manual_seed(0)
    gm.mcmc_inject_noise(1.0)                                      # noise = None draws its own
    assert torch.isfinite(gm._xyz).all()
    assert gm._opacity.grad is None and gm._scaling.grad is None
    gm.mcmc_add_regularizer_grads(0.01, 0.02)                      # a missing .grad starts as zeros
    ref_o, ref_s = MR.reg_delta(n(gm._opacity), n(gm._scaling), 0.01, 0.02)
    MR.check_reg(n(gm._opacity.grad), ref_o, np.zeros(300), "model reg opacity")
    MR.check_reg(n(gm._scaling.grad), ref_s, np.zeros(900), "model reg scaling")
    g0 = gm._opacity.grad.clone()
    gm.mcmc_add_regularizer_grads(0.01, 0.02)                      # ... and an existing one is added to
    MR.check_reg(n(gm._opacity.grad).astype(np.float64) - n(g0), ref_o, n(g0), "model reg opacity, second call")


def test_multinomial_limit_is_reported():
    gm = GaussianModel(0)
    gm.MULTINOMIAL_MAX = 100                                       # the limit itself (2^24 rows) is too large for a test
    import scene_synth as S
    gm.adopt_scene(S.make_scene(200, 64, 64, 0, 7), device="cpu")
    assert GaussianModel.MULTINOMIAL_MAX == 2 ** 24
    with pytest.raises(ValueError, match=r"2\^24"):
        gm.mcmc_grow(1000, 0.005)


def test_defaults_and_refusals_of_training_setup():
    d = OptimizationDefaults()
    assert (d.densify_strategy, d.mcmc_cap_max, d.mcmc_noise_lr, d.mcmc_min_opacity, d.mcmc_opacity_reg, d.mcmc_scale_reg) == \
        ("default", 1_000_000, 5e5, 0.005, 0.01, 0.01)
    import scene_synth as S
    gm = GaussianModel(0)
    gm.adopt_scene(S.make_scene(50, 64, 64, 0, 7), device="cpu")
    with pytest.raises(ValueError, match="densify_strategy"):
        gm.training_setup(replace(d, densify_strategy="MCMC"))
    with pytest.raises(ValueError, match="densify_absgrad"):
        gm.training_setup(replace(d, densify_strategy="mcmc", densify_absgrad=True))
    gm.training_setup(replace(d, densify_absgrad=True))
    assert gm.densify_strategy == "default"
    gm.training_setup(replace(d, densify_strategy="mcmc"))
    assert gm.densify_strategy == "mcmc"
