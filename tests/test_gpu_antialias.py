"""The anti-aliasing switch (GaussianRasterizer(..., antialiasing=True)) on the GPU.

1. The op alone (diff_gaussian_rasterization.antialias.compensate_opacity, the HIP kernels of csrc/gsr_antialias.hip) against the
   binary64 restatement (tests/antialias_ref.py) under its error rule: x = rho^2, the compensated opacity and every gradient within
   4 x the worst error of the restatement evaluated in binary32 on the same inputs, plus 2^-23 of the tensor's largest magnitude.
   Activated and raw inputs; the same inputs give the same bits.
2. Whole frames: pixels against oracle.rasterize(float64) fed opacities * rho64 at the suite's 1e-5 on strict pixels; gradients of a
   dL/dcolor masked to strict pixels against the oracle's backward, its dL/dopacity' chained through the restatement's autograd and
   added to the oracle's means3D / scales / rotations gradients, every Gaussian at the suite's 1e-4 (_check_grads).
3. Off is off: antialiasing=False is bit-equal to a rasterizer built without the keyword and launches no aa_* kernel; on, exactly
   one aa_fwd and one aa_bwd per step.
4. Through render() with pipe.antialiasing: the raw path and the getter path agree, the alpha map is 1 - T_final of the compensated
   frame, every parameter of LatentGaussianModel receives a gradient.

Measured on an MI355X (worst error / worst error of the binary32 restatement, over the six scenes): see DESIGN.md section 12."""
import numpy as np
import pytest
import torch

import antialias_ref as AR
import oracle
import scene_synth as S
from test_gpu_parity import DEV, FRAGILE_CAP, _check_forward, _check_grads, _inputs, _settings, _strict_pixels
from util import raster_kwargs

pytestmark = pytest.mark.gpu

CASES = ("p2048", "p2048_small", "p64", "posed", "mod0.5", "xclamp")
F64 = torch.float64


@pytest.fixture(scope="module")
def refs():
    """Per scene, computed once and left unchanged: the raster kwargs, the binary64 rule on the activated inputs and the oracle's
    binary64 frame of the COMPENSATED opacities."""
    out = {}
    for name, (scene, cam, mod) in AR.scene_cases().items():
        kw = raster_kwargs(scene, cam, scale_modifier=mod)
        c = AR.camera_of(kw)
        r64 = AR.rule(*AR.case_inputs(scene, False), c)
        kw_c = dict(kw, opacities=np.asarray(kw["opacities"], np.float64) * r64["rho"].numpy()[:, None])
        fr64 = oracle.rasterize(dtype=np.float64, **kw_c)
        out[name] = dict(scene=scene, cam=cam, kw=kw, c=c, r64=r64, fr64=fr64, kw_c=kw_c)
    return out


def test_the_scenes_exercise_the_feature(refs):
    """Asserted on the binary64 side, among the Gaussians the oracle renders (radius > 0): the tests below cannot pass on scenes
    where the feature is idle."""
    vis = lambda n: torch.as_tensor(refs[n]["fr64"].radii > 0)
    r, v = refs["p2048"]["r64"], vis("p2048")
    assert int((r["clamped"] & v).sum()) == 0
    assert float((r["rho"][v] < 0.5).double().mean()) >= 0.10 and float((r["rho"][v] > 0.5).double().mean()) >= 0.10
    q = np.quantile(r["rho"][v].numpy(), [0.05, 0.5, 0.95])
    print(f"p2048: rho among {int(v.sum())} visible Gaussians: 5 % {q[0]:.3f}, median {q[1]:.3f}, 95 % {q[2]:.3f}")
    assert int(refs["p2048_small"]["r64"]["clamped"].sum()) >= 50
    assert int((refs["xclamp"]["r64"]["xmul0"] & vis("xclamp")).sum()) >= 16
    assert int(refs["posed"]["r64"]["through"].sum()) > 0 and np.abs(refs["posed"]["c"]["V"][:3, :3]).min() > 0.1


# ---- 1. the op alone ----------------------------------------------------------------------------------------------------------------
def _run_op(inputs, rs, g, raw):
    from diff_gaussian_rasterization.antialias import compensate_opacity
    leaves = [t.to(DEV).requires_grad_(True) for t in inputs]
    out = compensate_opacity(*leaves, rs, raw=raw)
    grads = torch.autograd.grad(out, leaves, g.to(DEV).reshape(out.shape))
    torch.cuda.synchronize()
    return out.detach(), grads


@pytest.mark.parametrize("raw", [False, True], ids=["activated", "raw"])
@pytest.mark.parametrize("case", CASES)
def test_op_against_the_restatement(refs, case, raw):
    ref = refs[case]
    rs = _settings(ref["kw"])
    inputs = AR.case_inputs(ref["scene"], raw)
    g = AR.upstream(ref["scene"].P, 11).to(torch.float32)
    out, grads = _run_op(inputs, rs, g, raw)
    assert out.is_cuda and out.shape == inputs[0].shape
    AR.check_against_ref(inputs, ref["c"], g, out.cpu(), {n: t.cpu() for n, t in zip(AR.GRAD_NAMES, grads)}, raw=raw,
                         what=f"gpu {case} {'raw' if raw else 'act'}")
    zero = (g == 0).to(DEV)
    assert zero.any() and all(not t[zero].any() for t in grads)          # rows without an incoming gradient: exact zeros
    out2, grads2 = _run_op(inputs, rs, g, raw)                           # the same inputs give the same bits
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_unwanted_gradients_and_no_grad(refs):
    from diff_gaussian_rasterization.antialias import compensate_opacity
    ref = refs["p64"]
    rs = _settings(ref["kw"])
    inputs = [t.to(DEV) for t in AR.case_inputs(ref["scene"], False)]
    g = AR.upstream(ref["scene"].P, 12).to(torch.float32).to(DEV)
    full = [t.clone().requires_grad_(True) for t in inputs]
    want = torch.autograd.grad(compensate_opacity(*full, rs), full, g.reshape(-1, 1))
    for keep in (0, 2):                                                  # only the opacities, only the scales
        leaves = [t.clone().requires_grad_(i == keep) for i, t in enumerate(inputs)]
        got, = torch.autograd.grad(compensate_opacity(*leaves, rs), [leaves[keep]], g.reshape(-1, 1))
        assert torch.equal(got, want[keep])
    with torch.no_grad():
        assert not compensate_opacity(*full, rs).requires_grad
    empty = [t[:0] for t in inputs]
    assert compensate_opacity(*empty, rs).shape == (0, 1)


# ---- 2. whole frames ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_frames_against_the_oracle(refs, case):
    from diff_gaussian_rasterization import GaussianRasterizer
    ref = refs[case]
    kw, fr64, scene = ref["kw"], ref["fr64"], ref["scene"]
    H, W = kw["image_height"], kw["image_width"]
    inp = _inputs(kw)
    means2D = torch.zeros(scene.P, 3, device=DEV, requires_grad=True)
    color, radii = GaussianRasterizer(_settings(kw), antialiasing=True)(means2D=means2D, **inp)
    _check_forward(ref["kw_c"], fr64, color.detach().cpu().numpy(), radii.cpu().numpy(), frag_cap=FRAGILE_CAP)
    strict = _strict_pixels(fr64, radii.cpu().numpy())
    gm = np.where(strict[None], S.make_grad_image(W, H, 23).numpy(), 0.0)
    color.backward(torch.as_tensor(gm, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    got = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    got["means2D"] = means2D.grad.detach().cpu().numpy()
    # the oracle's backward stops at the compensated opacity; the restatement's autograd takes dL/dopacity' the rest of the way
    want = fr64.backward(gm.astype(np.float64))
    _, chain = AR.evaluate(AR.case_inputs(scene, False), ref["c"], want["opacities"].reshape(-1))
    total = dict(want)
    total["opacities"] = chain["opacities"].numpy()
    for n in ("means3D", "scales", "rotations"):
        total[n] = want[n].reshape(chain[n].shape) + chain[n].numpy()
    live, strict_live = _check_grads(fr64, total, got, ["means3D", "means2D", "opacities", "shs", "scales", "rotations"], masked=True)
    assert live > 20 and strict_live == live
    moved = np.abs(chain["scales"].numpy()).max() / max(np.abs(want["scales"]).max(), 1e-30)
    print(f"{case}: {live} Gaussians with a gradient; the compensation's share of the scales gradient: {moved:.2f} of the oracle's largest")
    assert moved > 1e-2                                                  # the chained term is not lost in the tolerance


# ---- 3. off is off, on is one launch each way -----------------------------------------------------------------------------------------
def _step(kw, **ctor):
    from diff_gaussian_rasterization import GaussianRasterizer
    inp = _inputs(kw)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=True)
    color, radii = GaussianRasterizer(_settings(kw), **ctor)(means2D=means2D, **inp)
    color.backward(S.make_grad_image(kw["image_width"], kw["image_height"], 5).to(DEV))
    torch.cuda.synchronize()
    return color.detach(), radii, {k: v.grad for k, v in inp.items()}, means2D.grad


def test_switch_off_is_the_plain_rasterizer_bit_for_bit(refs):
    from diff_gaussian_rasterization import _native as N
    kw = refs["p2048"]["kw"]
    plain = _step(kw)
    N.profile_enable(True)
    off = _step(kw, antialiasing=False)
    prof_off = N.profile_read(128)
    N.profile_enable(True)
    on = _step(kw, antialiasing=True)
    prof_on = N.profile_read(128)
    N.profile_enable(False)
    assert torch.equal(plain[0], off[0]) and torch.equal(plain[1], off[1]) and torch.equal(plain[3], off[3])
    for k in plain[2]:
        assert torch.equal(plain[2][k], off[2][k]), k
    assert not [k for k in prof_off if k.startswith("aa_")], prof_off
    assert prof_on["aa_fwd"][1] == 1 and prof_on["aa_bwd"][1] == 1, prof_on
    assert torch.equal(plain[1], on[1]) and not torch.equal(plain[0], on[0])          # the same radii, another image


# ---- 4. through render() ------------------------------------------------------------------------------------------------------------
def _aa_pipe(**kv):
    from gaussian_params import Pipe
    pipe = Pipe()
    pipe.antialiasing = True
    for k, v in kv.items():
        setattr(pipe, k, v)
    return pipe


def test_render_raw_path_and_getter_path_agree():
    """scene.GaussianModel renders from its raw leaves (raw mode 2, the compensation on logits); fused_activations=False goes through
    the getters (the compensation on activated values).  The tolerance of test_gpu_parity's raw-mode-against-getters test."""
    from gaussian_renderer import render
    from scene import GaussianModel
    W, H, D = 320, 208, 3
    # zmin = 2: without the near splats that saturate every pixel, the compensation changes the image (asserted below)
    scene, cam = S.make_scene(20_000, W, H, D, 20, scale_lo=0.003, scale_hi=0.06, zmin=2.0), S.make_camera(W, H).to(DEV)
    bg = torch.tensor([0.1, 0.0, 0.2], device=DEV)
    gimg = S.make_grad_image(W, H, 6).to(DEV)
    results = []
    for fused in (False, None):
        gm = GaussianModel(D)
        gm.adopt_scene(scene, device=DEV)
        out = render(cam, gm, _aa_pipe(fused_activations=fused), bg)
        out["render"].backward(gimg)
        torch.cuda.synchronize()
        grads = {n: getattr(gm, n).grad.detach().clone() for n in ("_xyz", "_features", "_opacity", "_scaling", "_rotation")}
        results.append((out["render"].detach(), out["radii"], out["viewspace_points"].grad.detach().clone(), grads))
    (img_a, rad_a, vp_a, g_a), (img_b, rad_b, vp_b, g_b) = results
    assert int((rad_a != rad_b).sum()) <= 2
    derr = (img_a - img_b).abs().amax(0)
    assert float((derr > 2e-5).float().mean()) <= 1e-4 and float(derr.max()) <= 8e-3
    for n in g_a:
        a, b = g_a[n].reshape(g_a[n].shape[0], -1), g_b[n].reshape(g_b[n].shape[0], -1)
        scale = float(a.abs().max())
        assert scale > 0, n
        bad_rows = ((a - b).abs() > 2e-5 * scale + 2e-3 * a.abs()).any(1)
        assert float(bad_rows.float().mean()) <= 2e-4, f"{n}: {int(bad_rows.sum())} rows differ"
        assert float((a - b).norm() / a.norm()) <= 1e-4, n
    assert float((vp_a - vp_b).norm() / vp_a.norm()) <= 1e-4
    # and the switch did something: the plain frame is another image
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    from gaussian_params import Pipe
    with torch.no_grad():
        plain = render(cam, gm, Pipe(), bg)["render"]
    assert float((plain - img_b).abs().max()) > 0.05


def test_render_alpha_map_is_that_of_the_compensated_frame():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    from diff_gaussian_rasterization.antialias import compensate_opacity
    from gaussian_renderer import render
    from scene import GaussianModel
    W, H, D = 128, 128, 3
    scene, cam = S.make_scene(2048, W, H, D, 105), S.make_camera(W, H).to(DEV)
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    with torch.no_grad():
        out = render(cam, gm, _aa_pipe(), torch.zeros(3, device=DEV), depth_alpha=True)
        kw = raster_kwargs(scene, cam.to("cpu"))
        rs = _settings(kw)
        logits = compensate_opacity(gm._opacity, gm._xyz, gm._scaling, gm._rotation, rs, raw=True)
        color, radii, fr = dgr.rasterize_forward(gm._xyz, gm._features, None, logits, gm._scaling, gm._rotation, None, rs, raw=2)
        torch.cuda.synchronize()
        v = N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan)
        assert torch.equal(out["render"], color) and torch.equal(out["alpha"][0], 1 - v["final_T"].abs())
        plain = render(cam, gm, _aa_pipe(antialiasing=False), torch.zeros(3, device=DEV), depth_alpha=True)
    assert float(out["alpha"].max()) > 0.5 and float((plain["alpha"] - out["alpha"]).max()) > 0.05         # thinner than the plain frame's


def test_latent_model_trains_through_the_switch():
    from gaussian_renderer import render
    from test_gpu_structured import H as MH, W as MW, _model
    from diff_gaussian_rasterization import _native as N
    m = _model(1)
    cam, bg = S.make_camera(MW, MH).to(DEV), torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = (S.make_grad_image(MW, MH, 3) * 0.5 + 0.5).to(DEV)
    N.profile_enable(True)
    m()
    out = render(cam, m, _aa_pipe(), bg)
    (out["render"] - target).abs().mean().backward()
    torch.cuda.synchronize()
    prof = N.profile_read(128)
    N.profile_enable(False)
    assert prof["aa_fwd"][1] == 1 and prof["aa_bwd"][1] == 1 and prof["structured_bwd"][1] == 1, prof
    assert (out["radii"] > 0).sum() > 100
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, name
