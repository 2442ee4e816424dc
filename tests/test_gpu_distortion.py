"""GPU checks of the depth-distortion ops (diff_gaussian_rasterization/distortion.py, csrc/gsr_distortion.hip): the
kernels against the binary64 restatement (tests/distortion_ref.py) under its error rule, element by element, forward and every
gradient; two runs give the same bits, a gradient asked for alone has the bits it has beside the other, and non-contiguous inputs give
the contiguous call's bits; through a frame, on the cases of tests/test_gpu_extra.py: the distortion map against the float64 oracle's
blend of the same (m, m^2) and distortion_loss(...).backward() on every input leaf against the oracle's backward; render_with_distortion
is render() plus the maps; train() with lambda_dist, and without it the launches and bits of a run that never reaches the term.
Every check prints the worst ratio error / bound it saw.

Shapes of the ops alone (H x W; a block is 1 024 consecutive pixels, a thread four; the 16-byte path needs H W to be a multiple of 4):
    1x1, 17x33    one block, the 4-byte path, a ragged tail        12x20, 16x64   the 16-byte path: a ragged block, exactly one block
    130x257       33 blocks, the 4-byte path                       64x260         17 blocks, the 16-byte path
    513x513       258 blocks: the second stage of the loss (256 partials a trip) takes TWO trips - 257 blocks is the least that does,
                  so any H W above 256 x 1 024 = 262 144 would do; the 4-byte path.  512x516: 258 blocks on the 16-byte path."""
import numpy as np
import pytest
import torch

import distortion_ref as DR
import oracle
import scene_synth as S
import streams as ST
from test_distortion_ref import GRAD_LOSS, ratio
from test_gpu_extra import CASES, _bits, _id, _kwargs, _model, _reference
from test_gpu_parity import DEV, FRAGILE_CAP, _check_grads, _inputs, _settings, _strict_pixels

pytestmark = pytest.mark.gpu
F64 = torch.float64
MAP_SHAPES = [(1, 1), (17, 33), (12, 20), (16, 64), (130, 257), (64, 260), (513, 513), (512, 516)]
PIXEL_BOUND = 1e-5           # what tests/test_gpu_extra.py holds the extra map (|extra| <= 1) and test_gpu_depth_alpha._check_maps alpha to


def dev(a, grad=False):
    return torch.as_tensor(np.asarray(a)).to(DEV).contiguous().requires_grad_(grad)


def host(t):
    return t.detach().cpu()


# ---- the ops alone --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H, W", MAP_SHAPES)
def test_map_and_loss_against_the_reference(H, W):
    from diff_gaussian_rasterization.distortion import distortion_loss, distortion_map
    form = "holes" if (H, W) in ((17, 33), (130, 257), (512, 516)) else "linear" if (H, W) == (64, 260) else "ndc"
    mom, alpha = DR.make_maps(H, W, form)
    g = DR.make_upstream(H, W)
    n = H * W
    assert (DR.loss_blocks(n) > DR.SUM_BLOCK) == (n > 262144) and DR.loss_adds64(513 * 513) == DR.loss_adds64(262144) + 1
    tag = f"gpu {H}x{W} {form}"
    Mr, ar = (torch.tensor(v, dtype=F64, requires_grad=True) for v in (mom, alpha))
    Dr = DR.distortion_map_ref(Mr, ar)
    Dr.backward(torch.as_tensor(g, dtype=F64))
    t = DR.distortion_tracked(mom, alpha, grad_map=g)

    def run(want_m=True, want_a=True):
        M, a = dev(mom, want_m), dev(alpha[None], want_a)
        D = distortion_map(M, a)
        D.backward(dev(g[None]))
        return D, M, a
    D, M, a = run()
    assert D.shape == (1, H, W) and M.grad.shape == (3, H, W) and a.grad.shape == (1, H, W)
    assert ST.same_bits(host(M), torch.as_tensor(mom)) and ST.same_bits(host(a), torch.as_tensor(alpha[None]))          # unwritten
    assert ratio(host(D), DR.Tracked(Dr.detach(), t["D"].e), tag + " D") <= 1
    assert ratio(host(M.grad), DR.Tracked(Mr.grad, t["dmoments"].e), tag + " dmoments") <= 1
    assert ratio(host(a.grad), DR.Tracked(ar.grad, t["dalpha"].e), tag + " dalpha") <= 1
    assert int(host(M.grad[2]).view(torch.int32).abs().max()) == 0                                                    # plane 2: +0.0
    D2, M2, a2 = run()
    assert ST.same_bits(host(D2), host(D)) and ST.same_bits(host(M2.grad), host(M.grad)) and ST.same_bits(host(a2.grad), host(a.grad))
    _, M3, a3 = run(want_a=False)
    _, M4, a4 = run(want_m=False)
    assert a3.grad is None and M4.grad is None
    assert ST.same_bits(host(M3.grad), host(M.grad)) and ST.same_bits(host(a4.grad), host(a.grad))
    # the loss
    Ml, al = (torch.tensor(v, dtype=F64, requires_grad=True) for v in (mom, alpha))
    Lr = DR.distortion_loss_ref(Ml, al)
    Lr.backward(torch.tensor(GRAD_LOSS, dtype=F64))
    tl = DR.distortion_tracked(mom, alpha, grad_loss=GRAD_LOSS)

    def run_loss(want_m=True, want_a=True):
        M, a = dev(mom, want_m), dev(alpha[None], want_a)
        L = distortion_loss(M, a)
        L.backward(torch.tensor(GRAD_LOSS, device=DEV))
        return L, M, a
    L, M, a = run_loss()
    r = abs(float(L.detach()) - float(Lr.detach())) / float(tl["loss"].e)
    print(f"{tag} loss: worst error / bound = {r:.3f}")
    assert L.shape == () and r <= 1
    assert ratio(host(M.grad), DR.Tracked(Ml.grad, tl["dmoments"].e), tag + " dmoments (loss)") <= 1
    assert ratio(host(a.grad), DR.Tracked(al.grad, tl["dalpha"].e), tag + " dalpha (loss)") <= 1
    assert int(host(M.grad[2]).view(torch.int32).abs().max()) == 0
    L2, M2, a2 = run_loss()
    assert ST.same_bits(host(L2), host(L)) and ST.same_bits(host(M2.grad), host(M.grad)) and ST.same_bits(host(a2.grad), host(a.grad))
    _, M3, a3 = run_loss(want_a=False)
    _, M4, a4 = run_loss(want_m=False)
    assert a3.grad is None and M4.grad is None
    assert ST.same_bits(host(M3.grad), host(M.grad)) and ST.same_bits(host(a4.grad), host(a.grad))


@pytest.mark.parametrize("H, W", [(17, 33), (64, 260)])
def test_non_contiguous_inputs_give_the_contiguous_bits(H, W):
    from diff_gaussian_rasterization.distortion import distortion_loss, distortion_map
    mom, alpha = DR.make_maps(H, W, "ndc")
    wide = torch.zeros(5, H, W + 3)
    wide[1:4, :, 2:W + 2] = torch.as_tensor(mom)
    Ms = wide.to(DEV)[1:4, :, 2:W + 2]                                   # a sliced moments map: neither contiguous nor 16-byte aligned
    at = torch.as_tensor(alpha).t().contiguous().to(DEV).t()              # a transposed alpha [H,W]
    assert not Ms.is_contiguous() and not at.is_contiguous()
    Mc, ac = dev(mom, True), dev(alpha[None], True)
    Ms, at = Ms.requires_grad_(True), at.requires_grad_(True)
    for fn, up in ((distortion_map, dev(DR.make_upstream(H, W)[None])), (distortion_loss, torch.tensor(GRAD_LOSS, device=DEV))):
        for t in (Mc, ac, Ms, at):
            t.grad = None
        want, got = fn(Mc, ac), fn(Ms, at)
        want.backward(up)
        got.backward(up)
        assert ST.same_bits(host(got), host(want)) and ST.same_bits(host(Ms.grad), host(Mc.grad))
        assert at.grad.shape == (H, W) and ST.same_bits(host(at.grad), host(ac.grad[0]))


@pytest.mark.parametrize("mapping", ["ndc", "linear"])
@pytest.mark.parametrize("P", [1, 257, 100_003])
def test_depth_moments_against_the_reference(P, mapping):
    from diff_gaussian_rasterization.distortion import depth_moments
    means, V, g = DR.make_gaussians(P)
    mr = torch.tensor(means, dtype=F64, requires_grad=True)
    out, front = DR.depth_moments_ref(mr, V, mapping=mapping)
    out.backward(torch.as_tensor(g, dtype=F64))
    t = DR.depth_moments_tracked(means, V, mapping=mapping, grad_out32=g)
    assert int(t["fragile"].sum()) == 0 and torch.equal(t["front"], front)
    tag = f"gpu P={P} {mapping}"

    def run():
        m = dev(means, True)
        o = depth_moments(m, dev(V), mapping=mapping)
        o.backward(dev(g))
        return o, m
    o, m = run()
    assert o.shape == (P, 3) and ST.same_bits(host(m), torch.as_tensor(means))
    assert ratio(host(o), DR.Tracked(out.detach(), t["out"].e), tag + " moments") <= 1
    assert ratio(host(m.grad), DR.Tracked(mr.grad, t["dmeans"].e), tag + " dmeans") <= 1
    culled = ~front
    assert not bool(torch.signbit(host(o)[culled]).any()) and not bool(torch.signbit(host(m.grad)[culled]).any())
    assert int(host(o[:, 2]).view(torch.int32).abs().max()) == 0
    o2, m2 = run()
    assert ST.same_bits(host(o2), host(o)) and ST.same_bits(host(m2.grad), host(m.grad))
    if P == 257:                                                       # a sliced means3D gives the contiguous call's bits
        wide = torch.zeros(P, 5)
        wide[:, 1:4] = torch.as_tensor(means)
        sl = wide.to(DEV)[:, 1:4].requires_grad_(True)
        o3 = depth_moments(sl, dev(V), mapping=mapping)
        o3.backward(dev(g))
        assert not sl.is_contiguous() and ST.same_bits(host(o3), host(o)) and ST.same_bits(host(sl.grad), host(m.grad))


def test_exact_cases_are_strict_on_the_device():
    from diff_gaussian_rasterization.distortion import depth_moments, distortion_loss, distortion_map
    M = dev(np.array([[[1.0, 0.0]], [[4.0, 0.0]], [[9.0, 9.0]]], np.float32), True)
    a = dev(np.array([[[0.5, 0.0]]], np.float32), True)
    D = distortion_map(M, a)
    assert host(D).tolist() == [[[1.0, 0.0]]] and not bool(torch.signbit(host(D)).any())
    L = distortion_loss(M, a)
    assert float(L.detach()) == 0.5
    L.backward(torch.tensor(4.0, device=DEV))
    assert host(M.grad).tolist() == [[[-4.0, 0.0]], [[1.0, 0.0]], [[0.0, 0.0]]] and host(a.grad).tolist() == [[[8.0, 0.0]]]
    f = np.float32
    near = f(DR.NEAR)
    means = np.array([[0, 0, near], [1, -2, np.nextafter(near, f(1))], [0, 0, 0], [0, 0, -1], [3, 1, 0.5], [0, 0, np.nextafter(near, f(0))]], np.float32)
    for mapping in ("ndc", "linear"):
        m = dev(means, True)
        o = depth_moments(m, dev(np.eye(4, dtype=np.float32)), mapping=mapping)
        o.backward(torch.ones_like(o))
        twin = depth_moments(torch.as_tensor(means), torch.eye(4), mapping=mapping)      # (held to the numpy replay in test_distortion_ref.py)
        assert ST.same_bits(host(o), twin), (mapping, host(o), twin)
        cull = means[:, 2] <= (near if mapping == "ndc" else 0)
        assert not host(o)[cull].any() and not host(m.grad)[cull].any() and not bool(torch.signbit(host(m.grad)).any())
        assert bool((host(o)[~cull, 0] > 0).all()) and bool((host(m.grad)[~cull, 2] > 0).all())


# ---- through a frame ------------------------------------------------------------------------------------------------------------
_MOM = {}


def _moments_reference(c):
    """(the device's (m, m^2, 0) rows as numpy binary32, the float64 oracle's frame of the colours (m, m^2, 1) over a zero background:
    channels M1, M2 and alpha), once per scene; never modified."""
    from diff_gaussian_rasterization.distortion import depth_moments
    key = _id(c)
    if key not in _MOM:
        kw, _ = _kwargs(c)
        with torch.no_grad():
            mom = depth_moments(dev(np.asarray(kw["means3D"], np.float32)), dev(np.asarray(kw["viewmatrix"], np.float32))).cpu().numpy()
        col = mom.astype(np.float64)
        col[:, 2] = 1.0
        okw = {k: v for k, v in kw.items() if k != "shs"}
        okw.update(colors_precomp=col, bg=np.zeros(3))
        _MOM[key] = (mom, oracle.rasterize(dtype=np.float64, parallel=isinstance(c, str), **okw))
    return _MOM[key]


def _frame(c, grad):
    """The frame of case c with the depth moments of its own means3D as extra colours -> (outputs, leaves, means2D, moments)"""
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization.distortion import depth_moments
    kw, _ = _kwargs(c)
    rs = _settings(kw)
    inp = _inputs(kw, grad)
    means2D = torch.zeros(inp["means3D"].shape[0], 3, device=DEV, requires_grad=grad)
    mom = depth_moments(inp["means3D"], rs.viewmatrix)
    return GaussianRasterizer(rs, depth_alpha=True)(means2D=means2D, extra_colors=mom, **inp), inp, means2D, mom


def _strict(c, radii):
    fr_sh, fr_aux, _, _ = _reference(c)
    fr_mom = _moments_reference(c)[1]
    strict = _strict_pixels(fr_sh, radii.cpu().numpy()) & (fr_aux.fragile_px == 0) & (fr_mom.fragile_px == 0)
    assert 1 - strict.mean() < FRAGILE_CAP, f"too many fragile pixels: {1 - strict.mean():.5f}"
    return strict


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_distortion_map_of_a_frame_against_the_oracle(c):
    from diff_gaussian_rasterization import GaussianRasterizer
    from diff_gaussian_rasterization.distortion import distortion_map
    mom, fr_mom = _moments_reference(c)
    with torch.no_grad():
        (color, radii, depth, alpha, emap), inp, means2D, mom_dev = _frame(c, False)
        assert np.array_equal(host(mom_dev).numpy(), mom) and 0 <= mom[:, 0].min() and mom[:, 0].max() < 1
        # the frame is the extra_colors frame of those rows, bit for bit
        kw, _ = _kwargs(c)
        plain = GaussianRasterizer(_settings(kw), depth_alpha=True)(means2D=means2D, extra_colors=dev(mom), **inp)
        assert all(_bits(x, y) for x, y in zip(plain, (color, radii, depth, alpha, emap)))
        D = distortion_map(emap, alpha)
    strict = _strict(c, radii)
    M1, M2, A = fr_mom.color
    e = np.abs(host(emap).numpy()[:2] - fr_mom.color[:2]).max(0)
    ea = np.abs(host(alpha).numpy()[0] - A)
    assert e[strict].max() <= PIXEL_BOUND and ea[strict].max() <= PIXEL_BOUND          # the premise: the bounds the maps are already held to
    # |dD| <= M2 |dA| + A |dM2| + 2 |M1| |dM1| (+ the second-order terms) with every |d.| <= PIXEL_BOUND, plus the op's replayed bound
    t = DR.distortion_tracked(host(emap).numpy(), host(alpha).numpy()[0])
    bound = PIXEL_BOUND * (M2 + A + 2 * np.abs(M1)) + 2 * PIXEL_BOUND ** 2 + t["D"].e.numpy()
    err = np.abs(host(D).numpy()[0] - (A * M2 - M1 * M1))
    r = (err / bound)[strict].max()
    print(f"{_id(c)}: distortion map on {int(strict.sum())} strict pixels: max {err[strict].max():.2e}, worst error / bound = {r:.3f}; "
          f"D max {(A * M2 - M1 * M1)[strict].max():.2e}; extra map max error {e[strict].max():.2e}")
    assert r <= 1 and (A * M2 - M1 * M1)[strict].max() > 1e-4


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_loss_gradients_through_a_frame_against_the_oracle(c):
    """distortion_loss(...).backward() on every input leaf, means3D through both routes (the blend's weights and m).  The loss is taken
    over the strict pixels (the maps are multiplied by their mask, on both sides), so that every Gaussian is held to the strict bound,
    as tests/test_gpu_extra.py's upstream gradients are masked."""
    from diff_gaussian_rasterization.distortion import distortion_loss
    multi = isinstance(c, str)
    kw, _ = _kwargs(c)
    mom, fr_mom = _moments_reference(c)
    fr_sh = _reference(c)[0]
    (color, radii, depth, alpha, emap), inp, means2D, mom_dev = _frame(c, True)
    strict = _strict(c, radii)
    mask = dev(strict.astype(np.float32))
    loss = distortion_loss(emap * mask[None], alpha * mask[None])
    loss.backward()
    got = {k: v.grad.detach().cpu().numpy() for k, v in inp.items()}
    got["means2D"] = means2D.grad.detach().cpu().numpy()
    # the reference: binary64 gradients of the masked mean at the oracle's maps, through the oracle's backward ...
    maps = torch.tensor(fr_mom.color * strict[None], dtype=F64, requires_grad=True)
    Lr = DR.distortion_loss_ref(maps[:2], maps[2])
    Lr.backward()
    got_loss, want_loss = float(loss.detach()), float(Lr.detach())
    print(f"{_id(c)}: loss {got_loss:.6e}, reference {want_loss:.6e}")
    assert abs(got_loss - want_loss) <= PIXEL_BOUND * float(maps.detach()[1].mean() + maps.detach()[2].mean() + 2 * maps.detach()[0].mean()) + 1e-7
    want = fr_mom.backward(maps.grad.numpy() * strict[None], parallel=multi)
    # ... and the colours' gradient (dL/dm, dL/dm^2, .) through the reference's dm / dmeans3D
    mr = torch.tensor(np.asarray(kw["means3D"], np.float32), dtype=F64, requires_grad=True)
    rows, _ = DR.depth_moments_ref(mr, np.asarray(kw["viewmatrix"], np.float32))
    rows.backward(torch.as_tensor(want["colors_precomp"]))
    want = {n: want[n] for n in ("means3D", "means2D", "opacities", "scales", "rotations")}
    want["means3D"] = want["means3D"] + mr.grad.numpy()
    want["shs"] = np.zeros_like(got["shs"], dtype=np.float64)
    live, strict_live = _check_grads(fr_sh, want, got, ["means3D", "means2D", "opacities", "shs", "scales", "rotations"], masked=True)
    assert live > (1000 if multi else 0) and strict_live == live and not got["shs"].any()
    assert np.abs(mr.grad.numpy()).max() > 0 and np.abs(got["opacities"]).max() > 0


# ---- render_with_distortion -----------------------------------------------------------------------------------------------------
def _scene_model(c):
    from scene import GaussianModel
    from test_gpu_parity import _fixture_scene
    if isinstance(c, str):                                              # test_gpu_depth_alpha._uncovered_half_kwargs' scene
        scene = S.make_scene(260_000, 480, 320, 1, 91, scale_lo=0.01, scale_hi=0.07)
        scene.means3D[:, 1] = -scene.means3D[:, 1].abs() - 0.02 * scene.means3D[:, 2]
        cam, D = S.make_camera(480, 320), 1
    else:
        scene, cam, _ = _fixture_scene(c)
        D = c["D"]
    gm = GaussianModel(D)
    gm.adopt_scene(scene, device=DEV)
    return gm, cam.to(DEV)


@pytest.mark.parametrize("fused", [False, None], ids=["getter path", "raw path"])
@pytest.mark.parametrize("c", CASES, ids=_id)
def test_render_with_distortion_is_render_plus_the_maps(c, fused):
    from diff_gaussian_rasterization.distortion import depth_moments, distortion_map
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_with_distortion
    gm, cam = _scene_model(c)
    pipe = Pipe()
    pipe.fused_activations = fused
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    with torch.no_grad():
        one = render_with_distortion(cam, gm, pipe, bg)
        color = render(cam, gm, pipe, bg)
        ext = render(cam, gm, pipe, bg, depth_alpha=True, extra_colors=depth_moments(gm.get_xyz, cam.world_view_transform))
        lin = render_with_distortion(cam, gm, pipe, bg, near=0.1, far=50.0, mapping="linear", with_map=False)
    assert set(one) >= {"render", "radii", "viewspace_points", "visibility_filter", "depth", "alpha", "extra", "distortion"}
    assert ST.same_bits(one["render"], color["render"]) and ST.same_bits(one["radii"], color["radii"])
    for k in ("extra", "depth", "alpha"):
        assert ST.same_bits(one[k], ext[k]), k
    assert one["distortion"].shape == (1,) + tuple(one["render"].shape[1:]) and ST.same_bits(one["distortion"], distortion_map(ext["extra"], ext["alpha"]))
    assert float(one["distortion"].max()) > 1e-5 and float(one["extra"][2].abs().max()) == 0
    assert "distortion" not in lin and float(lin["extra"][0].max()) > float(one["extra"][0].max()) and ST.same_bits(lin["render"], color["render"])


def test_render_with_distortion_composes_and_refuses():
    from diff_gaussian_rasterization.distortion import distortion_loss
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_with_distortion
    from scene.latent_gaussian_model import LatentGaussianModel
    gm, cam = _model()
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    # gradients reach the positions through the weights and through m, on the raw path
    pkg = render_with_distortion(cam, gm, Pipe(), bg, with_map=False)
    distortion_loss(pkg["extra"], pkg["alpha"]).backward()
    assert float(gm._xyz.grad.abs().max()) > 0 and float(gm._opacity.grad.abs().max()) > 0 and bool(torch.isfinite(gm._xyz.grad).all())
    assert float(pkg["viewspace_points"].grad.abs().max()) > 0
    # antialiasing, and a model with a 3D filter, on both paths: render()'s image, bit for bit
    gm.compute_3D_filter([cam])
    for fused in (False, None):
        pipe = Pipe()
        pipe.fused_activations = fused
        pipe.antialiasing = True
        with torch.no_grad():
            one, color = render_with_distortion(cam, gm, pipe, bg), render(cam, gm, pipe, bg)
        assert ST.same_bits(one["render"], color["render"]) and ST.same_bits(one["radii"], color["radii"]) and float(one["distortion"].max()) > 1e-6
    pipe = Pipe()
    pipe.absgrad = True
    with pytest.raises(ValueError, match="absgrad"):
        render_with_distortion(cam, gm, pipe, bg)
    # a LatentGaussianModel: the decoded means are the frame's and the moments'
    torch.manual_seed(3)
    lm = LatentGaussianModel(1, torch.randn(64, 3) * 0.3 + torch.tensor([0.0, 0.0, 3.0]), gaussians_per_structure=4).to(DEV)
    lm()
    one = render_with_distortion(cam, lm, Pipe(), bg)
    with torch.no_grad():
        color = render(cam, lm, Pipe(), bg)
    assert ST.same_bits(one["render"].detach(), color["render"]) and bool(torch.isfinite(one["distortion"]).all())
    distortion_loss(one["extra"], one["alpha"]).backward()
    assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in lm.parameters())


# ---- train() --------------------------------------------------------------------------------------------------------------------
DIST_SCOPES = {"depth_moments_fwd", "depth_moments_bwd", "distortion_loss_fwd", "distortion_loss_bwd", "distortion_map_fwd", "distortion_map_bwd"}


def test_training_loop_with_and_without_the_distortion_term():
    from test_gpu_extra import _train                                    # -> (model, image losses, {scope: launches}, frames rendered)
    off, losses_off, scopes_off, fwd_off = _train(iterations=6)
    assert not DIST_SCOPES & set(scopes_off), "the default loop launched a distortion kernel"
    assert "render_fwd_ext" not in scopes_off and fwd_off == 6
    # a weight whose first iteration lies behind the window: the same launches, the same bits
    late, losses_late, scopes_late, fwd_late = _train(iterations=6, lambda_dist=100.0)
    assert scopes_late == scopes_off and fwd_late == fwd_off and losses_late == losses_off
    for name in ("_xyz", "_rotation", "_scaling", "_opacity", "_features"):
        assert ST.same_bits(host(getattr(late, name)), host(getattr(off, name))), name
    on, losses_on, scopes_on, fwd_on = _train(iterations=6, lambda_dist=100.0, dist_from_iter=1)
    for name in ("depth_moments_fwd", "depth_moments_bwd", "distortion_loss_fwd", "distortion_loss_bwd"):
        assert scopes_on.get(name) == 6, (name, scopes_on.get(name))                 # iterations 1 .. 6: one launch each way
    assert "distortion_map_fwd" not in scopes_on                                     # the fused loss: the map is never stored
    assert fwd_on == 6 and scopes_on.get("render_fwd_ext", 0) >= 6                   # one frame an iteration, no second render
    assert losses_on[0] == losses_off[0] and all(np.isfinite(losses_on))             # the reported loss is the image loss alone
    assert not torch.equal(on._xyz, off._xyz) and all(bool(torch.isfinite(getattr(on, n)).all()) for n in ("_xyz", "_opacity", "_scaling"))
    # with the two-frame normal term, sparse Adam, MCMC, the bilateral grid and the 3D filter
    for kw in (dict(lambda_normal=0.05, normal_from_iter=2), dict(optimizer_type="sparse_adam"), dict(densify_strategy="mcmc"),
               dict(bilateral_grid=True), dict(filter_3d=True)):
        gm, losses, scopes, fwd = _train(iterations=3, lambda_dist=100.0, dist_from_iter=2, **kw)
        assert scopes.get("distortion_loss_bwd") == 2 and all(np.isfinite(losses)) and bool(torch.isfinite(gm._xyz).all()), kw
        assert fwd == (5 if "lambda_normal" in kw else 3), (kw, fwd)
    for kw, why in ((dict(lambda_dist=-1.0), "at least 0"), (dict(lambda_dist=1.0, lambda_normal=0.05, normal_in_frame=True), "fourth extra channel"),
                    (dict(lambda_dist=1.0, densify_absgrad=True), "depth and alpha")):
        with pytest.raises(ValueError, match=why):
            _train(iterations=1, **kw)
