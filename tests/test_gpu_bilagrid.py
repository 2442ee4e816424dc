"""csrc/gsr_bilagrid.hip on the GPU: the slice-and-apply forward, both of its gradients and the total variation, every element against
the float64 reference (tests/bilagrid_ref.py) under its error rule; what must be zero or untouched is compared bit for bit, two runs
give the same bits, and a gradient asked for alone has the bits it has beside the other.  Then the op behind the rasterizer in front
of the loss (native against the torch path), and train() with the switch on, off and absent.

Worst errors in units of the bound on an MI355X (printed by every test; DESIGN section 17 keeps the table): out 0.023, dgrids 0.047,
dimage 0.013, tv value 0.013, tv gradient 0.336."""
import random
from dataclasses import replace
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bilagrid_ref as BR
import scene_synth as S
from diff_gaussian_rasterization import bilagrid

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = lambda s: "x".join(map(str, s))


def host(t):
    return t.detach().cpu().numpy()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def run_native(ref, want_grids=True, want_image=True):
    grids = ref.grids.to(DEV).requires_grad_(want_grids)
    image = ref.image.to(DEV).requires_grad_(want_image)
    before = bits(grids).clone()
    out = bilagrid.slice_apply(grids, image, BR.IDX, native=True)
    out.backward(ref.go.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(bits(grids), before), "the grids were written"
    return out.detach(), grids.grad, image.grad


# ---- slice and apply -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BR.SHAPES, ids=IDS)
def test_slice_apply_against_the_reference(shape):
    ref = BR.reference(shape)
    out, dgrids, dimage = run_native(ref)
    assert out.shape == ref.image.shape and dgrids.shape == ref.grids.shape and dimage.shape == ref.image.shape
    assert out.dtype == dgrids.dtype == dimage.dtype == torch.float32
    # the rows of the other images: exactly zero (+0: all bits)
    assert not bits(dgrids[0]).any() and not bits(dgrids[2]).any()
    BR.check_slice(ref, host(out), host(dgrids[BR.IDX]), host(dimage), f"native {shape}")
    # the same inputs give the same bits
    out2, dgrids2, dimage2 = run_native(ref)
    assert torch.equal(bits(out), bits(out2)) and torch.equal(bits(dgrids), bits(dgrids2)) and torch.equal(bits(dimage), bits(dimage2))
    # a gradient asked for alone has the bits it has beside the other
    out_g, dgrids_g, none_i = run_native(ref, want_image=False)
    out_i, none_g, dimage_i = run_native(ref, want_grids=False)
    assert none_i is None and none_g is None
    assert torch.equal(bits(out_g), bits(out)) and torch.equal(bits(out_i), bits(out))
    assert torch.equal(bits(dgrids_g), bits(dgrids)) and torch.equal(bits(dimage_i), bits(dimage))


def test_slice_apply_picks_the_grid_of_idx_and_refuses_bad_input():
    ref = BR.reference(BR.SHAPES[1])
    grids, image = ref.grids.to(DEV), ref.image.to(DEV)
    outs = [bilagrid.slice_apply(grids, image, i) for i in range(3)]             # native=None: device tensors go native
    assert torch.equal(bits(outs[1]), bits(run_native(ref)[0])) and not torch.equal(outs[0], outs[1]) and not torch.equal(outs[2], outs[1])
    eye = bilagrid.BilateralGrid(2, 4, 3, 2).to(DEV)
    assert float((eye(image, 1).detach() - image).abs().max()) <= 1e-6
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.slice_apply(grids, image.transpose(1, 2), 1)
    with pytest.raises(ValueError, match="contiguous float32"):
        bilagrid.slice_apply(grids.double(), image, 1)
    with pytest.raises(IndexError):
        bilagrid.slice_apply(grids, image, 3)
    with pytest.raises(ValueError, match="grids are on"):
        bilagrid.slice_apply(grids.cpu(), image, 1, native=True)
    empty = bilagrid.slice_apply(grids.clone().requires_grad_(True), torch.zeros(3, 0, 7, device=DEV), 1)
    assert empty.shape == (3, 0, 7)


# ---- total variation -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", BR.TV_SHAPES, ids=IDS)
def test_total_variation_against_the_reference(shape):
    ref = BR.tv_reference(shape)

    def run():
        grids = ref.grids.to(DEV).requires_grad_(True)
        tv = bilagrid.total_variation_loss(grids, native=True)
        (tv * ref.upstream).backward()
        torch.cuda.synchronize()
        return tv.detach(), grids.grad
    tv, grad = run()
    assert tv.shape == () and grad.shape == ref.grids.shape
    assert torch.isfinite(tv) and torch.isfinite(grad).all()
    if shape[1:] == (1, 1, 1):
        assert float(tv) == 0.0 and not grad.any()
    BR.check_tv(ref, float(tv), host(grad), f"native tv {shape}")
    for _ in range(3):                                       # the same bits, whichever block draws the last ticket
        tv2, grad2 = run()
        assert torch.equal(bits(tv.reshape(1)), bits(tv2.reshape(1))) and torch.equal(bits(grad), bits(grad2))


def test_total_variation_of_many_grids():
    """More elements than one pass of the blocks covers (the grid-stride loop) and every block of the launch in use."""
    ref = BR.tv_reference((40, 8, 16, 16))
    grids = ref.grids.to(DEV).requires_grad_(True)
    tv = bilagrid.total_variation_loss(grids)
    (tv * ref.upstream).backward()
    BR.check_tv(ref, float(tv.detach()), host(grids.grad), "native tv of 40 grids")


# ---- behind the rasterizer, in front of the loss ---------------------------------------------------------------------------------------
def test_render_grid_loss_backward_native_against_torch():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    from scene import GaussianModel, OptimizationDefaults
    W = H = 64
    cam = S.arc_cameras(W, H, 1)[0].to(DEV)
    scene = S.make_scene(2000, W, H, 2, 11, scale_lo=0.01, scale_hi=0.08)
    bg = torch.tensor([0.1, 0.2, 0.3], device=DEV)
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(3)).to(DEV)
    grids0 = BR.make_inputs(H, W, 8, 16, 16, seed=9)[0]

    def run(native):
        gm = GaussianModel(2)
        gm.adopt_scene(scene, device=DEV)
        gm.training_setup(OptimizationDefaults())
        bg_module = bilagrid.BilateralGrid(3).to(DEV)
        with torch.no_grad():
            bg_module.grids.copy_(grids0.to(DEV))
        image = render(cam, gm, Pipe(), bg)["render"]
        out = bg_module(image, BR.IDX, native=native)
        out.retain_grad()
        training_loss(out, target, 0.2).backward()
        torch.cuda.synchronize()
        leaves = {k: host(t.grad) for k, t in gm._t.items()}
        return leaves, bg_module.grids.grad, image.detach(), out.grad
    leaves_n, dgrids_n, image, go = run(True)
    leaves_t, dgrids_t, image_t, _ = run(False)
    assert torch.equal(image, image_t)
    for k, want in leaves_t.items():
        got = leaves_n[k]
        err, bound = np.abs(got - want), 1e-4 * np.abs(want).max() + 1e-4 * np.abs(want)
        assert np.abs(want).max() > 0 and (err <= bound).all(), f"{k}: worst {np.max(err / bound):.3f} x the gradient bound"
        print(f"{k}: worst error {np.max(err / bound):.3f} x the gradient bound")
    ref = BR.Reference(H, W, 8, 16, 16, tensors=(grids0, image.cpu(), go.cpu()))
    for label, dg in (("native", dgrids_n), ("torch on the device", dgrids_t)):
        assert not dg[0].any() and not dg[2].any()
        BR.check_slice(ref, None, host(dg[BR.IDX]), None, f"render -> grid -> loss, {label}")


# ---- the training loop -----------------------------------------------------------------------------------------------------------------
class _Recording(list):
    def __init__(self, items):
        super().__init__(items)
        self.seen = []

    def __getitem__(self, i):
        self.seen.append(i)
        return super().__getitem__(i)


def _training_fixture():
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    W, H = 96, 64
    base = [c.to(DEV) for c in S.arc_cameras(W, H, 4)]
    scene = S.make_scene(2000, W, H, 2, 30, scale_lo=0.01, scale_hi=0.08)
    truth = GaussianModel(2)
    truth.adopt_scene(scene, device=DEV)
    bg = torch.zeros(3, device=DEV)
    with torch.no_grad():                                          # every view with an exposure and a tint of its own
        targets = [(render(c, truth, Pipe(), bg)["render"] * torch.tensor([0.8 + 0.1 * i, 1.0, 1.1 - 0.1 * i], device=DEV).view(3, 1, 1)).clone()
                   for i, c in enumerate(base)]
    return scene, base, targets, bg


def _fresh_model(scene, opt):
    from scene import GaussianModel
    gm = GaussianModel(2)
    gm.adopt_scene(scene, device=DEV)
    gm.training_setup(opt)
    return gm


@pytest.mark.parametrize("optimizer_type", ("default", "sparse_adam"))
def test_training_loop_with_the_bilateral_grid(optimizer_type):
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, base, targets, bg = _training_fixture()
    opt = replace(OptimizationDefaults(), bilateral_grid=True, bilateral_grid_shape=(4, 3, 2), densify_from_iter=10 ** 9, densify_until_iter=0,
                  optimizer_type=optimizer_type)
    gm = _fresh_model(scene, opt)
    cams = _Recording(base * 10)                                   # 40 images, 29 steps: some are never visited
    losses = []
    random.seed(1)
    torch.manual_seed(1)
    train(gm, cams, targets * 10, opt, Pipe(), bg, iterations=30, scene_extent=3.0,
          on_iteration=lambda it, loss, g: losses.append(float(loss.detach())))
    assert len(losses) == 30 and all(np.isfinite(losses))
    grids = gm.bilagrid.grids.detach()
    assert tuple(grids.shape) == (40, 12, 2, 3, 4) and torch.isfinite(grids).all()
    eye = torch.eye(4, device=DEV)[:3].reshape(1, 12, 1, 1, 1).expand_as(grids)
    moved = (grids != eye).flatten(1).any(1).cpu().numpy()
    stepped = np.zeros(40, bool)
    stepped[cams.seen[:29]] = True                                 # the last iteration renders without a step
    assert stepped.sum() < 40 and np.array_equal(moved, stepped), (moved, stepped)
    # the warm-up holds the steps small: Adam moves a coefficient by at most (1 - beta1) / sqrt(1 - beta2) = 3.17 learning rates per
    # step, whatever the gradients were; without the warm-up a single visit and its momentum would carry a coefficient past this
    lr_sum = sum(bilagrid.bilateral_grid_lr(opt.bilateral_grid_lr, it, 30) for it in range(29))
    assert 0 < float((grids - eye).abs().max()) <= 3.17 * lr_sum


def test_training_loop_without_the_switch_is_the_loop_as_it_was():
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    scene, base, targets, bg = _training_fixture()
    off = replace(OptimizationDefaults(), densify_from_iter=10 ** 9, densify_until_iter=0)
    assert off.bilateral_grid is False
    absent = SimpleNamespace(**{k: v for k, v in vars(off).items() if not k.startswith("bilateral_grid")})
    finals = []
    for opt, kw in ((off, dict(bilagrid=None)), (off, dict(bilagrid=None)), (absent, dict())):
        gm = _fresh_model(scene, off)
        random.seed(2)
        torch.manual_seed(2)
        train(gm, base, targets, opt, Pipe(), bg, iterations=12, scene_extent=3.0, **kw)
        assert not hasattr(gm, "bilagrid")
        finals.append({k: bits(t).clone() for k, t in gm._t.items()})
    for k in finals[0]:
        assert torch.equal(finals[0][k], finals[1][k]) and torch.equal(finals[0][k], finals[2][k]), k
