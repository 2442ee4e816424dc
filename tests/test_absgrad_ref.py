"""Absgrad without a device: the float64 reference (tests/absgrad_ref.py) anchored to the oracle, a single symmetric splat whose
signed gradient cancels while its absolute sums do not, the C ABI's two additive calls, and the host path of the densification
statistics."""
import os

import numpy as np
import pytest
import torch

import absgrad_ref as AR
import oracle
import scene_synth as S
import test_gpu_parity as TP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ANCHOR_FIXTURES = (0, 2, 4, 6, 8)


@pytest.mark.parametrize("i", ANCHOR_FIXTURES)
def test_reference_signed_sums_equal_the_oracles_means2D_gradient(i):
    """(a) signed sums == fr64.backward(g)["means2D"][:, :2] within 1e-12 x max|want|; absolute sums >= |signed| elementwise."""
    c = TP.FIXTURES[i]
    kw = TP._fixture_kwargs(c)
    fr = oracle.rasterize(dtype=np.float64, **kw)
    gimg = S.make_grad_image(c["W"], c["H"], c["seed"]).numpy().astype(np.float64)
    want = fr.backward(gimg)["means2D"][:, :2]
    signed, absolute = AR.signed_and_abs_means2D(fr, kw["bg"], gimg)
    scale = np.abs(want).max()
    err = np.abs(signed - want).max()
    live = np.abs(want).max(1) > 0
    ratio = np.median(np.linalg.norm(absolute[live], axis=1) / np.linalg.norm(want[live], axis=1)) if live.any() else float("nan")
    nz = np.abs(want) > 0
    per_component = np.median(absolute[nz] / np.abs(want[nz])) if nz.any() else float("nan")
    print(f"fixture {i}: max |signed - oracle| = {err:.3e} (scale {scale:.3e}); median absgrad / |grad| = {per_component:.2f} per "
          f"component, {ratio:.2f} as a ratio of row norms")
    assert scale > 0 and err <= 1e-12 * scale
    assert (absolute >= np.abs(signed)).all()


def test_symmetric_single_splat_cancels_signed_but_not_absolute():
    """(b) one isotropic splat, opacity 0.2, centred on a pixel centre, constant dL/dcolor: signed <= 1e-12 x absolute, absolute > 0."""
    kw = AR.single_splat_kwargs()
    fr = oracle.rasterize(dtype=np.float64, **kw)
    assert np.abs(fr.xy[0] - np.round(fr.xy[0])).max() <= 1e-12 and fr.radii[0] > 0
    gimg = np.ones((3, kw["image_height"], kw["image_width"])) * np.array([0.3, -0.8, 0.5])[:, None, None]
    signed, absolute = AR.signed_and_abs_means2D(fr, kw["bg"], gimg)
    print(f"single splat: signed {signed[0]}, absolute {absolute[0]}")
    assert (absolute[0] > 0).all()
    assert (np.abs(signed[0]) <= 1e-12 * absolute[0]).all()
    want = fr.backward(gimg)["means2D"][0, :2]
    assert (np.abs(want) <= 1e-12 * absolute[0]).all()


def test_abi_declares_and_exports_the_absgrad_calls():
    """(c) additive ABI: both symbols declared in the header, exported by the library and bound; the version is still 12."""
    import re

    from diff_gaussian_rasterization import _native as native
    lib = native.load()
    hdr = open(os.path.join(ROOT, "include", "gsrast.h")).read()
    declared = set(re.findall(r"\b(gsr_[a-z0-9_]+)\s*\(", hdr))
    for name in ("gsr_backward_render_abs", "gsr_screen_absgrad"):
        assert name in declared, f"{name} not declared in gsrast.h"
        assert hasattr(lib, name), f"{name} not exported"
        assert name in native.EXPORTS
    assert lib.gsr_version() == 12
    assert re.search(r"#define\s+GSR_VERSION\s+12\b", hdr)


def _model(P, absgrad):
    from dataclasses import replace

    from scene import GaussianModel, OptimizationDefaults
    gm = GaussianModel(1)
    gm.adopt_scene(S.make_scene(P, 64, 64, 1, 7), device="cpu")
    gm.training_setup(replace(OptimizationDefaults(), densify_absgrad=absgrad))
    return gm


def test_host_densification_stats_follow_densify_absgrad():
    """(d) CPU tensors: flag on -> accumulates |absgrad[:, :2]|; off -> |grad[:, :2]| (the two chosen different); on without .absgrad
    -> ValueError naming pipe.absgrad."""
    from scene import OptimizationDefaults
    assert OptimizationDefaults().densify_absgrad is False and OptimizationDefaults().densify_grad_threshold == 0.0002
    P = 40
    gen = torch.Generator().manual_seed(6)
    grad, absgrad = torch.randn(P, 3, generator=gen), torch.rand(P, 3, generator=gen) + 2.0
    radii = (torch.rand(P, generator=gen) < 0.7).int() * 3
    vis = radii > 0
    for on in (False, True):
        gm = _model(P, on)
        vsp = torch.zeros(P, 3, requires_grad=True)
        vsp.grad, vsp.absgrad = grad.clone(), absgrad.clone()
        gm.update_densification_stats(vsp, radii)
        want = torch.zeros(P, 1)
        want[vis] = torch.norm((absgrad if on else grad)[vis, :2], dim=-1, keepdim=True)
        assert torch.equal(gm.xyz_gradient_accum, want)
        assert torch.equal(gm.denom, vis.float()[:, None])
        assert torch.equal(gm.max_radii2D, radii.to(gm.max_radii2D.dtype))
    gm = _model(P, True)
    vsp = torch.zeros(P, 3, requires_grad=True)
    vsp.grad = grad.clone()
    with pytest.raises(ValueError, match="pipe.absgrad"):
        gm.update_densification_stats(vsp, radii)


def test_pipe_default_and_refusals_without_a_device():
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    from gaussian_params import Pipe
    assert Pipe.absgrad is False
    z = torch.zeros(3)
    rs = GaussianRasterizationSettings(8, 8, 0.5, 0.5, z, 1.0, torch.eye(4), torch.eye(4), 0, z, False, False)
    assert GaussianRasterizer(rs).absgrad is False and GaussianRasterizer(rs, absgrad=True).absgrad is True
    with pytest.raises(ValueError, match="depth_alpha"):
        GaussianRasterizer(rs, depth_alpha=True, absgrad=True)
