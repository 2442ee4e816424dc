"""The oracle's front-to-back backward (the HIP backward's algebra: E = <out - C_ckpt, dL/dpix> rebuilt every 128 entries, then
E -= w <c, dL/dpix> and dL/dalpha = T <c, dL/dpix> - E / (1 - alpha)), its per-instance transmittance, the fragile-pixel causes, and
the per-Gaussian gradient checker of tests/gradcheck.py -- all on the CPU.

The frame is the deep small frame of the GPU suite (gradcheck.deep_small_kwargs: the cfg3n recipe, dense enough that lists pass 384
entries and the blend reaches the transmittance cut-off in the third list segment or later), so every T_max stratum is populated.
"""
import numpy as np
import pytest

import gradcheck as GC
import oracle
import scene_synth as S

NAMES = ("means3D", "means2D", "opacities", "shs", "scales", "rotations")


@pytest.fixture(scope="module")
def deep():
    kw = GC.deep_small_kwargs()
    f64 = oracle.rasterize(dtype=np.float64, parallel=True, **kw)
    f32 = oracle.rasterize(dtype=np.float32, parallel=True, **kw)
    W, H = kw["image_width"], kw["image_height"]
    gimg = np.where((f64.fragile_px == 0)[None], S.make_grad_image(W, H, GC.DEEP_SMALL["seed"]).numpy(), 0.0)
    out = dict(kw=kw, f64=f64, f32=f32, gimg=gimg)
    out["want"] = f64.backward(gimg.astype(np.float64), parallel=True)
    out["want_f2b"] = f64.backward(gimg.astype(np.float64), parallel=True, order="front_to_back")
    out["b2f"] = f32.backward(gimg.astype(np.float32), parallel=True)
    out["f2b"] = f32.backward(gimg.astype(np.float32), parallel=True, order="front_to_back")
    out["T_max"] = f64.T_max()
    out["min_pos"] = GC.oracle_min_position(f64)
    return out


def test_inst_T_is_the_transmittance_in_front_of_each_instance():
    """Three splats on the image centre, one behind the other: T_max of the front one is 1, of the next 1 - alpha_front at the
    pixel where the front one is faintest among those the back one is composited at (the largest T over them), and so on."""
    W = H = 16
    cam = S.make_camera(W, H)
    means = np.array([[0.0, 0.0, 2.0], [0.0, 0.0, 2.5], [0.0, 0.0, 3.0]])
    op = np.array([[0.6], [0.5], [0.9]])
    kw = dict(image_height=H, image_width=W, tanfovx=0.5, tanfovy=0.5, bg=np.zeros(3), scale_modifier=1.0,
              viewmatrix=cam.world_view_transform.numpy(), projmatrix=cam.full_proj_transform.numpy(), sh_degree=0,
              campos=np.zeros(3), means3D=means, opacities=op, colors_precomp=np.full((3, 3), 0.5),
              scales=np.full((3, 3), 0.3), rotations=np.tile([1.0, 0, 0, 0], (3, 1)))
    fr = oracle.rasterize(dtype=np.float64, **kw)
    assert list(fr.point_list) == [0, 1, 2]
    Tm = fr.T_max()
    # the nearer splats are larger on screen: wherever a farther one is composited, the ones in front are too
    assert Tm[0] == 1.0
    assert 1 - op[0, 0] <= Tm[1] < 1
    assert (1 - op[0, 0]) * (1 - op[1, 0]) <= Tm[2] < Tm[1]
    assert fr.stopped.sum() == 0 and fr.inst_T.shape == (3,)


def test_fragile_bits_name_the_causes(deep):
    """fragile_px is a bit mask (oracle.FRAGILE_BITS); `!= 0` still means fragile, and the deep frame has pixels of the alpha and
    T cut-off bands.  The binary32 instantiation marks the same pixels (the bands are evaluated in each precision)."""
    f64 = deep["f64"]
    counts = f64.fragile_counts()
    print("deep small frame: fragile pixels by cause", counts, "of", f64.W * f64.H, "; stopped at the cut-off:", int(f64.stopped.sum()))
    assert set(np.unique(f64.fragile_px)) <= set(range(32))
    assert counts["any"] == int(f64.fragile_px.astype(bool).sum()) <= sum(v for k, v in counts.items() if k != "any")
    assert counts["alpha"] > 0 and counts["T_cut"] > 0
    assert counts["any"] / (f64.W * f64.H) < 0.03
    assert f64.stopped.mean() > 0.01


def test_front_to_back_restatement_equals_a9_in_binary64(deep):
    """In binary64 the front-to-back algebra is A.9 (the cancellation in E costs ~1e-16 / T): equal to 1e-9 of each tensor's scale."""
    for n in NAMES:
        w, g = deep["want"][n], deep["want_f2b"][n]
        assert np.abs(g - w).max() <= 1e-9 * np.abs(w).max(), n


def test_cancellation_front_to_back_by_T_max(deep):
    """The measured answer to "how much does dL/dalpha = T cdp - E / (1 - alpha) lose at low T": both binary32 oracles against
    binary64, per Gaussian and leaf, by T_max stratum.  In the two shallow strata front to back is within 3x of back to front
    (p50 and p99); the deep strata's excess is printed and recorded in DESIGN.md section 2."""
    live = np.isfinite(GC.per_gaussian_error(deep["want"], deep["want"], ["means3D"])["means3D"])
    e_b = GC.per_gaussian_error(deep["want"], deep["b2f"], NAMES)
    e_f = GC.per_gaussian_error(deep["want"], deep["f2b"], NAMES)
    strata = GC.t_max_strata(deep["T_max"])
    for lab, (mask, _) in strata.items():
        m = mask & live
        assert m.sum() >= 100, (lab, int(m.sum()))
        for n in ("means3D", "opacities", "rotations", "shs"):
            ok = m & np.isfinite(e_b[n])
            qb, qf = np.quantile(e_b[n][ok], [0.5, 0.99]), np.quantile(e_f[n][ok], [0.5, 0.99])
            print(f"  {lab:24s} {n:10s} n={int(ok.sum()):6d}  back-to-front p50 {qb[0]:.2e} p99 {qb[1]:.2e} | "
                  f"front-to-back p50 {qf[0]:.2e} p99 {qf[1]:.2e} | ratio {qf[0] / qb[0]:.2f} {qf[1] / qb[1]:.2f}")
            if lab in ("T_max in [1e-1, 1]", "T_max in [1e-2, 1e-1)"):
                assert qf[0] <= 3 * qb[0] and qf[1] <= 3 * qb[1], (lab, n, qb, qf)


def test_checker_catches_what_the_tensor_wide_bound_passes(deep):
    """Self-test of gradcheck.check_grads_per_gaussian, with the binary32 oracle as "got": it passes the front-to-back binary32 oracle
    and fails two perturbations applied only to the Gaussians behind low transmittance (T_max < 1e-2) or deep in the list
    (every instance at position >= 256): their gradients scaled by 1 + 1e-2, and an error proportional to T_max added.
    The test records what test_gpu_parity._check_grads (tensor-wide bound) says about each: the T-proportional error passes it."""
    from test_gpu_parity import _check_grads
    f64, want = deep["f64"], deep["want"]
    yard = GC.yardstick(want, deep["b2f"], deep["f2b"], NAMES)
    strata = GC.t_max_strata(deep["T_max"], {"T_max in [1e-3, 1e-2)": 100})
    strata["every instance at position >= 256"] = (deep["min_pos"] >= 256, 1000)
    GC.check_grads_per_gaussian(want, yard, deep["f2b"], strata, NAMES, label="binary32 front to back")
    target = (deep["T_max"] < 1e-2) | (deep["min_pos"] >= 256)
    assert target.sum() > 1000

    def perturbed(kind):
        got = {}
        for n in NAMES:
            g = deep["f2b"][n].astype(np.float64).copy()
            t = target.reshape((-1,) + (1,) * (g.ndim - 1))
            if kind == "scale":
                g = np.where(t, g * (1 + 1e-2), g)
            else:               # an absolute error of 2e-5 x the tensor's scale x T_max: what a checkpoint off by 2e-5 leaves
                Tm = deep["T_max"].reshape(t.shape)
                g = np.where(t, g + 2e-5 * np.abs(want[n]).max() * Tm * np.sign(want[n]), g)
            got[n] = g
        return got

    def old_bound_passes(got):
        try:
            _check_grads(f64, want, got, list(NAMES), masked=True)
            return True
        except AssertionError:
            return False
    results = {}
    for kind in ("scale by 1 + 1e-2", "error proportional to T_max"):
        got = perturbed("scale" if kind.startswith("scale") else "T")
        fails = GC.check_grads_per_gaussian(want, yard, got, strata, NAMES, label=kind, raise_on_fail=False)
        results[kind] = (old_bound_passes(got), bool(fails))
        print(f"{kind}: tensor-wide bound {'PASSES' if results[kind][0] else 'fails'}; per-Gaussian check "
              f"{'fails' if fails else 'PASSES'} ({len(fails)} reports, first: {fails[:1]})")
    assert all(new_fails for _, new_fails in results.values()), results
    assert results["error proportional to T_max"][0], "the gap this checker closes: the tensor-wide bound passes a T-proportional error"
