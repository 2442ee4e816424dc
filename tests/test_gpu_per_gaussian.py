"""Every Gaussian's gradient held to its own scale (tests/gradcheck.py), by how the HIP backward reaches it, plus the blend decisions
against the oracle's, pixel by pixel.

test_gpu_parity._check_grads bounds each gradient tensor relative to its largest element: the Gaussians behind low transmittance --
the ones the HIP backward (csrc/gsr_render.hip k_render_bwd) reaches from a segment checkpoint (every kSeg = 128 list entries) or a
chunk-start checkpoint, carrying the front-to-back state E -- have small gradients and so the loosest check.  Here, per Gaussian and
leaf, e(g) = max_k |got - want| / max_k |want| against the binary64 oracle, compared with yard32(g): the larger of the two binary32
oracles' errors (A.9 back to front, and the kernel's algebra front to back: oracle backward order="front_to_back").

Strata: T_max (the largest transmittance in front of the Gaussian over the pixels it is composited at, oracle inst_T), and from HIP's
own culled lists: some instance at position < 128 of chunk 0; every instance at position >= 128 (segment checkpoint); every instance
in a chunk >= 1 (chunk-start checkpoint).  The tensor-wide bound stays in place next to this check (the frames below run it too).

Bounds (gradcheck.Q_FACTOR, Q_ADD, G_FACTOR): per stratum and leaf p50 and p99 of e at most 4x those of yard32 + 1e-6, and every
Gaussian within G_FACTOR x max(yard32(g), the stratum's median yard32).  Measured on an MI355X (first run): the largest ratio of
e's p50 to yard32's over all strata and leaves is 1.74, of the p99s 3.27 (uncovered half, segment stratum; 1.29 and 1.18 on the deep
small frame).  Single Gaussians reach 142x their max(yard32(g), median) -- in every stratum, the shallowest included, so not a
checkpoint: the kernel's alpha (exp2 of the pre-scaled conic) rounds differently from both oracles', which matters for the few Gaussians
whose gradient cancels over their pixels -- hence G_FACTOR = 512.  Scratch mutants of k_render_bwd that scale the checkpoint T at segment
or chunk starts by 1 + 2^-12 fail the p50 / p99 bounds here (uncovered half: p99 4x and more above yard32's).
"""
import numpy as np
import pytest
import torch

import gradcheck as GC
import oracle
import scene_synth as S
from test_gpu_parity import (GRAD_NAMES, _check_forward, _check_grads, _decode_n_contrib, _inputs, _per_tile_lists, _run_gpu, _settings,
                             _strict_pixels, fragile_cap)
from util import raster_kwargs

pytestmark = pytest.mark.gpu

SEG = 128


def _hip_frame_views(kw):
    """HIP's own culled per-tile lists and per-pixel decisions of the frame (the standard API's forward; deterministic)."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _native as N
    rs, inp = _settings(kw), _inputs(kw, False)
    _, _, fr = dgr.rasterize_forward(inp["means3D"], inp.get("shs"), inp.get("colors_precomp"), inp["opacities"], inp.get("scales"),
                                     inp.get("rotations"), inp.get("cov3D_precomp"), rs)
    torch.cuda.synchronize()
    v = N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, fr.plan)
    W, H = kw["image_width"], kw["image_height"]
    Gx, Gy = (W + 15) // 16, (H + 15) // 16
    Tn, C = Gx * Gy, fr.plan.chunks_run
    P = np.asarray(kw["means3D"]).shape[0]
    sg = v["sorted_gaussian"].cpu().numpy().astype(np.int64) if v["sorted_gaussian"] is not None else np.zeros(0, np.int64)
    rng = v["ranges"].cpu().numpy().astype(np.int64)[:C].reshape(C * Tn, 2)
    L = rng[:, 1] - rng[:, 0]
    offs = np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)           # position in its (tile, chunk) list
    gid = sg[np.repeat(rng[:, 0], L) + offs]
    chunk = np.repeat(np.repeat(np.arange(C), Tn), L)
    head = np.zeros(P, bool)
    head[gid[(chunk == 0) & (offs < SEG)]] = True
    seen, not_seg, not_late = np.zeros(P, bool), np.zeros(P, bool), np.zeros(P, bool)
    seen[gid] = True
    not_seg[gid[offs < SEG]] = True
    not_late[gid[chunk == 0]] = True
    strata = {"chunk 0, some position < 128": head, "every position >= 128 (segment)": seen & ~not_seg,
              "every chunk >= 1 (chunk start)": seen & ~not_late}
    # per pixel: the last contributor's Gaussian and the cut-off flag
    lists, lens = _per_tile_lists(v, fr.plan, Tn)
    nc = _decode_n_contrib(v, lens, W, H)
    flat = np.concatenate(lists + [np.zeros(1, np.uint32)]).astype(np.int64)
    toff = np.concatenate([[0], np.cumsum([l.size for l in lists])])
    ys, xs = np.mgrid[0:H, 0:W]
    tile = (ys // 16) * Gx + xs // 16
    last_g = np.where(nc > 0, flat[np.minimum(toff[tile] + nc - 1, flat.size - 1)], -1)
    stopped = v["final_T"].cpu().numpy() < 0
    print(f"  HIP lists: {C} chunk(s) run of {fr.plan.num_chunks}; longest (tile, chunk) list {int(L.max(initial=0))}; "
          + "; ".join(f"{k}: {int(m.sum())}" for k, m in strata.items()))
    return strata, last_g, stopped


def _oracle_last_g(fr):
    ys, xs = np.mgrid[0:fr.H, 0:fr.W]
    tile = (ys // 16) * fr.Gx + xs // 16
    idx = fr.ranges[tile, 0] + fr.n_contrib - 1
    return np.where(fr.n_contrib > 0, fr.point_list[np.clip(idx, 0, max(fr.num_rendered - 1, 0))].astype(np.int64), -1)


def check_decisions(fr64, fr32, last_g, stopped, label):
    """Each pixel's last contributor and cut-off flag: on strict pixels >= 99.99 % equal to binary64's; on fragile pixels HIP differs
    from binary64 on at most 1.25 x as many pixels as the binary32 oracle does, + 1e-4 of the fragile pixels."""
    strict = fr64.fragile_px == 0
    d_hip = (last_g != _oracle_last_g(fr64)) | (stopped != fr64.stopped.astype(bool))
    d_32 = (_oracle_last_g(fr32) != _oracle_last_g(fr64)) | (fr32.stopped != fr64.stopped)
    n_frag = int((~strict).sum())
    print(f"  {label} decisions: strict pixels agreeing with binary64 {1 - d_hip[strict].mean():.6f} of {int(strict.sum())}; "
          f"fragile pixels differing: HIP {int(d_hip[~strict].sum())}, binary32 oracle {int(d_32[~strict].sum())} of {n_frag}")
    assert 1 - d_hip[strict].mean() >= 0.9999, (label, int(d_hip[strict].sum()))
    assert d_hip[~strict].sum() <= 1.25 * d_32[~strict].sum() + 1e-4 * n_frag, label


def _yardstick(fr32, want64, gm, names, parallel=True):
    b2f = fr32.backward(gm.astype(np.float32), parallel=parallel)
    f2b = fr32.backward(gm.astype(np.float32), parallel=parallel, order="front_to_back")
    return GC.yardstick(want64, b2f, f2b, names)


def per_gaussian_direct(kw, fr64, fr32, gimg, label, min_counts, frag_cap, exact_radii=True, parallel=True):
    """The standard API: forward, masked backward, both gradient checks (tensor-wide and per Gaussian), decisions."""
    state = {}

    def masked(color, radii):
        state["strict"] = _strict_pixels(fr64, radii, exact_radii)
        return np.where(state["strict"][None], gimg, 0.0).astype(np.float32)
    color, radii, grads = _run_gpu(kw, masked)
    _check_forward(kw, fr64, color, radii, exact_radii, fr32=fr32, frag_cap=frag_cap)
    gm = np.where(state["strict"][None], gimg, 0.0).astype(np.float64)
    want = fr64.backward(gm, parallel=parallel)
    names = [n for n in GRAD_NAMES if n in grads]
    live, strict_live = _check_grads(fr64, want, grads, names, masked=True)
    assert strict_live == live
    hip_strata, last_g, stopped = _hip_frame_views(kw)
    strata = GC.t_max_strata(fr64.T_max(), min_counts)
    strata.update({k: (m, int(min_counts.get(k, 0))) for k, m in hip_strata.items()})
    yard = _yardstick(fr32, want, gm, names, parallel)
    GC.check_grads_per_gaussian(want, yard, grads, strata, names, label=label)
    check_decisions(fr64, fr32, last_g, stopped, label)
    return live


def test_deep_small_frame_per_gaussian_direct_api():
    """The deep small frame (gradcheck.DEEP_SMALL: lists of up to ~950 entries, the cut-off taken in the third segment or later):
    >= 1 000 segment-checkpoint Gaussians, >= 100 with T_max < 1e-2.  Then the un-masked gradient image, as the fixtures have it:
    the strict bound outside oracle fragile_g, the one-flip bound inside."""
    kw = GC.deep_small_kwargs()
    c = GC.DEEP_SMALL
    fr64 = oracle.rasterize(dtype=np.float64, parallel=True, **kw)
    fr32 = oracle.rasterize(dtype=np.float32, parallel=True, **kw)
    gimg = S.make_grad_image(c["W"], c["H"], c["seed"]).numpy()
    mins = {"every position >= 128 (segment)": 1000, "chunk 0, some position < 128": 1000,
            "T_max in [1e-3, 1e-2)": 100, "T_max in [1e-2, 1e-1)": 1000, "T_max in [1e-1, 1]": 1000}
    live = per_gaussian_direct(kw, fr64, fr32, gimg, "deep small frame", mins, fragile_cap(0.0034), exact_radii=False)
    assert live > 100_000
    color, radii, grads = _run_gpu(kw, gimg)
    want = fr64.backward(gimg.astype(np.float64), parallel=True)
    _check_grads(fr64, want, grads, [n for n in GRAD_NAMES if n in grads])


def test_deep_small_frame_per_gaussian_timed_path():
    """The same frame through the path bench.py times (raw leaves, test_gpu_timed_path): per-Gaussian check on every raw leaf, T_max
    strata and HIP's list strata (the lists of the activated parameters through the standard API)."""
    from test_gpu_timed_path import RAW_NAMES, _oracle_raw, _render_timed_path
    scene, cam = GC.deep_small_scene()
    c = GC.DEEP_SMALL
    fr = _oracle_raw(scene, cam)
    fr32 = _oracle_raw(scene, cam, dtype=np.float32)
    gimg = S.make_grad_image(c["W"], c["H"], c["seed"]).numpy()
    state = {}

    def masked(color, radii):
        state["strict"] = _strict_pixels(fr, radii, exact_radii=False)
        return np.where(state["strict"][None], gimg, 0.0).astype(np.float32)
    color, radii, grads = _render_timed_path(scene, cam, (0.0, 0.0, 0.0), masked)
    _check_forward(None, fr, color, radii, exact_radii=False, fr32=fr32, frag_cap=fragile_cap(0.0034))
    gm = np.where(state["strict"][None], gimg, 0.0)
    want = fr.backward(gm.astype(np.float64), parallel=True)
    live, strict_live = _check_grads(fr, want, grads, list(RAW_NAMES), masked=True)
    assert strict_live == live and live > 100_000
    hip_strata, _, _ = _hip_frame_views(raster_kwargs(scene, cam))
    strata = GC.t_max_strata(fr.T_max(), {"T_max in [1e-3, 1e-2)": 100})
    strata.update({k: (m, 1000 if "segment" in k else 0) for k, m in hip_strata.items()})
    yard = _yardstick(fr32, want, gm, list(RAW_NAMES))
    GC.check_grads_per_gaussian(want, yard, grads, strata, list(RAW_NAMES), label="deep small frame [timed path]")


def test_uncovered_half_frame_chunk_start_stratum():
    """The frame of test_gpu_parity.test_frame_with_an_uncovered_region_...: every planned chunk runs, so >= 100 Gaussians are reached
    only from a chunk-start checkpoint."""
    W, H, P = 480, 320, 260_000
    scene = S.make_scene(P, W, H, 1, 91, scale_lo=0.01, scale_hi=0.07)
    scene.means3D[:, 1] = -scene.means3D[:, 1].abs() - 0.02 * scene.means3D[:, 2]
    kw = raster_kwargs(scene, S.make_camera(W, H))
    fr64 = oracle.rasterize(dtype=np.float64, parallel=True, **kw)
    fr32 = oracle.rasterize(dtype=np.float32, parallel=True, **kw)
    gimg = S.make_grad_image(W, H, 4).numpy()
    live = per_gaussian_direct(kw, fr64, fr32, gimg, "uncovered half", {"every chunk >= 1 (chunk start)": 100}, fragile_cap(0.0098))
    assert live > 1000
