"""Per-Gaussian gradient check: every Gaussian's gradient held to ITS OWN scale, against what binary32 arithmetic reaches.

The tensor-wide bound of test_gpu_parity._check_grads (|err| <= 1e-4 max|want| + 1e-4 |want|) is relative to the tensor's
largest element, so the smaller a Gaussian's gradient, the looser the check on it -- and the Gaussians with small gradients
are the ones that blend behind low transmittance, reached by the HIP backward from a checkpoint (a segment start every 128
list entries, or a chunk start).  An error that scales with the transmittance in front of a splat passes that bound.

Here, per Gaussian g and leaf:   e(g) = max_k |got - want| / max_k |want|   (want: the binary64 oracle), and the yardstick
yard32(g) is the larger of the same error for the two binary32 oracles (back to front as A.9 has it, and front to back in the
HIP backward's algebra).  Per stratum (a set of Gaussians) and leaf:
  * the 50th and 99th percentiles of e are at most Q_FACTOR x those of yard32, + Q_ADD;
  * every Gaussian has e(g) <= G_FACTOR x max(yard32(g), median yard32 of the stratum);
  * the stratum holds at least its minimum count of Gaussians (a check on an empty stratum passes nothing).
"""
from __future__ import annotations

import numpy as np

Q_FACTOR = 4.0
Q_ADD = 1e-6
G_FACTOR = 512.0           # measured worst single Gaussian on an MI355X: 142 (tests/test_gpu_per_gaussian.py)

T_STRATA = (("T_max in [1e-1, 1]", 1e-1, np.inf), ("T_max in [1e-2, 1e-1)", 1e-2, 1e-1),
            ("T_max in [1e-3, 1e-2)", 1e-3, 1e-2), ("T_max in [1e-4, 1e-3)", 1e-4, 1e-3))


# The deep small frame: the cfg3n recipe (zmin = 2, seed 3, SH 3) at 320 x 192 with 120 000 Gaussians of scales 0.003 .. 0.03 --
# lists of up to ~950 entries (mean 820 composited per pixel), the blend reaches the 1e-4 cut-off on 3.5 % of the pixels, all of
# them in the third list segment or later, and every T_max stratum holds more than 100 Gaussians.
DEEP_SMALL = dict(P=120_000, W=320, H=192, D=3, seed=3, zmin=2.0, scale_lo=0.003, scale_hi=0.03)


def deep_small_scene():
    import scene_synth as S
    c = DEEP_SMALL
    return (S.make_scene(c["P"], c["W"], c["H"], c["D"], c["seed"], scale_lo=c["scale_lo"], scale_hi=c["scale_hi"], zmin=c["zmin"]),
            S.make_camera(c["W"], c["H"]))


def deep_small_kwargs():
    from util import raster_kwargs
    return raster_kwargs(*deep_small_scene())


def oracle_min_position(fr) -> np.ndarray:
    """[P]: the smallest position of any of a Gaussian's instances in its tile's list (oracle lists; a large value: none)."""
    out = np.full(fr.P, np.iinfo(np.int64).max, np.int64)
    if fr.num_rendered:
        np.minimum.at(out, fr.point_list.astype(np.int64), fr.inst_position())
    return out


def per_gaussian_error(want: dict, got: dict, names) -> dict:
    """{leaf: e[P]} with e(g) = max_k |got - want| / max_k |want|; NaN where the Gaussian has no gradient on that leaf."""
    out = {}
    for n in names:
        w = np.asarray(want[n], np.float64)
        P = w.shape[0]
        w = w.reshape(P, -1)
        g = np.asarray(got[n], np.float64).reshape(P, -1)
        s = np.abs(w).max(1, initial=0.0)
        err = np.abs(g - w).max(1, initial=0.0)
        out[n] = np.where(s > 0, err / np.where(s > 0, s, 1.0), np.nan)
    return out


def yardstick(want64: dict, b2f32: dict, f2b32: dict, names) -> dict:
    """yard32(g) per leaf: the larger of the two binary32 oracles' per-Gaussian errors against binary64."""
    a, b = per_gaussian_error(want64, b2f32, names), per_gaussian_error(want64, f2b32, names)
    return {n: np.fmax(a[n], b[n]) for n in names}


def t_max_strata(T_max: np.ndarray, min_count: dict | None = None) -> dict:
    """Strata by the largest transmittance in front of a Gaussian (oracle T_max): {label: (mask, min_count)}."""
    min_count = min_count or {}
    return {lab: ((T_max >= lo) & (T_max < hi), int(min_count.get(lab, 0))) for lab, lo, hi in T_STRATA}


def check_grads_per_gaussian(want64: dict, yard32: dict, got: dict, strata: dict, names=None, label: str = "",
                             q_factor: float = Q_FACTOR, q_add: float = Q_ADD, g_factor: float = G_FACTOR,
                             raise_on_fail: bool = True) -> list:
    """strata: {label: (bool mask [P], minimum count)}.  Prints one line per stratum and leaf (count, e and yard32 quantiles);
    returns the list of failures (strings), and raises AssertionError on the first report when raise_on_fail."""
    names = list(names if names is not None else yard32.keys())
    e = per_gaussian_error(want64, got, names)
    failures = []
    for slab, (mask, min_count) in strata.items():
        for n in names:
            m = mask & np.isfinite(e[n]) & np.isfinite(yard32[n])
            cnt = int(m.sum())
            if cnt < min_count:
                failures.append(f"{label} {slab} {n}: {cnt} Gaussians < {min_count}")
                continue
            if cnt == 0:
                continue
            eg, yg = e[n][m], yard32[n][m]
            qe, qy = np.quantile(eg, [0.5, 0.99]), np.quantile(yg, [0.5, 0.99])
            ratio = eg / np.maximum(yg, qy[0])
            print(f"  {label} {slab:24s} {n:10s} n={cnt:7d}  e p50 {qe[0]:.2e} p99 {qe[1]:.2e} max {eg.max():.2e} | "
                  f"yard32 p50 {qy[0]:.2e} p99 {qy[1]:.2e} | worst e/max(yard, p50) {ratio.max():.2f}")
            for q, a, b in (("p50", qe[0], qy[0]), ("p99", qe[1], qy[1])):
                if a > q_factor * b + q_add:
                    failures.append(f"{label} {slab} {n}: {q} {a:.3e} > {q_factor:g} x yard32 {q} {b:.3e} + {q_add:g}")
            if ratio.max() > g_factor:
                k = int(np.argmax(ratio))
                failures.append(f"{label} {slab} {n}: {int((ratio > g_factor).sum())} Gaussians beyond {g_factor:g} x max(yard32, "
                                f"stratum median); worst {ratio[k]:.1f} (e {eg[k]:.3e}, yard32 {yg[k]:.3e})")
    if failures and raise_on_fail:
        raise AssertionError("; ".join(failures[:6]))
    return failures

