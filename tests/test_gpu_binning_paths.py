"""Every binning and tile-sort path against the exact host reference (tests/binning_ref.py).

launch_chunk_binning (csrc/gsr_binning.hip) picks a path per depth chunk: flat (k_bin_chunk + radix sort, quadrant_mask_q) or a
team of 1, 4 or 16 waves (k_count_team + k_emit_team + radix sort, quadrant_mask_bbox), or the gather (k_count_team<W, true>,
k_tile_ranges with the rank scan fused up to 16384 Gaussians, k_tile_gather); a sort of n_max >= 4 Mi instances carries the
Gaussian word through the radix passes (gid_emit depends on the pass count's parity).  Chunks may go through the live filter and
be merged (csrc/gsr_api.hip).  Each frame below is rendered once; binning_ref.chunk_cells names every chunk's path, the library's
own launch counts (profile_read) confirm it, and the device's ranges, lists and quadrant bits are compared with the reference
built from the device's own records.  Together the frames must reach every cell in REQUIRED.  The experiment switches
GSR_NO_GATHER, GSR_NO_LIVE_FILTER and GSR_NO_CHUNK_MERGE are read once per process: those runs are child processes.
"""
import json
import math
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

import binning_ref as BR
import scene_synth as S
from util import raster_kwargs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))

# cells the frames must reach together (binning_ref.cell_names); "sort-gather-table": a sort below 4 Mi instances whose Gaussian
# words are gathered behind it (k_ranges<true>)
# (team chunks emit + sort only where they cannot gather: the GSR_NO_GATHER child asserts that path)
REQUIRED = {"flat", "team1", "team4", "team16", "sort", "gather-fused", "gather-unfused", "flat/sort", "sort-gather-table",
            "carry-1pass", "carry-2pass", "carry-3pass", "filtered", "merged", "slab"}


def _faint_scene(P, W, H, seed, sigma_px, opacity):
    """Splats of a fixed pixel size and opacity spread over the frustum: faint ones never saturate the frame, so the whole scene
    is one depth chunk and its instance count is set by P."""
    sc = S.make_scene(P, W, H, 0, seed, zmin=2.0, zmax=6.0)
    z = sc.means3D[:, 2:3]
    focal = H / (2 * 0.5)
    sc.log_scales = torch.log(sigma_px * z / focal).expand(P, 3).contiguous()
    sc.opacity_logits = torch.full((P, 1), math.log(opacity / (1 - opacity)))
    return sc


def _frame(name):
    """(scene, camera, tile_rows) of each frame."""
    if name == "p20k_320x200":
        return S.make_scene(20000, 320, 200, 3, 201, scale_lo=0.005, scale_hi=0.06), S.make_camera(320, 200), None
    if name == "team16":
        return S.make_scene(300, 1280, 720, 1, 301, scale_lo=0.5, scale_hi=2.0), S.make_camera(1280, 720), None
    if name == "team4":
        return S.make_scene(300, 1280, 720, 1, 301, scale_lo=0.08, scale_hi=0.3), S.make_camera(1280, 720), None
    if name == "wide_faint":            # 20 000 Gaussians of ~200 tiles each: a gather chunk above the fused scan's 16384
        return _faint_scene(20000, 1280, 720, 7, 70.0, 0.02), S.make_camera(1280, 720), None
    if name == "uncovered":             # the lower half stays uncovered: late chunks are filtered and merged
        sc = S.make_scene(260_000, 480, 320, 1, 91, scale_lo=0.01, scale_hi=0.07)
        sc.means3D[:, 1] = -sc.means3D[:, 1].abs() - 0.02 * sc.means3D[:, 2]
        return sc, S.make_camera(480, 320), None
    if name == "slab":
        return S.make_scene(5000, 256, 192, 3, 109, scale_lo=0.005, scale_hi=0.06), S.make_camera(256, 192), (3, 9)
    if name == "carry_1pass":           # 240 tiles (1 radix pass), one chunk of >= 4 Mi instances
        return _faint_scene(3_500_000, 256, 240, 11, 2.0, 0.012), S.make_camera(256, 240), None
    if name == "carry_3pass":           # 272 x 257 tiles (3 passes), one chunk of >= 4 Mi instances
        return _faint_scene(3_000_000, 4352, 4112, 12, 2.0, 0.012), S.make_camera(4352, 4112), None
    if name == "posed_edge":            # tests/posed.py: splats with far off-screen centres (clamped), near-plane giants, needles
        import posed as PO
        cam = PO.posed_camera(640, 360, "c", tanfovx=1.2 * 0.5 * 640 / 360)
        return PO.edge_scene(640, 360, cam, 122, 12000)[0], cam, None
    if name == "cfg5n":
        sc, cam = S.make_config("cfg5n")
        return sc, cam, None
    raise KeyError(name)


FRAMES = ["p20k_320x200", "team16", "team4", "wide_faint", "uncovered", "slab", "carry_1pass", "carry_3pass", "cfg5n", "posed_edge"]
# the frames whose paths an experiment switch changes
SWITCHED = {"GSR_NO_GATHER": ["team16", "team4", "wide_faint"], "GSR_NO_LIVE_FILTER": ["uncovered"],
            "GSR_NO_CHUNK_MERGE": ["uncovered"]}


def run_frame(name, hh):
    """Render one frame, check its lists against the reference; returns the per-frame report."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from diff_gaussian_rasterization import _native as N
    t0 = time.time()
    scene, cam, rows = _frame(name)
    kw = raster_kwargs(scene, cam, as_numpy=False)
    d = lambda t: t.to(DEV) if isinstance(t, torch.Tensor) else t
    rs = GaussianRasterizationSettings(image_height=kw["image_height"], image_width=kw["image_width"], tanfovx=kw["tanfovx"],
                                       tanfovy=kw["tanfovy"], bg=d(kw["bg"]), scale_modifier=1.0, viewmatrix=d(kw["viewmatrix"]),
                                       projmatrix=d(kw["projmatrix"]), sh_degree=kw["sh_degree"], campos=d(kw["campos"]),
                                       prefiltered=False, debug=False)
    args = (d(kw["means3D"]), d(kw["shs"]), None, d(kw["opacities"]), d(kw["scales"]), d(kw["rotations"]), None, rs)
    N.profile_enable(True)
    _, _, fr = dgr.rasterize_forward(*args, tile_rows=rows) if rows else dgr.rasterize_forward(*args)
    torch.cuda.synchronize()
    prof = N.profile_read()
    N.profile_enable(False)
    W, H = kw["image_width"], kw["image_height"]
    Gx, Gy = (W + 15) // 16, (H + 15) // 16
    ty0, ty1 = rows if rows else (0, Gy)
    plan = fr.plan
    v = N.debug_views(fr.desc, fr.geom_ws, fr.binning_ws, fr.image_ws, plan)
    cells = BR.chunk_cells(plan, Gx, Gy, ty0, ty1, no_gather="GSR_NO_GATHER" in os.environ)
    # (one readback per array)
    rec = v["splat_records"].cpu().numpy()
    order = v["depth_order"].cpu().numpy()
    words = (v["sorted_gaussian"] | (v["sorted_quadrants"] << 28)).cpu().numpy().view(np.uint32)
    ranges = v["ranges"][:plan.chunks_run].cpu().numpy().view(np.uint32)
    enc = v["n_contrib"].cpu().numpy()
    rb = [int(plan.chunk_rank_begin[c]) for c in range(plan.num_chunks + 1)]
    BR.check_depth_order(rec, order, rb, [int(plan.chunk_key_end[c]) for c in range(plan.num_chunks)], plan.chunks_run,
                         plan.chunks_filtered, plan.num_visible)
    last = BR.last_chunk_per_tile(enc, W, H)
    last[: ty0 * Gx] = -1
    last[ty1 * Gx:] = -1
    BR.reference(hh, Gx, Gy, ty0, ty1, rec, order, rb[:plan.chunks_run + 1], [c["bbox"] for c in cells])
    rep = BR.check(hh, ranges, words, ty0 * Gx, ty1 * Gx, last)
    n_gather = sum(c["build"] != "sort" for c in cells)
    n_sort = len(cells) - n_gather
    launches = {k: prof.get(k, (0.0, 0))[1] for k in ("tile_gather", "emit", "tile_sort")}
    rep.update(frame=name, cells=cells, launches=launches, n_gather=n_gather, n_sort=n_sort, seconds=round(time.time() - t0, 1),
               names=sorted(set().union(*[BR.cell_names(c, rows is not None) for c in cells])))
    return rep


def _summary(rep):
    cs = "; ".join(f"c{c['c']} n={c['n']} n_max={c['n_max']} {c['path']}/{c['build']}"
                   + (f" carry {c['passes']}p" if c["carry"] else "") + (" filtered" if c["filtered"] else "")
                   + (" merged" if c["merged"] else "") for c in rep["cells"])
    return (f"{rep['frame']}: [{cs}] | compared {rep['compared']}, boundary {rep['boundary_in']}+{rep['boundary_quad']} "
            f"(max margin {rep['max_margin']:.2e}), closed tiles {rep['closed_tiles']}, launches {rep['launches']}, {rep['seconds']} s")


def _assert_frame(rep):
    BR.assert_clean(rep, rep["frame"])
    assert rep["compared"] > 0
    L = rep["launches"]
    # the mirror names the path the library took: gather chunks launch k_tile_gather, the others emit + tile sort
    assert (L["tile_gather"] > 0) == (rep["n_gather"] > 0) and L["tile_gather"] >= rep["n_gather"], rep["launches"]
    assert (L["emit"] > 0) == (rep["n_sort"] > 0) and L["emit"] >= rep["n_sort"] and L["tile_sort"] >= rep["n_sort"], rep["launches"]


def _main(names, out):
    hh = BR.build_harness(os.path.dirname(out))
    reps = []
    for n in names:
        rep = run_frame(n, hh)
        print(_summary(rep), flush=True)
        reps.append(rep)
    with open(out, "w") as f:
        json.dump(reps, f)


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    return BR.build_harness(str(tmp_path_factory.mktemp("hh_bin")))


def test_every_binning_path_matches_the_reference(hh):
    reached = set()
    for name in FRAMES:
        rep = run_frame(name, hh)
        print(_summary(rep))
        _assert_frame(rep)
        reached |= set(rep["names"])
    print("cells reached:", sorted(reached))
    assert REQUIRED <= reached, f"cells no frame reaches: {sorted(REQUIRED - reached)}"


@pytest.mark.parametrize("switch", sorted(SWITCHED))
def test_experiment_switches_take_paths_that_match_the_reference(switch, tmp_path):
    """Each switch is read once per process: a fresh child process per switch, with its own time limit."""
    out = str(tmp_path / "reps.json")
    env = dict(os.environ, **{switch: "1"})
    code = f"import sys; sys.path[:0] = {[HERE, os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), 'structured-gaussian-splatting_amd')]!r}; " \
           f"import test_gpu_binning_paths as T; T._main({SWITCHED[switch]!r}, {out!r})"
    p = subprocess.run([sys.executable, "-c", code], env=env, timeout=300, capture_output=True, text=True)
    print(p.stdout[-4000:])
    assert p.returncode == 0, p.stderr[-4000:]
    reps = json.load(open(out))
    for rep in reps:
        _assert_frame(rep)
        if switch == "GSR_NO_GATHER":
            assert rep["n_gather"] == 0 and any(c["path"].startswith("team") for c in rep["cells"])
        if switch == "GSR_NO_LIVE_FILTER":
            assert not any(c["filtered"] for c in rep["cells"])
        if switch == "GSR_NO_CHUNK_MERGE":
            assert not any(c["merged"] for c in rep["cells"])


@pytest.mark.parametrize("n,n_max,base,end_bit,payload,even", [
    (4_194_303, 4_194_303, 0, 13, True, False), (4_194_304, 4_194_304, 0, 13, True, False), (9_000_000, 9_000_000, 3, 17, True, False),
    (0, 5_000_000, 1, 8, True, False), (1, 5_000_000, 7, 13, True, False), (1000, 5_000_000, 12345, 17, True, False),
    (1_000_000, 1_000_000, 5, 8, True, True), (5_000_000, 5_000_000, 0, 17, True, True), (300_000, 300_000, 9, 13, False, True),
    (70_000, 4_194_304, 1, 8, True, False)])
def test_sort_as_the_frame_calls_it(n, n_max, base, end_bit, payload, even):
    """gsr_debug_sort_pairs_ex against torch.sort(stable=True): count and base on the device, n_max on both sides of the
    4 Mi switch to the LDS-reordering scatter and far above the count, 1 to 3 passes, a second payload, even_passes."""
    from diff_gaussian_rasterization import _native as N
    g = torch.Generator(device="cpu").manual_seed(n + end_bit + base)
    keys = torch.randint(0, 1 << end_bit, (n,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)
    if n > 10:                        # long runs of equal keys: stability matters
        keys[: n // 3] = keys[0]
        keys[n // 2: n // 2 + n // 8] = keys[n // 2]
    vals = torch.arange(n, dtype=torch.int32, device=DEV)
    v2 = (torch.randint(0, 1 << 30, (n,), generator=g, dtype=torch.int64).to(torch.int32).to(DEV)) if payload else None
    ks, vs, v2s, res = N.debug_sort_pairs_ex(keys, vals, end_bit, n_max, base, v2, even)
    torch.cuda.synchronize()
    passes = (end_bit + 7) // 8
    assert res == (0 if even else passes & 1)
    want_k, order = torch.sort(keys.long(), stable=True)
    assert torch.equal(ks.long(), want_k)
    assert torch.equal(vs.long(), order)
    if payload:
        assert torch.equal(v2s, v2[order])
