"""The depth selection's chunk plan (csrc/gsr_select.hip) against the exact host reference (tests/select_ref.py).

Each case runs gsr_forward_preprocess only (no render, no binning workspace), reads the rule's per-Gaussian inputs back from the
geometry workspace - depth keys, tiles touched, fixed-point optical mass - and holds every plan field the host receives, and the
partition behind it, to the reference built from those integers: exact equality, nothing else.  The cases of select_ref.CASES
each target one coverage cell and must reach it on the device's own integers; random frames, a frame of more than one partition
round per block, a slab, a reused workspace, the plan read back both ways (pinned mirror with an image workspace, copy without),
the full forward's chunk sort and the gradient exchange's gather complete the set.
"""
import math
import os

import numpy as np
import pytest
import torch

import binning_ref as BR
import scene_synth as S
import select_ref as SR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


class Frame:
    """Device inputs of one frame and what gsr_forward_preprocess needs to run on them."""

    def __init__(self, W, H, means, scales, opacities, tile_rows=None, rotations=None):
        from diff_gaussian_rasterization import _native as N
        P = means.shape[0]
        self.W, self.H, self.P, self.tile_rows = W, H, P, tile_rows
        cam = S.make_camera(W, H)
        t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().to(DEV)
        self.means, self.scales, self.opacities = t(means), t(scales), t(opacities).reshape(P, 1)
        self.rotations = t(rotations) if rotations is not None else t(np.tile(np.float32([1, 0, 0, 0]), (P, 1)))
        self.shs = torch.zeros(P, 1, 3, device=DEV)
        self.tanfovx, self.tanfovy = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        self.bg = torch.zeros(3, device=DEV)
        self.view, self.proj, self.campos = (x.contiguous().to(DEV) for x in (cam.world_view_transform, cam.full_proj_transform,
                                                                             cam.camera_center))
        self.desc = N.make_desc(P, 0, 1, W, H, self.tanfovx, self.tanfovy, 1.0, False, False, tile_rows)
        self.cam = N.Camera(N._ptr(self.bg), N._ptr(self.view), N._ptr(self.proj), N._ptr(self.campos))
        self.gauss = N.Gaussians(N._ptr(self.means), N._ptr(self.shs), None, N._ptr(self.opacities), N._ptr(self.scales),
                                 N._ptr(self.rotations), None, None, 0)
        self.slab_px = SR.slab_pixels(W, H, tile_rows)

    def workspaces(self, with_image):
        from diff_gaussian_rasterization import _native as N
        geom_bytes, image_bytes = N.workspace_sizes(self.desc)
        return (torch.empty(geom_bytes, dtype=torch.uint8, device=DEV),
                torch.empty(image_bytes, dtype=torch.uint8, device=DEV) if with_image else None)


def case_frame(name):
    """A case of select_ref.CASES as a scene: isotropic splats on the optical axis at depth z, sigma = 2 max(W, H) pixels."""
    c = SR.CASES[name]
    z = np.asarray(c["z"](), np.float32)
    W, H = c["W"], c["H"]
    means = np.zeros((z.size, 3), np.float32)
    means[:, 2] = z
    focal = H / (2 * 0.5)
    scales = np.repeat((np.float32(2 * max(W, H) / focal) * z)[:, None], 3, 1)
    return Frame(W, H, means, scales, np.full(z.size, c["opacity"], np.float32), c.get("tile_rows"))


def random_frame(P, W, H, seed, sigma_lo=0.5, sigma_hi=80.0, behind=0.05):
    """Log-uniform depth over 0.21 .. 1e4, random positions, sizes (in pixels), orientations and opacities; a few behind the camera."""
    g = np.random.default_rng(seed)
    z = np.exp(g.uniform(np.log(0.21), np.log(1e4), P)).astype(np.float32)
    tanx = 0.5 * W / H
    means = np.stack([g.uniform(-1.1, 1.1, P) * tanx * z, g.uniform(-1.1, 1.1, P) * 0.5 * z, z], 1).astype(np.float32)
    means[g.random(P) < behind, 2] *= -1
    focal = H / (2 * 0.5)
    sigma = np.exp(g.uniform(np.log(sigma_lo), np.log(sigma_hi), (P, 3)))
    scales = (sigma * z[:, None] / focal).astype(np.float32)
    rot = g.normal(size=(P, 4)).astype(np.float32)
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    return Frame(W, H, means, scales, g.uniform(0.002, 1.0, P).astype(np.float32), rotations=rot)


def preprocess(fr, geom=None, image=None, with_image=False):
    """gsr_forward_preprocess on fresh (or the given) workspaces; the host's plan and the device's integers as numpy."""
    from diff_gaussian_rasterization import _native as N
    if geom is None:
        geom, image = fr.workspaces(with_image)
    radii = torch.empty(fr.P, dtype=torch.int32, device=DEV)
    plan = N.forward_preprocess(fr.desc, fr.cam, fr.gauss, geom, radii, torch.device(DEV), image_ws=image)
    torch.cuda.synchronize()
    keys, order = N.frame_arrays(fr.desc, geom)
    v = N.debug_views(fr.desc, geom, None, None, plan)
    u32 = lambda t: t.contiguous().cpu().numpy().view(np.uint32)
    return dict(plan=plan, geom=geom, keys=u32(keys), order=u32(order).astype(np.int64), tiles=u32(v["tiles_touched"]),
                mass=u32(v["optical_mass"]), radii=radii.cpu().numpy())


def plan_fields(plan):
    return dict(V=int(plan.num_visible), R=int(plan.num_rendered), num_chunks=int(plan.num_chunks),
                key_end=[int(x) for x in plan.chunk_key_end], rank_begin=[int(x) for x in plan.chunk_rank_begin],
                instances_max=[int(x) for x in plan.chunk_instances_max], key_max=int(plan.key_max))


def assert_plan(out, slab_px, label):
    """Every plan field and the partition equal the reference built from the device's own keys, tiles and masses."""
    ref = SR.plan_ref(out["keys"], out["tiles"], out["mass"], slab_px)
    got = plan_fields(out["plan"])
    print(f"{label}: V={got['V']} R={got['R']} chunks={got['num_chunks']} rank_begin={got['rank_begin']} "
          f"key_end={[hex(k) for k in got['key_end']]} instances_max={got['instances_max']} key_max={got['key_max']:#x} "
          f"cells={sorted(ref['cells'])}")
    for f in ("V", "R", "num_chunks", "rank_begin", "key_end", "instances_max"):
        assert got[f] == ref[f], (label, f, got[f], ref[f])
    if ref["V"]:                                    # (no bin is occupied in an empty frame: key_max bounds nothing there)
        assert got["key_max"] == ref["key_max"], (label, hex(got["key_max"]), hex(ref["key_max"]))
    assert sum(got["instances_max"]) == got["R"], label
    assert int((out["radii"] > 0).sum()) == ref["V"] and np.array_equal(out["radii"] > 0, out["keys"] != SR.INVISIBLE), label
    want = SR.partition_ref(out["keys"], ref["key_end"], ref["num_chunks"])
    assert np.array_equal(out["order"][:ref["V"]], want), (label, "depth_order")
    return ref


def both_ways(fr, label):
    """The frame with image_ws = None (plan read by copy) and with an image workspace (pinned mirror): identical, both exact."""
    a = preprocess(fr, with_image=False)
    ref = assert_plan(a, fr.slab_px, label + " [copy]")
    b = preprocess(fr, with_image=True)
    assert_plan(b, fr.slab_px, label + " [mirror]")
    assert plan_fields(a["plan"]) == plan_fields(b["plan"]), label
    for f in ("keys", "tiles", "mass"):
        assert np.array_equal(a[f], b[f]), (label, f)
    return a, ref


@pytest.mark.parametrize("case", sorted(SR.CASES))
def test_cell_case_matches_the_reference(case):
    fr = case_frame(case)
    out, ref = both_ways(fr, case)
    c = SR.CASES[case]
    assert {c["cell"], *c.get("also", ())} <= ref["cells"], (case, sorted(ref["cells"]))
    if case != "V0":                                # wider than the screen: every splat takes the slab's tiles
        Gx, Gy = (fr.W + 15) // 16, (fr.H + 15) // 16
        rows = (c["tile_rows"][1] - c["tile_rows"][0]) if c.get("tile_rows") else Gy
        assert np.all(out["tiles"] == Gx * rows), case
    if case == "slab":                              # the mass target follows the slab's pixels, not the image's
        whole = SR.plan_ref(out["keys"], out["tiles"], out["mass"], SR.slab_pixels(fr.W, fr.H))
        assert whole["rank_begin"] != ref["rank_begin"]


@pytest.mark.parametrize("P", [1, 63, 513, 100_003])
@pytest.mark.parametrize("seed", [11, 12])
def test_random_frame_matches_the_reference(P, seed):
    both_ways(random_frame(P, 640, 400, seed * 1000 + P), f"random P={P} seed={seed}")


def test_more_than_one_partition_round_per_block():
    """P = 2 200 003 tiny splats: kSelBlocks blocks of 512 threads take more than four rounds each."""
    P = 2_200_003
    assert P > SR.K["sel_blocks"] * 512 * 4
    fr = random_frame(P, 64, 64, 77, sigma_lo=0.2, sigma_hi=1.5)
    out, ref = both_ways(fr, "P=2200003")
    assert ref["num_chunks"] >= 2


def test_workspace_reuse_leaves_nothing_behind():
    """One geometry and image workspace of fixed P and image size: chunks8, one-subbin, V0, a random frame.  Stale histograms,
    level-2 tables or per-block counters of the frame before would show in the plan or the partition."""
    c8 = case_frame("chunks8")
    W, H, P = c8.W, c8.H, c8.P
    geom, image = c8.workspaces(True)
    focal = H / (2 * 0.5)

    def planes(z, opacity):
        means = np.zeros((P, 3), np.float32)
        means[:, 2] = z
        return Frame(W, H, means, np.repeat((np.float32(2 * W / focal) * means[:, 2])[:, None], 3, 1), np.full(P, opacity, np.float32))
    one = planes(SR.f32_from_bits(np.uint32(0x40000000) + np.random.default_rng(21).integers(0, 300, P).astype(np.uint32)), 0.99)
    none = planes(np.full(P, 0.1, np.float32), 0.99)
    frames = [("chunks8", c8, "chunks8"), ("one-subbin", one, "one-subbin"), ("V0", none, "V0"),
              ("random", random_frame(P, W, H, 31, sigma_hi=400.0), None)]
    for label, fr, cell in frames:
        ref = assert_plan(preprocess(fr, geom, image), fr.slab_px, "reuse: " + label)
        assert cell is None or cell in ref["cells"], (label, sorted(ref["cells"]))
    # and the same geometry workspace without the image workspace (plan read by copy)
    for label, fr, _ in frames[:2]:
        assert_plan(preprocess(fr, geom, None), fr.slab_px, "reuse, copy: " + label)


def _full_forward(fr, label):
    """rasterize_forward of the frame: the plan again, and the binned chunks strictly in (key, index) order."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import GaussianRasterizationSettings
    from diff_gaussian_rasterization import _native as N
    rs = GaussianRasterizationSettings(image_height=fr.H, image_width=fr.W, tanfovx=fr.tanfovx, tanfovy=fr.tanfovy, bg=fr.bg,
                                       scale_modifier=1.0, viewmatrix=fr.view, projmatrix=fr.proj, sh_degree=0, campos=fr.campos,
                                       prefiltered=False, debug=False)
    _, radii, f = dgr.rasterize_forward(fr.means, fr.shs, None, fr.opacities, fr.scales, fr.rotations, None, rs)
    torch.cuda.synchronize()
    plan = f.plan
    v = N.debug_views(f.desc, f.geom_ws, f.binning_ws, f.image_ws, plan)
    keys, _ = N.frame_arrays(f.desc, f.geom_ws)
    u32 = lambda t: t.contiguous().cpu().numpy().view(np.uint32)
    keys, tiles, mass = u32(keys), u32(v["tiles_touched"]), u32(v["optical_mass"])
    ref = SR.plan_ref(keys, tiles, mass, fr.slab_px)
    got = plan_fields(plan)
    assert plan.chunks_filtered == 0, label         # (no chunk was merged or filtered: the plan is still the planned one)
    for k in ("V", "R", "num_chunks", "rank_begin", "key_end", "instances_max", "key_max"):
        assert got[k] == ref[k], (label, k, got[k], ref[k])
    order = u32(v["depth_order"]).astype(np.int64)
    n, run = ref["num_chunks"], int(plan.chunks_run)
    print(f"{label}: chunks {n}, run {run}, chunk sizes {np.diff(ref['rank_begin'][:n + 1]).tolist()}")
    BR.check_depth_order(v["splat_records"].cpu().numpy(), order, ref["rank_begin"][:n + 1], ref["key_end"][:n], run, 0, ref["V"])
    # the chunks that ran are the head of the stable full sort, the others still in index order
    vis = np.nonzero(keys != SR.INVISIBLE)[0]
    full = vis[np.lexsort((vis, keys[vis]))]
    done = ref["rank_begin"][run]
    assert np.array_equal(order[:done], full[:done]), label
    assert np.array_equal(order[done:ref["V"]], SR.partition_ref(keys, ref["key_end"], n)[done:]), label
    return order[:ref["V"]].copy(), ref, run


# the frame closes after chunk 0 (opaque splats over every pixel); chunk 0 holds one key code (one-subbin's 300 codes crowd one
# bucket of the LDS sort: its fallback), 13 200 Gaussians (the 16 384-key LDS sort), more than 16 384 (the library's radix sort)
FORWARD_CASES = ["one-subbin", "bin-edge", "subbin-edge", "tile-bound", "empty-merged", "P1"]


@pytest.mark.parametrize("case", FORWARD_CASES)
def test_full_forward_sorts_the_planned_chunks(case):
    fr = case_frame(case)
    order, ref, run = _full_forward(fr, case)
    assert run == 1                                 # opaque and wider than the screen: every tile closes behind chunk 0
    if case in ("one-subbin", "bin-edge"):          # the LDS sort's chunks; its radix fallback, forced, gives the same order
        assert ref["rank_begin"][1] <= 16384
        os.environ["GSR_SORT_FORCE_RADIX"] = "1"
        try:
            twin, _, _ = _full_forward(fr, case + " (GSR_SORT_FORCE_RADIX)")
        finally:
            del os.environ["GSR_SORT_FORCE_RADIX"]
        assert np.array_equal(order, twin)
    elif case in ("subbin-edge", "tile-bound"):
        assert ref["rank_begin"][1] > 16384


@pytest.mark.parametrize("case", ["subbin-edge", "bin-edge"])
def test_exchange_rows_gather_takes_the_chunks_up_to_a_key_end(case):
    """gsr_exchange_rows_gather with key_max = chunk_key_end[c], n_rows = chunk_rank_begin[c + 1]: the sorted indices of chunks 0 .. c
    and their rows, nothing else."""
    from diff_gaussian_rasterization import _native as N
    fr = case_frame(case)
    out = preprocess(fr)
    ref = assert_plan(out, fr.slab_px, case)
    assert ref["num_chunks"] == 2
    screen = torch.randn(fr.P, N.SCREEN_GRAD_STRIDE, generator=torch.Generator().manual_seed(5)).to(DEV)
    order = SR.partition_ref(out["keys"], ref["key_end"], ref["num_chunks"])
    for c in range(ref["num_chunks"]):
        n = ref["rank_begin"][c + 1]
        rows, packed = N.exchange_rows_gather(fr.desc, out["geom"], ref["key_end"][c], screen, n)
        torch.cuda.synchronize()
        want = torch.as_tensor(np.sort(order[:n]), dtype=torch.int64)
        assert torch.equal(rows.cpu().long(), want), (case, c)
        assert torch.equal(packed.cpu(), screen.cpu()[want]), (case, c)
