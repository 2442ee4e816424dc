"""CPU self-tests of the binning reference and its checker (tests/binning_ref.py, tests/host_harness.cpp).

The reference, run on records from hh_preprocess, must agree with the binary32 oracle: every list is a subsequence of the
oracle's per-tile list and holds every Gaussian that some pixel of the tile accepts.  The checker must name each fault planted
into lists that are otherwise exactly the reference's (host only: no mutated kernels)."""
import numpy as np
import pytest

import binning_ref as BR
import oracle
import scene_synth as S
from test_host_math import _run
from util import raster_kwargs

W, H = 128, 96


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    return BR.build_harness(str(tmp_path_factory.mktemp("hh_bin")))


@pytest.fixture(scope="module")
def frame(hh):
    scene = S.make_scene(3000, W, H, 1, 77, scale_lo=0.005, scale_hi=0.08)
    kw = raster_kwargs(scene, S.make_camera(W, H))
    got = _run(hh, kw)
    fr = oracle.rasterize(dtype=np.float32, **kw)
    rec = got["rec"]
    vis = np.nonzero(got["radii"] > 0)[0]
    keys = rec[vis, 9].view(np.uint32)
    order = vis[np.lexsort((vis, keys))].astype(np.int32)        # (key, index): the binned chunks' order
    half = order.size // 2
    return dict(rec=rec, order=order, rb=np.array([0, half, order.size], np.int32), fr=fr, Gx=(W + 15) // 16, Gy=(H + 15) // 16)


@pytest.mark.parametrize("bbox", [0, 1])
def test_reference_lists_agree_with_the_oracle(hh, frame, bbox):
    """One chunk of every visible Gaussian: each list is a subsequence of the oracle's (tile, depth)-sorted list, and every
    Gaussian that a pixel of the tile accepts (alpha >= 1/255, power <= 0, by the oracle's own conic in float64) is in it."""
    fr, Gx, Gy = frame["fr"], frame["Gx"], frame["Gy"]
    order = frame["order"]
    ref = BR.reference(hh, Gx, Gy, 0, Gy, frame["rec"], order, np.array([0, order.size], np.int32), [bbox])
    ys, xs = np.mgrid[0:16, 0:16]
    n_acc = n_list = 0
    for t in range(Gx * Gy):
        gid, quad, flags = BR.ref_list(ref, 0, t)
        want = fr.point_list[fr.ranges[t, 0]:fr.ranges[t, 1]].astype(np.int64)
        pos = {g: i for i, g in enumerate(want.tolist())}
        idx = [pos.get(int(g), -1) for g in gid]
        assert min(idx, default=0) >= 0 and np.all(np.diff(idx) > 0), f"tile {t}: not a subsequence of the oracle's list"
        px = (t % Gx) * 16 + xs.ravel().astype(np.float64)
        py = (t // Gx) * 16 + ys.ravel().astype(np.float64)
        g = want
        dx = fr.xy[g, 0:1].astype(np.float64) - px[None]
        dy = fr.xy[g, 1:2].astype(np.float64) - py[None]
        co = fr.conic_opacity[g].astype(np.float64)
        power = -0.5 * (co[:, 0:1] * dx * dx + co[:, 2:3] * dy * dy) - co[:, 1:2] * dx * dy
        alpha = np.minimum(0.99, co[:, 3:4] * np.exp(power))
        inside = (px[None] < W) & (py[None] < H)
        acc = ((power <= 0) & (alpha >= (1.0 / 255) * (1 + 1e-4)) & inside).any(1)
        missing = set(g[acc].tolist()) - set(gid.tolist())
        assert not missing, f"tile {t}: accepted Gaussians {sorted(missing)[:5]} not in the reference list"
        if bbox == 0:           # quadrant_mask_q keeps every quadrant with an accepting pixel
            for j, gg in enumerate(gid.tolist()):
                k = np.nonzero(g == gg)[0][0]
                qa = ((power[k] <= 0) & (alpha[k] >= (1.0 / 255) * (1 + 1e-4)) & inside[0])
                qk = (ys.ravel() >= 8) * 2 + (xs.ravel() >= 8)
                need = np.bitwise_or.reduce((1 << qk[qa]).astype(np.int64)) if qa.any() else 0
                assert (int(need) & ~int(quad[j])) == 0, (t, gg)
        n_acc += int(acc.sum()); n_list += gid.size
    assert n_acc > 1000 and n_list >= n_acc and n_list < fr.num_rendered
    print(f"reference: {n_list} instances, {n_acc} accepted by a pixel, oracle lists {fr.num_rendered}; "
          f"{int((ref['flags'] & 0x10).sum())} inclusion decisions within the tolerance")


def _device_like(ref, t_begin, t_end):
    """The lists a correct device emits: host-accepted entries, ranges back to back in tile order, chunk after chunk."""
    lists = []
    for c in range(ref["n_chunks"]):
        per = {}
        for t in range(t_begin, t_end):
            gid, quad, flags = BR.ref_list(ref, c, t)
            keep = (flags & 0x20) != 0
            per[t] = [int(g) | (int(q) << 28) for g, q in zip(gid[keep], quad[keep])]
        lists.append(per)
    return lists


def _serialise(lists, Tn):
    ranges = np.zeros((len(lists), Tn, 2), np.uint32)
    words = []
    for c, per in enumerate(lists):
        for t in sorted(per):
            ranges[c, t] = (len(words), len(words) + len(per[t]))
            words += per[t]
    return ranges, np.array(words, np.uint32)


def test_checker_passes_correct_lists_and_names_each_fault(hh, frame):
    Gx, Gy = frame["Gx"], frame["Gy"]
    Tn = Gx * Gy
    ref = BR.reference(hh, Gx, Gy, 0, Gy, frame["rec"], frame["order"], frame["rb"], [0, 1])
    base = _device_like(ref, 0, Tn)
    ranges, words = _serialise(base, Tn)
    rep = BR.check(hh, ranges, words, 0, Tn)
    BR.assert_clean(rep, "unmutated")
    assert rep["compared"] == words.size > 1000 and rep["closed_tiles"] == 0

    # a tile with at least 3 entries in chunk 1, and one of its Gaussians with a quadrant bit the reference is sure of
    t = next(t for t in range(Tn) if len(base[1][t]) >= 3)
    gid, quad, flags = BR.ref_list(ref, 1, t)
    keep = (flags & 0x20) != 0
    gid, quad, flags = gid[keep], quad[keep], flags[keep]
    j, bit = next((j, b) for j in range(gid.size) for b in range(4) if (quad[j] >> b) & 1 and not (flags[j] >> b) & 1)
    other = next(int(g) for g in frame["order"] if int(g) not in set(gid.tolist()))

    def mutated(fn):
        lists = [dict((k, list(v)) for k, v in per.items()) for per in base]
        fn(lists[1][t])
        return _serialise(lists, Tn)

    def swap(l):
        l[0], l[1] = l[1], l[0]

    def replace(l):
        l[1] = other | (l[1] & 0xF0000000)

    def clear_bit(l):
        l[j] &= ~(1 << (28 + bit))
    cases = {"drop": (lambda l: l.pop(1), "list"), "duplicate": (lambda l: l.insert(1, l[1]), "list"), "swap": (swap, "list"),
             "replace": (replace, "list"), "quadrant bit": (clear_bit, "quad")}
    for name, (fn, kind) in cases.items():
        r, w = mutated(fn)
        rep = BR.check(hh, r, w, 0, Tn)
        assert rep[kind] >= 1 and rep["first_fault"] == (kind, 1, t), (name, rep)
    # one range shifted by one: the ranges no longer tile the chunk's segment
    r = ranges.copy()
    r[1, t, 0] += 1
    rep = BR.check(hh, r, words, 0, Tn)
    assert rep["range"] >= 1 and rep["first_fault"][0] == "range", rep
    r = ranges.copy()
    r[1, t] += 1
    assert BR.check(hh, r, words, 0, Tn)["range"] >= 1

    # closed tiles: empty in chunk 1 is a closed tile, fine unless a pixel's last contributor lies in chunk 1 or later
    lists = [dict((k, list(v)) for k, v in per.items()) for per in base]
    lists[1][t] = []
    r, w = _serialise(lists, Tn)
    rep = BR.check(hh, r, w, 0, Tn)
    BR.assert_clean(rep, "closed")
    assert rep["closed_tiles"] == 1
    last = np.full(Tn, 0, np.int32)
    last[t] = 1
    assert BR.check(hh, r, w, 0, Tn, last)["closed"] == 1
    # ... chunk 0 has no closed tiles, and a closed tile never reopens
    t0 = next(t for t in range(Tn) if base[0][t] and base[1][t])
    lists = [dict((k, list(v)) for k, v in per.items()) for per in base]
    lists[0][t0] = []
    r, w = _serialise(lists, Tn)
    rep = BR.check(hh, r, w, 0, Tn)
    assert rep["closed"] >= 2 and rep["first_fault"] == ("closed", 0, t0), rep


def test_checker_allows_only_flagged_boundary_decisions(hh, frame):
    """An entry the reference flags as within the tolerance may be dropped or kept; one it is sure of may not."""
    Gx, Gy = frame["Gx"], frame["Gy"]
    Tn = Gx * Gy
    # a tolerance so wide that some decisions are flagged, then drop exactly those
    ref = BR.reference(hh, Gx, Gy, 0, Gy, frame["rec"], frame["order"], frame["rb"], [0, 0], tol=0.05)
    maybe = (ref["flags"] & 0x30) == 0x30
    assert maybe.sum() > 0
    lists = []
    for c in range(2):
        per = {}
        for t in range(Tn):
            gid, quad, flags = BR.ref_list(ref, c, t)
            keep = (flags & 0x20) != 0
            keep &= (flags & 0x10) == 0          # drop every flagged one
            per[t] = [int(g) | (int(q) << 28) for g, q in zip(gid[keep], quad[keep])]
        lists.append(per)
    r, w = _serialise(lists, Tn)
    rep = BR.check(hh, r, w, 0, Tn)
    assert rep["list"] == 0 and rep["boundary_in"] == int(maybe.sum()) and 0 < rep["max_margin"] <= 0.05
