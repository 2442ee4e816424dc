"""tests/select_ref.py held to a second formulation of the chunk rule, and the coverage cells of its cases (no GPU).

walk() applies both thresholds Gaussian by Gaussian along the sorted order, rounds each cut up to its aligned key edge and
assembles the chunks; select_ref.plan_ref works on whole aligned groups with prefix sums.  The two must agree on the integer
twins of every case tests/test_gpu_depth_select.py runs on the device, and on random arrays; every twin must reach the cell its
case was built for.
"""
import numpy as np
import pytest

import select_ref as SR


def walk(keys, tiles, mass, slab_px):
    """(num_chunks, key_end, rank_begin, instances_max) by a walk over the sorted order, in Python integers."""
    keys = [int(x) for x in np.asarray(keys, np.uint32)]
    vis = sorted((k, i) for i, k in enumerate(keys) if k != SR.INVISIBLE)
    ks = [k for k, _ in vis]
    ts = [int(tiles[i]) for _, i in vis]
    ms = [int(mass[i]) for _, i in vis]
    V, R = len(ks), sum(ts)
    chunks, begin, begin_tiles = [], 0, 0           # (key_end, end rank, tiles)
    for c in range(SR.MAX_CHUNKS - 1):
        if begin >= V or SR.tile_floor(c) >= R:
            break                                   # a chunk may not be smaller than the floor: it takes the rest
        T, F = SR.mass_target(slab_px, c), SR.tile_floor(c)
        run_t = run_m = 0
        cut = None
        for i in range(V):
            run_t += ts[i]; run_m += ms[i]
            if run_m > T and run_t > F:
                cut = i
                break
        if cut is None:
            break
        a = SR.align_bits(c)
        edge = min((ks[cut] | ((1 << a) - 1)), SR.SENTINEL)
        while cut + 1 < V and ks[cut + 1] <= edge:  # round the cut up to its edge
            cut += 1
            run_t += ts[cut]
        if cut + 1 <= begin:
            continue                                # two boundaries behind the same Gaussian: the empty chunk is dropped
        if cut + 1 >= V:
            break
        chunks.append((edge, cut + 1, run_t - begin_tiles))
        begin, begin_tiles = cut + 1, run_t
    if begin < V:
        chunks.append((SR.SENTINEL, V, R - begin_tiles))
    n = len(chunks)
    pad = SR.MAX_CHUNKS - n
    return (max(n, 1), [c[0] for c in chunks] + [SR.SENTINEL] * pad, [0] + [c[1] for c in chunks] + [V] * pad,
            [c[2] for c in chunks] + [0] * pad)


def _agree(keys, tiles, mass, slab_px):
    ref = SR.plan_ref(keys, tiles, mass, slab_px)
    n, key_end, rank_begin, inst = walk(keys, tiles, mass, slab_px)
    assert (ref["num_chunks"], ref["key_end"], ref["rank_begin"], ref["instances_max"]) == (n, key_end, rank_begin, inst)
    assert sum(ref["instances_max"]) == ref["R"] and ref["rank_begin"][ref["num_chunks"]] == ref["V"]
    return ref


@pytest.mark.parametrize("case", sorted(SR.CASES))
def test_case_twins_agree_and_reach_their_cell(case):
    keys, tiles, mass, px = SR.twin_arrays(case)
    ref = _agree(keys, tiles, mass, px)
    want = {SR.CASES[case]["cell"], *SR.CASES[case].get("also", ())}
    assert want <= ref["cells"], (case, sorted(ref["cells"]))
    # the partition: chunk after chunk, index order inside each, every visible Gaussian once, keys inside their chunk's span
    order = SR.partition_ref(keys, ref["key_end"], ref["num_chunks"])
    assert sorted(order.tolist()) == np.nonzero(keys != SR.INVISIBLE)[0].tolist()
    for c in range(ref["num_chunks"]):
        o = order[ref["rank_begin"][c]:ref["rank_begin"][c + 1]]
        assert np.all(np.diff(o) > 0)
        if o.size:
            assert keys[o].max() <= ref["key_end"][c] and (c == 0 or keys[o].min() > ref["key_end"][c - 1])


def test_the_cases_reach_every_cell():
    reached = set()
    for case in SR.CASES:
        reached |= SR.plan_ref(*SR.twin_arrays(case))["cells"]
    assert set(SR.CELLS) <= reached, sorted(set(SR.CELLS) - reached)


def test_slab_twin_depends_on_the_slab_pixels():
    keys, tiles, mass, px = SR.twin_arrays("slab")
    c = SR.CASES["slab"]
    assert px == SR.slab_pixels(c["W"], c["H"]) // 2
    assert SR.plan_ref(keys, tiles, mass, px)["rank_begin"] != SR.plan_ref(keys, tiles, mass, 2 * px)["rank_begin"]


@pytest.mark.parametrize("seed", range(12))
def test_random_arrays_agree(seed):
    """Random keys (clustered, so that boundaries share sub-bins and bins), tiles and masses, at sizes around the thresholds."""
    g = np.random.default_rng(100 + seed)
    n = int(g.integers(1, 3000))
    centres = np.float32(np.exp(g.uniform(np.log(0.21), np.log(1e4), 1 + seed % 5))).view(np.uint32)
    spread = (1, 40, 600, 1 << 12, 1 << 21)[seed % 5]
    keys = (g.choice(centres, n).astype(np.int64) + g.integers(0, spread, n)).astype(np.uint32)
    keys[g.random(n) < 0.1] = SR.INVISIBLE
    tiles = g.integers(0, (1 << 12, 1 << 16, 1 << 21)[seed % 3], n).astype(np.uint32)
    mass = g.integers(0, (1 << 16, 1 << 26, 1 << 32)[(seed // 3) % 3], n).astype(np.uint32)
    px = (64 * 64, 256 * 256, 1024 * 1024)[seed % 3]
    ref = _agree(keys, tiles, mass, px)
    print(n, ref["num_chunks"], ref["rank_begin"], sorted(ref["cells"]))


def test_first_mass_restates_the_host_expression():
    # 5 x float(9.2103404f) x px x 64 in binary64, truncated, plus one
    assert SR.first_mass(4096) == int(5.0 * float(np.float32(9.2103404)) * 4096.0 * 64.0) + 1 == 12072178
    assert SR.tile_floor(0) == 1 << 18 and SR.tile_floor(3) == 1 << 24 and SR.mass_target(4096, 2) == 16 * 12072178
