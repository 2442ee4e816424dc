"""Exact host reference of the depth selection's chunk plan (csrc/gsr_select.hip), restated from the documented rule.

The rule (header of csrc/gsr_select.hip, csrc/gsr_internal.h "depth selection", launch_depth_select's first_mass).  Visible
Gaussians (key != 0xFFFFFFFF) in key order carry running sums of count, tiles touched and fixed-point optical mass.  Boundary c
(0 .. MAX_CHUNKS - 2) exists only if the tile floor kMinFirstChunk * 4^c is below R, the frame's tile total.  It is the smallest
ALIGNED key edge e at which the sums over the keys <= e satisfy both
    running mass  > first_mass * 4^c      and      running tiles > kMinFirstChunk * 4^c;
edges are aligned to 2^kSelShift2 for the first kSelRefine boundaries and to 2^kSelShift1 for the others.  If no edge satisfies
both, the boundary does not exist either.  The chunk behind a boundary ends at the last key code below that edge, with the sums
there.  A boundary that adds no Gaussian to the one before it is dropped; where a boundary does not exist the chunk takes
everything left; the chunk that reaches V is the last one, and its key_end and every later one are 0xFFFFFFFE.  key_max is the
last code of the highest occupied 2^kSelShift1 bin, capped at 0xFFFFFFFE (no bin is occupied when V = 0: unspecified, None here).

Everything is integer work: plan_ref() works on whole aligned groups of the sorted keys; tests/test_select_ref.py holds it to a
Gaussian-by-Gaussian walk.  The named constants are read out of the sources, so a retune does not fork the test.
"""
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
INVISIBLE = 0xFFFFFFFF
SENTINEL = 0xFFFFFFFE
TILE = 16

CELLS = ("one-subbin", "subbin-edge", "bin-edge", "empty-merged", "coarse", "chunks8", "floor-takes-rest", "mass-bound",
         "tile-bound", "V0", "P1")


def _constants():
    src = open(os.path.join(ROOT, "structured-gaussian-splatting_amd", "csrc", "gsr_internal.h")).read()
    pub = open(os.path.join(ROOT, "include", "gsrast.h")).read()

    def grab(name, text=src):
        m = re.search(r"constexpr\s+\w+\s+" + name + r"\s*=\s*([^;]+);", text)
        assert m, f"{name} not found in gsr_internal.h"
        return m.group(1).strip()

    def integer(expr):
        m = re.fullmatch(r"(\d+)u?\s*<<\s*(\d+)", expr)
        return int(m.group(1)) << int(m.group(2)) if m else int(expr.rstrip("u"))

    def f32(expr):
        return np.float32(expr.rstrip("f"))
    m = re.search(r"#define\s+GSR_MAX_CHUNKS\s+(\d+)", pub)
    assert m, "GSR_MAX_CHUNKS not found in gsrast.h"
    return dict(shift1=integer(grab("kSelShift1")), shift2=integer(grab("kSelShift2")), refine=integer(grab("kSelRefine")),
                sel_blocks=integer(grab("kSelBlocks")), min_first=integer(grab("kMinFirstChunk")),
                growth_log2=integer(grab("kChunkGrowthLog2")), cutoff=f32(grab("kCutoffOpticalDepth")),
                depths=f32(grab("kChunkOpticalDepths")), units=f32(grab("kMassUnitsPerPixelNeper")), max_chunks=int(m.group(1)))


K = _constants()
MAX_CHUNKS = K["max_chunks"]


def slab_pixels(W, H, tile_rows=None):
    Gx, Gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ty0, ty1 = tile_rows if tile_rows else (0, Gy)
    return (ty1 - ty0) * TILE * Gx * TILE


def first_mass(slab_px):
    """launch_depth_select's first_mass: binary32 constants, the product in binary64 left to right, truncated, plus one."""
    return int(float(K["depths"]) * float(K["cutoff"]) * float(slab_px) * float(K["units"])) + 1


def mass_target(slab_px, c):
    return first_mass(slab_px) << (K["growth_log2"] * c)


def tile_floor(c):
    return K["min_first"] << (K["growth_log2"] * c)


def align_bits(c):
    return K["shift2"] if c < K["refine"] else K["shift1"]


def sorted_visible(keys, tiles, mass):
    """Visible Gaussians in (key, index) order: keys, tiles, mass as Python-int-safe uint64 arrays."""
    keys = np.asarray(keys, np.uint32)
    vis = np.nonzero(keys != np.uint32(INVISIBLE))[0]
    o = vis[np.argsort(keys[vis], kind="stable")]
    return keys[o].astype(np.uint64), np.asarray(tiles, np.uint32)[o].astype(np.uint64), np.asarray(mass, np.uint32)[o].astype(np.uint64)


def plan_ref(keys, tiles, mass, slab_px):
    """The plan of one frame from its per-Gaussian keys, tile counts and masses (uint32 arrays; key 0xFFFFFFFF = invisible).
    Returns V, R, num_chunks (1 for an empty frame, as the library reports it), key_end[8], rank_begin[9], instances_max[8],
    key_max (None when V = 0) and `cells`, the coverage cells (CELLS) this input reaches."""
    n_in = int(np.asarray(keys).size)
    k, t, m = sorted_visible(keys, tiles, mass)
    V = int(k.size)
    cum_t, cum_m = np.cumsum(t, dtype=np.uint64), np.cumsum(m, dtype=np.uint64)
    R = int(cum_t[-1]) if V else 0
    cells = set()
    # boundary c: (edge key, Gaussians at or below it, tiles at or below it), or None
    bounds = []
    for c in range(MAX_CHUNKS - 1):
        T, F, a = mass_target(slab_px, c), tile_floor(c), align_bits(c)
        b = None
        if V and F < R:
            last = np.nonzero(np.append(k[1:] >> np.uint64(a) != k[:-1] >> np.uint64(a), True))[0]      # last Gaussian of each aligned group
            ok = np.nonzero((cum_m[last] > np.uint64(T)) & (cum_t[last] > np.uint64(F)))[0]
            if ok.size:
                j = int(last[ok[0]])
                edge = min((((int(k[j]) >> a) + 1) << a) - 1, SENTINEL)
                b = (edge, j + 1, int(cum_t[j]))
        bounds.append(b)
    key_end, rank_begin, inst = [], [0], []
    begin, begin_tiles, kept = 0, 0, []
    for c in range(MAX_CHUNKS):
        if begin >= V:
            break
        b = bounds[c] if c < MAX_CHUNKS - 1 else None
        edge, cnt, til = b if b else (SENTINEL, V, R)
        if cnt <= begin:
            continue                                    # adds nothing to the boundary before it
        if cnt >= V:
            edge = SENTINEL                             # the last chunk ends at "everything"
        elif b:
            kept.append((c, edge))
        key_end.append(edge); rank_begin.append(cnt); inst.append(min(til - begin_tiles, 0xFFFFFFFF))
        begin, begin_tiles = cnt, til
    n = len(key_end)
    key_end += [SENTINEL] * (MAX_CHUNKS - n)
    rank_begin += [V] * (MAX_CHUNKS - n)
    inst += [0] * (MAX_CHUNKS - n)
    key_max = min((((int(k[-1]) >> K["shift1"]) + 1) << K["shift1"]) - 1, SENTINEL) if V else None

    # ---- coverage cells
    if V == 0:
        cells.add("V0")
    if n_in == 1:
        cells.add("P1")
    if V and int(k[0]) >> K["shift2"] == int(k[-1]) >> K["shift2"] and R > K["min_first"]:
        cells.add("one-subbin")
    kset = k
    for c, edge in kept:
        if c >= K["refine"]:
            cells.add("coarse")
        i = int(np.searchsorted(kset, np.uint64(edge), side="right"))
        adjacent = 0 < i < V and int(kset[i - 1]) == edge and int(kset[i]) == edge + 1       # populations one key code apart
        if adjacent and c < K["refine"] and (edge + 1) % (1 << K["shift1"]):
            cells.add("subbin-edge")
        if adjacent and (edge + 1) % (1 << K["shift1"]) == 0:
            cells.add("bin-edge")
    if bounds[0] and bounds[1] and bounds[0][0] == bounds[1][0]:
        cells.add("empty-merged")
    if n == MAX_CHUNKS:
        cells.add("chunks8")
    if V:
        c_stop = next((c for c in range(MAX_CHUNKS - 1) if tile_floor(c) >= R), None)
        if c_stop is not None:                          # the floor ends the plan here: would the mass alone have cut the rest?
            i = int(np.searchsorted(cum_m, np.uint64(mass_target(slab_px, c_stop)), side="right"))      # first index with cum_m > T
            if i < V:
                a = align_bits(c_stop)
                e = (((int(k[i]) >> a) + 1) << a) - 1
                if int(np.searchsorted(k, np.uint64(e), side="right")) < V:
                    cells.add("floor-takes-rest")
    if bounds[0]:
        i_m = int(np.searchsorted(cum_m, np.uint64(mass_target(slab_px, 0)), side="right"))
        i_t = int(np.searchsorted(cum_t, np.uint64(tile_floor(0)), side="right"))
        if i_m > i_t:
            cells.add("mass-bound")
        if i_t > i_m:
            cells.add("tile-bound")
    return dict(V=V, R=R, num_chunks=max(n, 1), key_end=key_end, rank_begin=rank_begin, instances_max=inst, key_max=key_max, cells=cells)


def partition_ref(keys, key_end, num_chunks):
    """The expected depth_order[:V] behind the partition: chunk after chunk, index order inside each."""
    keys = np.asarray(keys, np.uint32)
    vis = np.nonzero(keys != np.uint32(INVISIBLE))[0]
    chunk = np.zeros(vis.size, np.int64)
    for c in range(num_chunks - 1):
        chunk += keys[vis] > np.uint32(key_end[c])
    return vis[np.argsort(chunk, kind="stable")].astype(np.int64)


# ---- the frames that target the cells.  Every splat sits on the optical axis of scene_synth.make_camera (view depth = z, an exactly
# representable plane), is isotropic and wider than the screen (sigma = 2 max(W, H) px), so its tile count is the slab's and its
# mass sits on the rectangle cap: the integers are predictable, and twin_arrays() states them without a device.
def f32_from_bits(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def _spread(n, z0, codes, seed):
    """n depths above z0 (a power of two), `codes` key codes apart, in a seeded shuffled index order."""
    z = (np.float32(z0).view(np.uint32) + np.arange(n, dtype=np.uint32) * np.uint32(codes)).view(np.float32)
    return np.random.default_rng(seed).permutation(z)


def _interleave(a, b, seed):
    z = np.concatenate([a, b])
    return np.random.default_rng(seed).permutation(z)


def _chunks8_depths():
    # group g sits in the first 2^20 bin of binade 2^g; boundary c (mass-bound: ~11.5 Gaussians x 4^c) falls inside group c
    sizes = (20, 40, 200, 800, 3000, 12000, 36000, 6000)
    parts = [(np.float32(2.0 ** g).view(np.uint32) + (np.arange(n, dtype=np.uint32) % np.uint32(1024)) * np.uint32(512)
              + np.arange(n, dtype=np.uint32) // np.uint32(1024)).view(np.float32) for g, n in enumerate(sizes)]
    return np.random.default_rng(8).permutation(np.concatenate(parts))


CASES = {
    # all of V inside one 512-code sub-bin (300 codes of it), 64 tiles each: R = 320 000 > 2^18
    "one-subbin": dict(W=128, H=128, opacity=0.99, cell="one-subbin",
                       z=lambda: f32_from_bits(np.uint32(0x40000000) + np.random.default_rng(1).integers(0, 300, 5000).astype(np.uint32))),
    # 16 390 Gaussians on the last code of a sub-bin, 1 000 on the next code; 16 tiles each: the floor is passed by the 16 385th
    "subbin-edge": dict(W=64, H=64, opacity=0.99, cell="subbin-edge",
                        z=lambda: _interleave(f32_from_bits(np.full(16390, 0x400001FF, np.uint32)),
                                              f32_from_bits(np.full(1000, 0x40000200, np.uint32)), 2)),
    # the same across a 2^20 edge: the float just below 2.0, and 2.0; 20 tiles each: the floor is passed by the 13 108th
    "bin-edge": dict(W=80, H=64, opacity=0.99, cell="bin-edge",
                     z=lambda: _interleave(np.full(13200, np.nextafter(np.float32(2.0), np.float32(0.0)), np.float32),
                                           np.full(900, 2.0, np.float32), 3)),
    # 256 tiles each: boundary 0 (1 025th) and boundary 1 (4 097th) both fall on the 6 000 Gaussians that share one key
    "empty-merged": dict(W=256, H=256, opacity=0.99, cell="empty-merged",
                         z=lambda: _interleave(np.concatenate([np.full(100, 1.0, np.float32), np.full(6000, 2.0, np.float32)]),
                                               np.full(500, 4.0, np.float32), 4)),
    "chunks8": dict(W=4096, H=4096, opacity=0.99, cell="chunks8", also=("coarse",), z=_chunks8_depths),
    # R = 160 000 <= 2^18 although the mass target is passed by the 11th Gaussian
    "floor-takes-rest": dict(W=64, H=64, opacity=0.99, cell="floor-takes-rest", z=lambda: _spread(10000, 1.0, 700, 5)),
    "tile-bound": dict(W=64, H=64, opacity=0.99, cell="tile-bound", z=lambda: _spread(17000, 1.0, 256, 6)),
    # 256 tiles each: the floor is passed by the 1 025th Gaussian, the mass target by about the 4 583rd
    "mass-bound": dict(W=256, H=256, opacity=0.01, cell="mass-bound", z=lambda: _spread(6000, 1.0, 700, 7)),
    "V0": dict(W=64, H=64, opacity=0.99, cell="V0", z=lambda: np.full(1000, 0.1, np.float32)),         # in front of the near cut
    "P1": dict(W=64, H=64, opacity=0.99, cell="P1", z=lambda: np.full(1, 3.0, np.float32)),
    # a slab of 6 of 12 tile rows: 96 tiles each, the mass target follows the slab's pixels
    "slab": dict(W=256, H=192, opacity=0.01, cell="mass-bound", tile_rows=(3, 9), z=lambda: _spread(6000, 1.0, 700, 9)),
}
NEAR_CUT = np.float32(0.2)
ALPHA_MAX = np.float32(0.99)


def twin_arrays(case):
    """(keys, tiles, mass, slab_px) a device is expected to derive from a case: csrc/gsr_math.h optical_mass on its cap."""
    c = CASES[case]
    z = np.asarray(c["z"](), np.float32)
    W, H = c["W"], c["H"]
    Gx, Gy = (W + TILE - 1) // TILE, (H + TILE - 1) // TILE
    ty0, ty1 = c.get("tile_rows") or (0, Gy)
    keys = np.where(z > NEAR_CUT, z.view(np.uint32), np.uint32(INVISIBLE))
    full, slab = Gx * Gy, Gx * (ty1 - ty0)
    op = min(np.float32(c["opacity"]), ALPHA_MAX)
    m = np.float32(full) * np.float32(TILE * TILE) * -np.log(np.float32(1) - op) * (np.float32(slab) / np.float32(full))
    units = np.uint32(min(np.float32(m) * K["units"], np.float32(4294967040.0)))
    vis = keys != np.uint32(INVISIBLE)
    return keys, np.where(vis, np.uint32(slab), np.uint32(0)), np.where(vis, units, np.uint32(0)), slab_pixels(W, H, c.get("tile_rows"))
