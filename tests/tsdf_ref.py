"""Binary64 restatement of TSDF fusion and surface nets (diff_gaussian_rasterization/tsdf.py, csrc/gsr_tsdf_math.h),
in an independent form, and their error rule.

Values.  Fusion (`fuse_ref`): an explicit loop over the cameras; every voxel centre as a homogeneous row vector times the view matrix,
the pixel by floor, the running mean as a sum and a count.  Surface nets (`surface_nets_ref`): cells as 2 x 2 x 2 sliding windows, the
twelve edges from an explicit table, crossing points in world coordinates, faces looked up in a padded cell array (a cell that does not
exist is an inactive one) and sorted by (voxel index, axis).

Error rule.  The rule of tests/normals_ref.py: `Tracked` carries a binary64 value and a first-order bound of the error of its binary32
counterpart, and the kernel's operations (csrc/gsr_tsdf_math.h) are replayed on it in the kernel's order.  The kernel's fmaf has one
rounding where the multiply and add replayed here have two, so the bound only over-estimates.  The inputs (maps, matrices, the grid's
origin and sizes: binary32 numbers) are exact.  Nothing here comes from what the code under test gives.

Fragile voxels.  The fusion takes decisions: z against 0, u and v against the integers (the pixel, and the image's edges), d against
depth_max, s against -sdf_trunc.  A voxel is fragile for a frame when one of these binary64 quantities lies within its replayed bound
of its threshold; a binary32 evaluation may then legitimately decide the other way.  The validity of a pixel (alpha >= alpha_min,
depth > 0) is decided on the binary32 inputs themselves and is never fragile.  `fuse_tracked` reports the fragile voxels and, for each,
every state a binary32 evaluation can reach (`alternatives`): the frame's update taken or not and, where u or v is within its bound of
an integer, the update through the pixel on either side of it.  A fragile voxel must equal one of them within that one's bound.
"""
import functools
import itertools

import numpy as np
import torch

from normals_ref import F64, Tracked, U  # noqa: F401  (U: for the tests' own bounds)


# ---- the grid and the frames ---------------------------------------------------------------------------------------------------------

class Grid:
    def __init__(self, dims, origin, voxel, trunc):
        self.dims = tuple(int(d) for d in dims)
        self.origin = np.asarray(origin, np.float32)
        self.voxel, self.trunc = np.float32(voxel), np.float32(trunc)

    @property
    def n(self):
        return self.dims[0] * self.dims[1] * self.dims[2]

    def coords(self, idx=None):
        """(ix, iy, iz) int64 of the voxels `idx` (all of them: x fastest)."""
        idx = np.arange(self.n, dtype=np.int64) if idx is None else np.asarray(idx, np.int64)
        nx, ny, _ = self.dims
        return idx % nx, (idx // nx) % ny, idx // (nx * ny)


class Frame:
    def __init__(self, V, depth, alpha, color, tanfovx, tanfovy, alpha_min=0.5, depth_max=np.inf):
        self.V = np.asarray(V, np.float32)
        self.depth, self.alpha, self.color = (np.ascontiguousarray(a, np.float32) for a in (depth, alpha, color))
        self.H, self.W = self.depth.shape
        self.tanfovx, self.tanfovy = float(np.float32(tanfovx)), float(np.float32(tanfovy))
        self.alpha_min, self.depth_max = float(np.float32(alpha_min)), float(np.float32(depth_max))

    @property
    def valid(self):
        """On the binary32 values themselves."""
        return (self.alpha >= np.float32(self.alpha_min)) & (self.depth > np.float32(0))


# ---- fusion: the independent form ----------------------------------------------------------------------------------------------------

def fuse_ref(grid: Grid, frames):
    """-> (tsdf [N], weight [N], color [3,N], updates): binary64, as sums and a count."""
    ix, iy, iz = grid.coords()
    P = np.stack([grid.origin[0].astype(np.float64) + float(grid.voxel) * ix, grid.origin[1].astype(np.float64) + float(grid.voxel) * iy,
                  grid.origin[2].astype(np.float64) + float(grid.voxel) * iz, np.ones(grid.n)], 1)
    tsum, csum, cnt, updates = np.zeros(grid.n), np.zeros((3, grid.n)), np.zeros(grid.n), 0
    for fr in frames:
        pv = P @ fr.V.astype(np.float64)
        z = pv[:, 2]
        front = z > 0
        zs = np.where(front, z, 1.0)
        u = fr.W / (2.0 * fr.tanfovx) * pv[:, 0] / zs + fr.W / 2.0
        v = fr.H / (2.0 * fr.tanfovy) * pv[:, 1] / zs + fr.H / 2.0
        seen = front & (u >= 0) & (u < fr.W) & (v >= 0) & (v < fr.H)
        px, py = np.floor(np.where(seen, u, 0)).astype(np.int64), np.floor(np.where(seen, v, 0)).astype(np.int64)
        ok = seen & fr.valid[py, px]
        d = np.where(ok, fr.depth[py, px].astype(np.float64), 1.0) / np.where(ok, fr.alpha[py, px].astype(np.float64), 1.0)
        s = d - z
        ok &= ~(d > fr.depth_max) & (s > -float(grid.trunc))
        t = np.minimum(1.0, s / float(grid.trunc))
        tsum += np.where(ok, t, 0.0)
        csum += np.where(ok[None], fr.color[:, py, px].astype(np.float64), 0.0)
        cnt += ok
        updates += int(ok.sum())
    den = np.maximum(cnt, 1.0)
    return tsum / den, cnt, csum / den, updates


# ---- fusion: the replay, its bound, the fragile voxels -------------------------------------------------------------------------------

def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def _view(grid: Grid, fr: Frame, idx):
    """tsdf_project's view transform on the voxels idx -> (x, y, z) Tracked."""
    w = [Tracked(float(grid.voxel)) * _t64(c) + float(o) for c, o in zip(grid.coords(idx), grid.origin)]
    V = fr.V.astype(np.float64)
    return [w[0] * float(V[0, j]) + (w[1] * float(V[1, j]) + (w[2] * float(V[2, j]) + float(V[3, j]))) for j in range(3)]


def _pixel_coords(fr: Frame, x, y, z):
    """u, v Tracked (z replaced by 1 where it is not positive)."""
    zs = z.where(z.v > 0, 1.0)
    fx, fy = Tracked(float(fr.W)) / Tracked(2.0 * fr.tanfovx), Tracked(float(fr.H)) / Tracked(2.0 * fr.tanfovy)
    return (fx * x) / zs + 0.5 * fr.W, (fy * y) / zs + 0.5 * fr.H


def _sample(grid: Grid, fr: Frame, z, pix):
    """tsdf_sample at the pixels pix (flat, >= 0) -> (t Tracked, can_update, can_skip): what a binary32 evaluation may decide."""
    valid = torch.from_numpy(fr.valid.reshape(-1))[pix]
    one = torch.ones(pix.shape, dtype=F64)
    d = Tracked(torch.where(valid, _t64(fr.depth.reshape(-1))[pix], one)) / Tracked(torch.where(valid, _t64(fr.alpha.reshape(-1))[pix], one))
    fd, over = (d.v - fr.depth_max).abs() <= d.e, d.v > fr.depth_max
    s = d - z
    trunc = float(grid.trunc)
    fs, behind = (s.v + trunc).abs() <= s.e, s.v <= -trunc
    q = s / trunc
    t = Tracked(q.v.clamp(max=1.0), torch.where(q.v - q.e >= 1, torch.zeros_like(q.e), q.e))
    return t, valid & (fd | ~over) & (fs | ~behind), ~valid | fd | over | fs | behind


def _mean(old: Tracked, w, sample: Tracked):
    """tsdf_mean: (old w + sample) / (w + 1), w exact."""
    return (old * Tracked(w) + sample) / (Tracked(w) + 1.0)


class State:
    """tsdf, color [3] Tracked and weight of some voxels."""

    def __init__(self, n):
        self.tsdf = Tracked(torch.zeros(n, dtype=F64))
        self.color = [Tracked(torch.zeros(n, dtype=F64)) for _ in range(3)]
        self.weight = torch.zeros(n, dtype=F64)

    def update(self, grid, fr, z, pix):
        """pix: the pixel each voxel is updated through, -1: skipped."""
        upd = pix >= 0
        p = pix.clamp(min=0)
        t, _, _ = _sample(grid, fr, z, p)
        upd = upd & torch.from_numpy(fr.valid.reshape(-1))[p]
        self.tsdf = _mean(self.tsdf, self.weight, t).where(upd, self.tsdf)
        for c in range(3):
            self.color[c] = _mean(self.color[c], self.weight, Tracked(_t64(fr.color[c].reshape(-1))[p])).where(upd, self.color[c])
        self.weight = torch.where(upd, self.weight + 1, self.weight)


def _near_integer(t: Tracked):
    return (t.v - t.v.round()).abs() <= t.e


def _decide(grid, fr, idx):
    """The binary64 decisions of one frame on the voxels idx -> (z, pix or -1, fragile, per-voxel candidate lists for the fragile)."""
    x, y, z = _view(grid, fr, idx)
    u, v = _pixel_coords(fr, x, y, z)
    front = z.v > 0
    inside = front & (u.v >= 0) & (u.v < fr.W) & (v.v >= 0) & (v.v < fr.H)
    px, py = u.v.floor().clamp(0, fr.W - 1).long(), v.v.floor().clamp(0, fr.H - 1).long()
    pix = py * fr.W + px
    _, can_update, can_skip = _sample(grid, fr, z, pix)
    fz = z.v.abs() <= z.e
    # an integer is a threshold of u only from 0 to W (a pixel's edge or the image's), and only where v can be inside; v likewise
    fu = _near_integer(u) & (u.v.round() >= 0) & (u.v.round() <= fr.W) & (v.v + v.e >= 0) & (v.v - v.e < fr.H)
    fv = _near_integer(v) & (v.v.round() >= 0) & (v.v.round() <= fr.H) & (u.v + u.e >= 0) & (u.v - u.e < fr.W)
    fuv = front & (fu | fv)
    fragile = fz | fuv | (inside & can_update & can_skip)
    t, _, _ = _sample(grid, fr, z, pix)
    valid = torch.from_numpy(fr.valid.reshape(-1))[pix]
    d_ok = valid & inside                                    # the binary64 path itself: _sample's flags without the bands
    one = torch.ones(pix.shape, dtype=F64)
    d = torch.where(d_ok, _t64(fr.depth.reshape(-1))[pix], one) / torch.where(d_ok, _t64(fr.alpha.reshape(-1))[pix], one)
    takes = d_ok & ~(d > fr.depth_max) & ((d - z.v) > -float(grid.trunc))
    return dict(z=z, u=u, v=v, pix=torch.where(takes, pix, torch.full_like(pix, -1)), fragile=fragile, front=front, fz=fz)


def _candidates(grid, fr, dec, k):
    """The outcomes a binary32 evaluation can reach for voxel k of `dec` (a fragile one): a set of pixels, -1 = skipped."""
    z = dec["z"][k:k + 1]
    out = set()
    if not bool(dec["front"][k]) or bool(dec["fz"][k]):
        out.add(-1)
    if not bool(dec["front"][k]):
        return out

    def along(t, n):
        val, err = float(t.v[k]), float(t.e[k])
        r = round(val)
        if abs(val - r) <= err:
            c = [r - 1, r]
        else:
            c = [int(np.floor(val))]
        return [q for q in c if 0 <= q < n], any(q < 0 or q >= n for q in c)
    xs, out_x = along(dec["u"], fr.W)
    ys, out_y = along(dec["v"], fr.H)
    if out_x or out_y:
        out.add(-1)
    for qx, qy in itertools.product(xs, ys):
        p = torch.tensor([qy * fr.W + qx])
        _, can_update, can_skip = _sample(grid, fr, z, p)
        if bool(can_update):
            out.add(int(p))
        if bool(can_skip):
            out.add(-1)
    return out


def fuse_tracked(grid: Grid, frames):
    """The replay over all voxels.  -> dict(state: State (the binary64 decisions), fragile: bool [N] (in any frame), fragile_events: the
    number of (voxel, frame) pairs that are fragile, updates: the number the reference updates, alternatives: {voxel: [State of one
    voxel, ...]} for the fragile voxels)."""
    n = grid.n
    idx = np.arange(n, dtype=np.int64)
    state = State(n)
    fragile_any = torch.zeros(n, dtype=torch.bool)
    events, updates, per_frame = 0, 0, []
    for fr in frames:
        dec = _decide(grid, fr, idx)
        state.update(grid, fr, dec["z"], dec["pix"])
        fragile_any |= dec["fragile"]
        events += int(dec["fragile"].sum())
        updates += int((dec["pix"] >= 0).sum())
        per_frame.append(dec)
    alternatives = {}
    for k in fragile_any.nonzero()[:, 0].tolist():
        cands = [sorted(_candidates(grid, fr, dec, k)) if bool(dec["fragile"][k]) else [int(dec["pix"][k])] for fr, dec in zip(frames, per_frame)]
        alts = []
        for combo in itertools.product(*cands):
            st = State(1)
            for fr, dec, p in zip(frames, per_frame, combo):
                st.update(grid, fr, dec["z"][k:k + 1], torch.tensor([p]))
            alts.append(st)
        alternatives[k] = alts
    return dict(state=state, fragile=fragile_any, fragile_events=events, updates=updates, alternatives=alternatives)


def check_volume(got_tsdf, got_weight, got_color, ref, what):
    """Holds a fused volume (arrays of N, N and [3,N]) to `ref` = fuse_tracked(...): every robust voxel within its bound with the exact
    weight, every fragile voxel equal to one of its alternatives.  Prints and returns the worst error / bound."""
    st = ref["state"]
    g_t, g_w, g_c = _t64(got_tsdf).reshape(-1), _t64(got_weight).reshape(-1), _t64(got_color).reshape(3, -1)
    robust = ~ref["fragile"]
    assert torch.equal(g_w[robust], st.weight[robust]), f"{what}: a weight differs on a robust voxel"
    worst = 0.0
    for name, got, want in [("tsdf", g_t, st.tsdf)] + [(f"color{c}", g_c[c], st.color[c]) for c in range(3)]:
        err, e = (got - want.v).abs()[robust], want.e[robust]
        assert (err[e == 0] == 0).all(), f"{what}: {name} must be exact where the bound is zero"
        r = float((err[e > 0] / e[e > 0]).max()) if (e > 0).any() else 0.0
        worst = max(worst, r)
    for k, alts in ref["alternatives"].items():
        def matches(a):
            if float(g_w[k]) != float(a.weight[0]):
                return False
            pairs = [(g_t[k], a.tsdf)] + [(g_c[c][k], a.color[c]) for c in range(3)]
            return all(abs(float(g) - float(w.v[0])) <= float(w.e[0]) for g, w in pairs)
        assert any(matches(a) for a in alts), f"{what}: fragile voxel {k} equals none of its {len(alts)} reachable states"
    print(f"{what}: worst error / bound = {worst:.3f} on {int(robust.sum())} robust voxels; {ref['fragile_events']} fragile (voxel, frame) pairs of "
          f"{ref['updates']} updates ({100.0 * ref['fragile_events'] / max(ref['updates'], 1):.4f} %)")
    return worst


FRAGILE_CAP = 0.01          # of the updates the reference makes: a condition on the fixtures, asserted wherever one is used


def assert_cap(ref, what):
    share = ref["fragile_events"] / max(ref["updates"], 1)
    print(f"{what}: fragile share {share:.6f} ({ref['fragile_events']} of {ref['updates']})")
    assert ref["updates"] > 0 and share <= FRAGILE_CAP, f"{what}: {share:.4f} of the updates are fragile: choose another fixture"


# ---- surface nets --------------------------------------------------------------------------------------------------------------------

# the twelve edges (lower corner, upper corner, axis): x edges, then y, then z, each by ascending lower corner; corner k = x + 2 y + 4 z
EDGES = tuple((ka, ka | (1 << a), a) for a in range(3) for ka in range(8) if not ka & (1 << a))
CORNER = np.array([[k & 1, (k >> 1) & 1, k >> 2] for k in range(8)], np.int64)


def surface_nets_ref(grid: Grid, tsdf32, weight32, color32, min_weight=1.0):
    """tsdf32, weight32 [nz,ny,nx], color32 [3,nz,ny,nx]: binary32 arrays -> dict(vertices: Tracked [V,3], colors: Tracked [V,3], faces:
    int64 [F,3], cells: int64 [V,3] (the cells' lowest corners), quad_owners: int64 [F/2] (the voxel index, x fastest, that owns each
    quad, in the faces' order)).  The values are the world-space means; the bounds the replay's."""
    nx, ny, nz = grid.dims
    empty = dict(vertices=Tracked(torch.zeros(0, 3, dtype=F64)), colors=Tracked(torch.zeros(0, 3, dtype=F64)), faces=np.zeros((0, 3), np.int64),
                 cells=np.zeros((0, 3), np.int64), quad_owners=np.zeros(0, np.int64))
    if min(nx, ny, nz) < 2:
        return empty
    tsdf32, weight32 = np.asarray(tsdf32, np.float32).reshape(nz, ny, nx), np.asarray(weight32, np.float32).reshape(nz, ny, nx)
    color32 = np.asarray(color32, np.float32).reshape(3, nz, ny, nx)
    obs, inside = weight32 >= np.float32(min_weight), tsdf32 < 0
    win = np.lib.stride_tricks.sliding_window_view
    wo, wi = win(obs, (2, 2, 2)), win(inside, (2, 2, 2))
    active = wo.all((3, 4, 5)) & wi.any((3, 4, 5)) & (~wi).any((3, 4, 5))
    cells = np.argwhere(active)[:, ::-1]                                  # (x, y, z) rows in ascending cell index
    nv = cells.shape[0]
    if nv == 0:
        return empty
    vid = np.full((nz + 1, ny + 1, nx + 1), -1, np.int64)                 # by cell + 1: a cell that does not exist is inactive
    vid[cells[:, 2] + 1, cells[:, 1] + 1, cells[:, 0] + 1] = np.arange(nv)
    # ---- the vertices
    corner = cells[:, None, :] + CORNER[None]                             # [V,8,3]
    f = tsdf32[corner[..., 2], corner[..., 1], corner[..., 0]].astype(np.float64)
    col = color32[:, corner[..., 2], corner[..., 1], corner[..., 0]].astype(np.float64)          # [3,V,8]
    world = grid.origin.astype(np.float64)[None, None] + float(grid.voxel) * corner
    psum, csum, cnt = np.zeros((nv, 3)), np.zeros((nv, 3)), np.zeros(nv)
    ft = _t64(f)
    acc = [Tracked(torch.zeros(nv, dtype=F64)) for _ in range(3)]
    cacc = [Tracked(torch.zeros(nv, dtype=F64)) for _ in range(3)]
    for ka, kb, a in EDGES:
        cross = (f[:, ka] < 0) != (f[:, kb] < 0)
        den = np.where(cross, f[:, ka] - f[:, kb], 1.0)
        lam = f[:, ka] / den
        psum += np.where(cross[:, None], world[:, ka] + (world[:, kb] - world[:, ka]) * lam[:, None], 0.0)
        csum += np.where(cross[:, None], (col[:, :, ka] + (col[:, :, kb] - col[:, :, ka]) * lam[None]).T, 0.0)
        cnt += cross
        # the replay: sn_vertex
        ct = torch.from_numpy(cross)
        t = Tracked(ft[:, ka]) / (Tracked(ft[:, ka]) - Tracked(torch.where(ct, ft[:, kb], ft[:, ka] - 1.0)))
        for j in range(3):
            acc[j] = (acc[j] + (t if j == a else Tracked(float(CORNER[ka, j])))).where(ct, acc[j])
        for c in range(3):
            ca, cb = Tracked(_t64(col[c, :, ka])), Tracked(_t64(col[c, :, kb]))
            cacc[c] = (cacc[c] + ((cb - ca) * t + ca)).where(ct, cacc[c])
    inv = Tracked(1.0) / Tracked(_t64(cnt))
    pos = [Tracked(float(grid.voxel)) * (acc[j] * inv + _t64(cells[:, j])) + float(grid.origin[j]) for j in range(3)]
    rgb = [cacc[c] * inv for c in range(3)]
    vertices = Tracked(_t64(psum / cnt[:, None]), torch.stack([p.e for p in pos], 1))
    colors = Tracked(_t64(csum / cnt[:, None]), torch.stack([c.e for c in rgb], 1))
    replay = dict(vertices=torch.stack([p.v for p in pos], 1), colors=torch.stack([c.v for c in rgb], 1))
    # ---- the faces
    n = (nx, ny, nz)
    rows = []
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        lo = [slice(0, n[j] - (j == a)) for j in range(3)]
        hi = [slice(int(j == a), n[j]) for j in range(3)]
        edge = obs[lo[2], lo[1], lo[0]] & obs[hi[2], hi[1], hi[0]] & (inside[lo[2], lo[1], lo[0]] != inside[hi[2], hi[1], hi[0]])
        p = np.argwhere(edge)[:, ::-1]                                    # (x, y, z) of the edge's lower voxel
        quad = []
        for ob, oc in ((-1, -1), (0, -1), (0, 0), (-1, 0)):               # counter-clockwise seen against the axis
            q = p.copy()
            q[:, b] += ob
            q[:, c] += oc
            quad.append(vid[q[:, 2] + 1, q[:, 1] + 1, q[:, 0] + 1])
        quad = np.stack(quad, 1) if len(p) else np.zeros((0, 4), np.int64)
        keep = (quad >= 0).all(1)
        p, quad = p[keep], quad[keep]
        lin = (p[:, 2] * ny + p[:, 1]) * nx + p[:, 0]
        rows.append(np.concatenate([lin[:, None], np.full((len(p), 1), a), quad, inside[p[:, 2], p[:, 1], p[:, 0]][:, None].astype(np.int64)], 1))
    rows = np.concatenate(rows)
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    faces = []
    for lin, a, v0, v1, v2, v3, voxel_inside in rows.tolist():
        faces += [(v0, v1, v2), (v0, v2, v3)] if voxel_inside else [(v0, v2, v1), (v0, v3, v2)]
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    return dict(vertices=vertices, colors=colors, faces=faces, cells=cells, replay=replay, quad_owners=rows[:, 0].copy())


# ---- the kernels' one-block scans: rounds, and the rules a scan could follow between them ----------------------------------------------

SCAN_BLOCK = 256                                            # voxels, faces or vertices per block (kSnBlock, kMeshBlock)
SCAN_ROUND = 8192 * SCAN_BLOCK                              # per round of k_sn_scan and of mesh_scan_counts: 1 024 threads x 8 blocks each
CARRY_RULES = ("right", "reset", "last")


def scan_rounds(owners, n):
    """The number of `owners` (element indices in [0, n)) per scan round of SCAN_ROUND elements -> int64 [ceil(n / SCAN_ROUND)]."""
    owners = np.asarray(owners, np.int64).reshape(-1)
    return np.bincount(owners // SCAN_ROUND, minlength=max(1, -(-int(n) // SCAN_ROUND))).astype(np.int64)


def block_counts(owners, n):
    """The number of `owners` per block of SCAN_BLOCK elements -> int64 [ceil(n / SCAN_BLOCK)]."""
    return np.bincount(np.asarray(owners, np.int64).reshape(-1) // SCAN_BLOCK, minlength=-(-int(n) // SCAN_BLOCK)).astype(np.int64)


def block_prefixes(counts, rule="right"):
    """The exclusive prefix of every block's count as a scan in rounds of 8 192 blocks gives it under `rule`: "right" (the carry is the
    sum of all rounds before), "reset" (the carry is 0 in every round), "last" (the carry is the previous round's total alone)."""
    counts = np.asarray(counts, np.int64)
    per = SCAN_ROUND // SCAN_BLOCK
    rounds = -(-len(counts) // per)
    padded = np.zeros(rounds * per, np.int64)
    padded[:len(counts)] = counts
    padded = padded.reshape(rounds, per)
    within = np.cumsum(padded, 1) - padded
    totals = padded.sum(1)
    carry = {"right": np.cumsum(totals) - totals, "reset": np.zeros(rounds, np.int64), "last": np.concatenate([[0], totals[:-1]])}[rule]
    return (within + carry[:, None]).reshape(-1)[:len(counts)]


def assert_rules_differ(counts, what):
    """A fixture of three rounds or more tells the two wrong carry rules from the right one: "reset" is wrong at every block of rounds
    1 and 2, "last" at every block of round 2, and both are right wherever else the first three rounds go."""
    per = SCAN_ROUND // SCAN_BLOCK
    assert len(counts) > 2 * per, f"{what}: {len(counts)} blocks are fewer than three rounds"
    right, reset, last = (block_prefixes(counts, r) for r in CARRY_RULES)
    assert np.array_equal(right, np.cumsum(counts) - counts)
    rnd = np.arange(len(counts)) // per
    assert np.array_equal(reset[rnd == 0], right[rnd == 0]) and (reset[rnd == 1] != right[rnd == 1]).all() and (reset[rnd == 2] != right[rnd == 2]).all()
    assert np.array_equal(last[rnd <= 1], right[rnd <= 1]) and (last[rnd == 2] != right[rnd == 2]).all()
    print(f"{what}: the prefixes of blocks {per} and {2 * per} are {right[per]} and {right[2 * per]}; with the carry reset {reset[per]} and "
          f"{reset[2 * per]}; with the last round's total alone {last[per]} and {last[2 * per]}")


def assert_rounds(owners, n, what, at_least=1000):
    """The condition on a fixture of the scans: three rounds or more, `at_least` owners in every round, and a non-zero prefix at the
    first block of rounds 1 and 2.  Prints and returns the counts per round."""
    rounds = scan_rounds(owners, n)
    print(f"{what}: {n} elements in {-(-n // SCAN_BLOCK)} blocks, {len(rounds)} rounds; per round {rounds.tolist()}")
    assert len(rounds) >= 3, f"{what}: {len(rounds)} rounds"
    assert int(rounds.min()) >= at_least, f"{what}: a round holds fewer than {at_least}"
    prefix = block_prefixes(block_counts(owners, n))
    per = SCAN_ROUND // SCAN_BLOCK
    assert prefix[per] > 0 and prefix[2 * per] > prefix[per], f"{what}: the first block of round 1 or 2 has a zero prefix"
    return rounds


def mesh_topology(faces):
    """-> dict(undirected_ok, directed_ok, euler) of a triangle list: every undirected edge in exactly two triangles, every directed
    edge in exactly one, V - E + F over the vertices the faces use."""
    faces = np.asarray(faces, np.int64)
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]])
    _, dc = np.unique(d, axis=0, return_counts=True)
    und, uc = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    return dict(undirected_ok=bool((uc == 2).all()), directed_ok=bool((dc == 1).all()),
                euler=int(np.unique(faces).size - und.shape[0] + faces.shape[0]))


def signed_volume(vertices, faces):
    v = np.asarray(vertices, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

SPHERE_R = 0.6
TANFOV = (float(np.float32(0.7)), float(np.float32(0.55)))


def look_at(campos, target, roll=0.0):
    """The view matrix [4,4] binary32 in the row-vector convention (x right, y down, z forward) of a camera at campos looking at target."""
    c, t = np.asarray(campos, np.float64), np.asarray(target, np.float64)
    fwd = (t - c) / np.linalg.norm(t - c)
    up = np.array([0.0, 0.0, 1.0]) if abs(fwd[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    cr, sr = np.cos(roll), np.sin(roll)
    right, down = cr * right + sr * down, -sr * right + cr * down
    V = np.eye(4)
    V[:3, :3] = np.stack([right, down, fwd], 1)
    V[3, :3] = -c @ V[:3, :3]
    return V.astype(np.float32)


def sphere_frame(V, W, H, radius=SPHERE_R, holes=True, depth_max=np.inf, seed=0, tanfov=TANFOV):
    """The maps of a camera that sees the sphere of `radius` around the origin (from outside: its near side; from inside: the far one),
    as depth_alpha=True leaves them: alpha below 1 and varying, depth = z alpha, alpha 0 where no ray hits; with `holes`, alpha under
    alpha_min at scattered pixels and along one row."""
    V64 = np.asarray(V, np.float64)
    R, c = V64[:3, :3], -V64[3, :3] @ V64[:3, :3].T
    fx, fy = W / (2.0 * tanfov[0]), H / (2.0 * tanfov[1])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    dv = np.stack([(x + 0.5 - W / 2) / fx, (y + 0.5 - H / 2) / fy, np.ones_like(x)], -1)
    dw = dv @ R.T
    A, B, C0 = (dw * dw).sum(-1), 2.0 * (dw @ c), float(c @ c) - radius * radius
    disc = B * B - 4 * A * C0
    hit = disc > 0
    root = np.sqrt(np.where(hit, disc, 0.0))
    near, far = (-B - root) / (2 * A), (-B + root) / (2 * A)
    lam = np.where(near > 0, near, far)
    hit &= lam > 0
    rng = np.random.default_rng(100 * W + H + seed)
    alpha = np.where(hit, 0.75 + 0.2 * np.sin(0.4 * x + 0.3 * y) + 0.04 * rng.random((H, W)), 0.0).astype(np.float32)
    if holes:
        for _ in range(max(2, H * W // 60)):
            alpha[rng.integers(H), rng.integers(W)] = np.float32(0.3)
        alpha[H // 3, :] = np.float32(0.2)
    depth = (np.where(hit, lam, 0.0).astype(np.float32) * alpha).astype(np.float32)
    pw = c[None, None] + lam[..., None] * dw
    color = np.clip(0.5 + 0.5 * np.moveaxis(pw, -1, 0) / radius, 0, 1) * alpha[None]
    return Frame(V, depth, alpha, color.astype(np.float32), tanfov[0], tanfov[1], 0.5, depth_max)


GRIDS = {                                                   # name -> Grid; the sphere of SPHERE_R around the world's origin passes through each
    "17x9x21": Grid((17, 9, 21), (-0.83, -0.37, -1.02), 0.1, 0.3),
    "1x1x1": Grid((1, 1, 1), (0.05, -0.02, -0.55), 0.1, 0.25),
    "64x64x64": Grid((64, 64, 64), (-1.0, -1.0, -1.0), 2.0 / 63.0, 5 * 2.0 / 63.0),
}
MESH_GRIDS = {                                              # for the extraction alone: one cell; block edges (256 voxels) along every axis
    "2x2x2": Grid((2, 2, 2), (0.02, -0.03, -0.66), 0.1, 0.3),
    "65x33x70": Grid((65, 33, 70), (-0.95, -0.5, -1.03), 0.03, 0.15),
}
MAPS = ((33, 17), (96, 96))                                 # W x H


def make_frames(W, H, seed=0):
    """Three frames in sequence: a rotated and translated camera outside the volume, with holes in alpha; a camera inside the volume
    (and the sphere), so that voxels lie behind it and project outside the image; another outside camera whose depth_max cuts the
    far pixels of its silhouette.  seed: another draw of the maps' noise and holes; the cameras stay."""
    return [sphere_frame(look_at((1.9, -1.2, 0.9), (0.05, 0.0, -0.1), roll=0.35), W, H, seed=10 * seed + 1),
            sphere_frame(look_at((0.12, 0.07, -0.21), (-0.4, 0.3, -0.9), roll=-0.2), W, H, seed=10 * seed + 2),
            sphere_frame(look_at((-0.3, 0.25, -2.4), (0.0, -0.05, 0.0), roll=1.1), W, H, depth_max=2.05, seed=10 * seed + 3)]


def analytic_sphere(n=24, radius=SPHERE_R):
    """(grid, tsdf, weight, color): the signed distance to the sphere sampled on n^3 voxels of [-1,1]^3, every voxel observed."""
    grid = Grid((n, n, n), (-1.0, -1.0, -1.0), 2.0 / (n - 1), 5 * 2.0 / (n - 1))
    ix, iy, iz = grid.coords()
    p = grid.origin.astype(np.float64)[None] + float(grid.voxel) * np.stack([ix, iy, iz], 1)
    sdf = (np.linalg.norm(p, axis=1) - radius) / float(grid.trunc)
    tsdf = np.clip(sdf, -1, 1).astype(np.float32).reshape(n, n, n)
    color = np.clip(0.5 + 0.5 * p.T / radius, 0, 1).astype(np.float32).reshape(3, n, n, n)
    return grid, tsdf, np.ones((n, n, n), np.float32), color


THREE_ROUND_DIMS = (131, 127, 300)                          # 4 991 100 voxels = 19 497 blocks of 256: three rounds of k_sn_scan; x no multiple of 64
THREE_ROUND_PLANE = ((1.0, 0.21, 0.13), 90.0)               # n . p = d, p in voxels: x runs from 24.7 to 90, so every z slab is crossed
THREE_ROUND_SPHERE = ((108.0, 50.0, 200.0), 14.0)           # wholly inside the volume, 35 voxels and more away from the plane
THREE_ROUND_HOLE = ((40, 80), (30, 60), (100, 140))         # [lo, hi) per axis: weight 0, a hole inside the plane (it does not split it)
THREE_ROUND_SEEN_TWICE = 40                                 # y >= this: weight 2 (it cuts the plane, the hole and the sphere)


@functools.lru_cache(maxsize=None)
def three_round_volume(small=True):
    """(grid, tsdf, weight, color), read-only and computed once: an analytic volume of THREE_ROUND_DIMS voxels (voxel size 1, trunc 3)
    that holds a tilted plane (inside: below it) and, with `small`, a sphere on its outer side; weight 0 in a box that the plane crosses,
    2 where y >= THREE_ROUND_SEEN_TWICE and 1 elsewhere; the colour is a function of the place.  Without `small` every value the plane's
    cells read is the same: the sphere's distance is past the truncation there."""
    nx, ny, nz = THREE_ROUND_DIMS
    grid = Grid(THREE_ROUND_DIMS, (0.0, 0.0, 0.0), 1.0, 3.0)
    x, y, z = np.arange(nx, dtype=np.float64)[None, None, :], np.arange(ny, dtype=np.float64)[None, :, None], np.arange(nz, dtype=np.float64)[:, None, None]
    (a, b, c), d = THREE_ROUND_PLANE
    sdf = (a * x + b * y + c * z - d) / np.sqrt(a * a + b * b + c * c)
    if small:
        (cx, cy, cz), r = THREE_ROUND_SPHERE
        sdf = np.minimum(sdf, np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2) - r)
    tsdf = np.clip(sdf / 3.0, -1, 1).astype(np.float32)
    weight = np.ones((nz, ny, nx), np.float32)
    weight[:, THREE_ROUND_SEEN_TWICE:, :] = 2.0
    (x0, x1), (y0, y1), (z0, z1) = THREE_ROUND_HOLE
    weight[z0:z1, y0:y1, x0:x1] = 0.0
    color = np.stack([np.broadcast_to(v / n, (nz, ny, nx)) for v, n in ((x, nx), (y, ny), (z, nz))]).astype(np.float32)
    for arr in (tsdf, weight, color):
        arr.setflags(write=False)
    return grid, tsdf, weight, color


def sphere_deviation(grid: Grid, vertices, radius=SPHERE_R):
    """The largest distance of a vertex from the sphere, in voxels."""
    return float(np.abs(np.linalg.norm(np.asarray(vertices, np.float64), axis=1) - radius).max() / float(grid.voxel))
