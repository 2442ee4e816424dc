"""CPU checks of the frame's host-side path rules (csrc/gsr_dispatch.h): the header, compiled by g++ under AddressSanitizer and UBSan
as a stand-alone program (tests/dispatch_host.cpp, run as a child process), against the independent statements the suite already has:
tests/binning_ref.py chunk_cells (the binning path of a chunk), tests/test_gpu_parity.py _geom_variants (colour kernels, sparse or dense
geometry backward), _native.binned_prefix / effective_binned_ranks / first_chunk_capacity, the exported gsr_binning_first_chunk_capacity,
and short restatements written here (the merge of the remaining chunks, the live filter, the plan's sizes).  The mirrors stay
independent: none of them calls the header.  Every comparison takes its mirror as an argument and returns the list of differences, so
that the self-checks can hand it a copy of the mirror with one threshold moved by one and see it fail (as test_abi.py's mutated tables).
"""
import inspect
import os
import random
import subprocess

import pytest

import binning_ref as BR
from test_gpu_parity import _geom_variants

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAXC = BR.MAX_CHUNKS
NEAR = 0x3E4CCCCD                    # bits of 0.2f: the lower end of the first chunk's keys
KEY_ALL = 0xFFFFFFFE


@pytest.fixture(scope="module")
def native():
    from diff_gaussian_rasterization import _native
    if not os.path.exists(_native.lib_path()):
        _native.build()
    return _native


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """run(lines) -> one list of ints per line that prints (every command but `plan`)."""
    exe = os.path.join(str(tmp_path_factory.mktemp("dispatch")), "dispatch_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "dispatch_host.cpp")])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        rows = [[int(x) for x in ln.split()] for ln in out.stdout.splitlines()]
        assert len(rows) == sum(1 for ln in lines if not ln.startswith("plan")), (len(rows), len(lines))
        return rows
    return run


def make_plan(N, sizes, avgs, chunks_run, filtered=0, num_rendered=None, key_ends=None, chunks_sorted=0, instances_emitted=-1,
              binning_capacity=0):
    """A plan of len(sizes) chunks: chunk c holds sizes[c] Gaussians that may emit sizes[c] * avgs[c] instances."""
    p = N.FramePlan()
    p.num_chunks = len(sizes)
    for c, n in enumerate(sizes):
        p.chunk_rank_begin[c + 1] = p.chunk_rank_begin[c] + n
        p.chunk_instances_max[c] = int(n * avgs[c])
    for c in range(len(sizes), MAXC):
        p.chunk_rank_begin[c + 1] = p.chunk_rank_begin[len(sizes)]
    ends = list(key_ends) if key_ends is not None else [NEAR + 1000 * (c + 1) for c in range(len(sizes))]
    for c in range(MAXC):
        p.chunk_key_end[c] = ends[c] if c < len(sizes) - 1 else KEY_ALL
    p.num_visible = p.chunk_rank_begin[len(sizes)]
    p.num_rendered = sum(p.chunk_instances_max) if num_rendered is None else num_rendered
    p.chunks_run, p.chunks_filtered, p.chunks_sorted = chunks_run, filtered, chunks_sorted
    p.instances_emitted, p.binning_capacity = instances_emitted, binning_capacity
    p.key_max = KEY_ALL
    return p


def plan_line(p):
    return " ".join(str(int(v)) for v in [p.num_rendered, p.num_visible, p.num_chunks, p.chunks_run, p.chunks_filtered, p.chunks_sorted,
                                          p.instances_emitted, p.binning_capacity, p.key_max, *p.chunk_rank_begin, *p.chunk_instances_max,
                                          *p.chunk_key_end])


def hand_made_plans(N):
    big = [3000, 70_000, 200_000]
    out = [make_plan(N, [5000], [30], 0), make_plan(N, [5000], [30], 1),                       # 0 and 1 chunks run
           make_plan(N, big, [400, 40, 9], 1), make_plan(N, big, [400, 40, 9], 0),
           make_plan(N, big, [400, 40, 9], 3, num_rendered=0),                                  # nothing rendered: the chunks do not count
           make_plan(N, [5000], [30], 1, num_rendered=0),
           make_plan(N, big, [400, 40, 9], 2, instances_emitted=123_456, binning_capacity=4_000_000),
           make_plan(N, big, [400, 40, 9], 3, binning_capacity=1000),
           make_plan(N, big[:2], [400, 40], 1)]                                                 # two chunks: the first-chunk capacity is below R
    out += [make_plan(N, big, [400, 40, 9], 3, filtered=m) for m in range(8)]                   # every filtered mask of three chunks
    out += [make_plan(N, big, [400, 40, 9], 2, filtered=m) for m in range(4)]
    return out


def random_plans(N, count, seed):
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        k = rng.randint(1, MAXC)
        sizes = [rng.choice([1, 7, 300, 16_384, 16_385, 65_535, 65_536, 100_000, 1_000_000]) for _ in range(k)]
        avgs = [rng.choice([1, 4, 5, 23, 24, 33, 47, 48, 95, 96, 700, 1024]) for _ in range(k)]
        ends, e = [], rng.choice([NEAR - 5000, NEAR, NEAR + 77])
        for _ in range(k):
            e += rng.randint(1, 1 << 20)
            ends.append(e)
        run = rng.randint(0, k)
        out.append(make_plan(N, sizes, avgs, run, filtered=rng.randrange(1 << k), key_ends=ends, chunks_sorted=rng.randint(0, k),
                             num_rendered=rng.choice([None, None, None, 0]), instances_emitted=rng.choice([-1, -1, 0, 5, 1 << 33]),
                             binning_capacity=rng.choice([0, 0, 1, 1 << 20, 1 << 34])))
    return out


def mutated(fn, old, new, extra=None):
    """A copy of the function `fn` with the one occurrence of `old` in its source replaced by `new`."""
    src = inspect.getsource(fn)
    assert src.count(old) == 1, (fn.__name__, old, src.count(old))
    ns = dict(inspect.getmodule(fn).__dict__)
    ns.update(extra or {})
    exec(src.replace(old, new), ns)
    return ns[fn.__name__]


# ---- the binning path of a chunk: bin_path against binning_ref.chunk_cells ---------------------------------------------------------

def bin_cases():
    """(n, n_max, slab tiles = Tn) on both sides of every edge of launch_chunk_binning's choices; each with filtered and no_gather on
    and off."""
    cases = []
    for avg in (23, 24, 95, 96, 1023, 1024):                       # flat | team1 | team4 | team16, at the top and the bottom of a value
        cases += [(1000, avg * 1000, 50), (1000, avg * 1000 + 999, 50)]
    for n in (1, 16_384, 16_385):                                  # the fused rank scan ends at 16 384 (gathered: 100 n <= 24 n_max)
        cases.append((n, 24 * 16_385, 100))
    for n in ((1 << 26) - 1, 1 << 26):                             # the gather's rank limit (one tile: n <= 24 n_max)
        cases.append((n, 30 * (1 << 26), 1))
    for n_max in ((4 << 20) - 1, 4 << 20):                         # the carried second payload, on a flat chunk (sorted) and a team chunk
        cases += [(200_000, n_max, 64), (40_000, n_max, 1 << 16)]
    for extra in (0, 1):                                           # n slab = 24 n_max + 2^22, and that plus 1
        cases.append((1, 100, 24 * 100 + (1 << 22) + extra))
        cases.append((4096, 175_104, 2050 + 3 * extra))            # (4096 x 2050 = 24 x 175 104 + 2^22; three tiles more: beyond)
    for n_max in (590, 589):                                       # scratch words n_max / 64 + 9 n + 5 = n_max, and one more than n_max
        cases.append((64, n_max, 16))                              # (both flat: see test_selfcheck's note on this bound)
    for Tn in (1, 2, 256, 257, 65_536, 65_537):                    # key bits 1, 1, 8, 9, 16, 17 -> 1, 1, 1, 2, 2, 3 radix passes
        cases += [(1000, 50_000, Tn), (300_000, 5_000_000, Tn)]
    return [(n, n_max, slab, filtered, no_gather) for n, n_max, slab in cases for filtered in (False, True) for no_gather in (False, True)]


def bin_differences(host, N, chunk_cells, cases):
    rows = host([f"bin {n} {n_max} {int(flt)} {slab} {slab} {int(ng)}" for n, n_max, slab, flt, ng in cases])
    bad = []
    for (n, n_max, slab, flt, ng), (flat, team, team_grid, gather, fused, carry, tile_bits, passes, result, gid_emit) in zip(cases, rows):
        plan = make_plan(N, [n], [1], 1, filtered=int(flt))
        plan.chunk_instances_max[0] = n_max
        cell = chunk_cells(plan, slab, 1, 0, 1, no_gather=ng)[0]                 # one tile row of `slab` tiles: Tn = slab
        got = dict(path="flat" if flat else f"team{team}", build=("gather-fused" if fused else "gather-unfused") if gather else "sort",
                   passes=passes, filtered=bool(flt), bbox=not flat)
        if not gather:
            got["carry"] = bool(carry)                                           # (the mirror defines it on the sort path only)
        diff = {k: (v, cell[k]) for k, v in got.items() if cell[k] != v}
        # what the mirror does not name follows from what it does
        ok = (result == passes & 1 and passes == (tile_bits + 7) // 8 and gid_emit == int(bool(carry) and passes % 2 == 0)
              and team_grid == (min(n, 65_536) if flt else n) and (fused <= gather) and not (gather and flat))
        if diff or not ok:
            bad.append(((n, n_max, slab, flt, ng), diff, ok))
    return bad


def test_bin_path_agrees_with_chunk_cells_on_both_sides_of_every_edge(host, native):
    cases = bin_cases()
    assert bin_differences(host, native, BR.chunk_cells, cases) == []
    # the cases reach every cell the mirror can name
    rows = host([f"bin {n} {n_max} {int(flt)} {slab} {slab} {int(ng)}" for n, n_max, slab, flt, ng in cases])
    seen = {("flat" if r[0] else f"team{r[1]}", "gather-fused" if r[4] else "gather-unfused" if r[3] else "sort", r[5] if not r[3] else None, r[7])
            for r in rows}
    assert {s[0] for s in seen} == {"flat", "team1", "team4", "team16"} and {s[1] for s in seen} == {"sort", "gather-fused", "gather-unfused"}
    assert {s[2] for s in seen} == {0, 1, None} and {s[3] for s in seen} == {1, 2, 3}
    print(f"{len(cases)} chunks, {len(seen)} distinct (path, build, carry, passes)")


BIN_MUTATIONS = [("avg < 24", "avg < {}", 24), ("avg >= 1024", "avg >= {}", 1024), ("avg >= 96", "avg >= {}", 96),
                 ("n < (1 << 26)", "n < {}", 1 << 26), ("24 * n_max", "{} * n_max", 24), ("(1 << 22)", "{}", 1 << 22),
                 ("(4 << 20)", "{}", 4 << 20), ("n <= 16384", "n <= {}", 16384), ("(tile_bits + 7)", "(tile_bits + {})", 7)]


def test_selfcheck_a_binning_threshold_moved_by_one_is_found(host, native):
    """Every threshold of a copy of chunk_cells, one up and one down: the comparison reports it.  Not moved: the scratch bound
    (n_max // 64 + 1 + 9 * n + 4 <= n_max).  It cannot decide while chunks are flat below 24 tiles per Gaussian: a team chunk has
    n <= n_max / 24, so its scratch is at most 0.4 n_max + 5 words; the cases at that bound are flat on both sides."""
    cases = bin_cases()
    for old, fmt, value in BIN_MUTATIONS:
        for moved in (value + 1, value - 1):
            bad = bin_differences(host, native, mutated(BR.chunk_cells, old, fmt.format(moved)), cases)
            assert bad, f"{old} -> {fmt.format(moved)} went unnoticed"
    print(f"{2 * len(BIN_MUTATIONS)} moved thresholds, each found")


# ---- the plan's rules: geometry rows, colours, sizes, first-chunk capacity ---------------------------------------------------------

def plan_Ps(N, p):
    """Gaussian counts around the edges a plan has: binned * 4 = P, P - 1 and P + 1 (prefix and effective ranks), 2 V = P and around."""
    base = {max(4 * b + d, 1) for b in (N.binned_prefix(p), N.effective_binned_ranks(p)) for d in (-1, 0, 1)}
    base |= {max(2 * int(p.num_visible) + d, 1) for d in (-1, 0, 1)}
    return sorted(base | {max(int(p.num_visible), 1), 4 * int(p.chunk_rank_begin[1]) + 1, 4 * int(p.chunk_rank_begin[1])})


def first_capacity_ref(p):
    first = int(p.chunk_instances_max[0])
    return min(first + first // 4 + (1 << 20), int(p.num_rendered)) if p.num_chunks > 1 else int(p.num_rendered)


def plan_differences(host, N, plans, geom_variants, effective, prefix, first_capacity):
    lines, checks = [], []
    for p in plans:
        lines += [f"plan {plan_line(p)}", "sizes"]
        checks.append(("sizes", p, None))
        for P in plan_Ps(N, p):
            lines += [f"early {P}", f"geom {P} 0 {P} {prefix(p)} 1", f"geom {P} 0 {P} -1 0", f"geom {P} 1 {P} {prefix(p)} 1"]
            checks += [("early", p, P), ("own", p, P), ("foreign", p, P), ("part", p, P)]
            for c in range(int(p.chunks_run)):
                lines.append(f"colors {p.chunk_rank_begin[c]} {p.chunk_rank_begin[c + 1]} {p.num_visible} {P}")
                checks.append(("colors", p, (P, c)))
    rows = host(lines)
    bad, colours = [], {}
    for (kind, p, arg), row in zip(checks, rows):
        runs = p.num_rendered > 0 and p.chunks_run > 0
        if kind == "sizes":
            cap = int(p.binning_capacity) if p.binning_capacity > 0 else int(p.num_rendered)
            bound = int(p.instances_emitted) if p.instances_emitted >= 0 else sum(p.chunk_instances_max[:p.chunks_run])
            bound = max(bound, 1)
            want = [cap, bound, (max(min(bound, cap), 1) + 15) // 16 * 16, first_capacity(p)]
            if N.binning_first_chunk_capacity(p) != row[3]:                    # the export, which needs no device
                bad.append((kind, "gsr_binning_first_chunk_capacity", row[3]))
        elif kind == "early":
            want = [int(p.num_chunks > 1 and int(p.chunk_rank_begin[1]) * 4 < arg)]
        elif kind == "own":                                                    # a frame's own backward over [0, P)
            own_sparse = bool(runs and effective(p) * 4 < arg)
            sparse = "sparse" in geom_variants(p, arg, False)
            n_ranks = prefix(p)
            want = [effective(p), n_ranks, int(own_sparse), int(sparse), n_ranks if sparse else arg, int(sparse), int(sparse and own_sparse)]
        elif kind == "foreign":                                                # no plan, no rank count: dense
            want = [effective(p), -1, 0, 0, arg, 0, 0]
        elif kind == "part":                                                   # a part of the range: dense, whatever the plan says
            want = [effective(p), prefix(p), 0, 0, arg - 1, 0, 0]
        else:
            P, c = arg
            if p.chunk_rank_begin[c + 1] > p.chunk_rank_begin[c]:
                colours.setdefault((id(p), P), set()).add("k_chunk_colors_all" if row[0] else "k_chunk_colors")
            continue
        if row != want:
            bad.append((kind, plan_line(p), arg, row, want))
    for p in plans:                                                            # the colour kernels of the chunks that ran, per frame
        for P in plan_Ps(N, p):
            want = {k for k in geom_variants(p, P, True) if k.startswith("k_chunk")}
            if colours.get((id(p), P), set()) != want:
                bad.append(("colors", plan_line(p), P, colours.get((id(p), P)), want))
    return bad


def test_plan_rules_agree_with_their_mirrors(host, native):
    N = native
    plans = hand_made_plans(N) + random_plans(N, 200, 11)
    bad = plan_differences(host, N, plans, _geom_variants, N.effective_binned_ranks, N.binned_prefix, N.first_chunk_capacity)
    assert bad == [], bad[:5]
    assert all(N.first_chunk_capacity(p) == first_capacity_ref(p) == N.binning_first_chunk_capacity(p) for p in plans)
    print(f"{len(plans)} plans")


def test_selfcheck_a_plan_threshold_moved_by_one_is_found(host, native):
    N = native
    plans = hand_made_plans(N) + random_plans(N, 40, 12)
    args = dict(geom_variants=_geom_variants, effective=N.effective_binned_ranks, prefix=N.binned_prefix, first_capacity=N.first_chunk_capacity)
    assert plan_differences(host, N, plans, **args) == []
    moved = [dict(geom_variants=mutated(_geom_variants, "own_sparse or binned * 4 < P", "own_sparse or binned * 4 < P + 1")),
             dict(geom_variants=mutated(_geom_variants, "own_sparse or binned * 4 < P", "own_sparse or binned * 4 < P - 1")),
             dict(geom_variants=mutated(_geom_variants, "N.effective_binned_ranks(plan) * 4 < P", "N.effective_binned_ranks(plan) * 4 < P + 1")),
             dict(geom_variants=mutated(_geom_variants, "2 * int(plan.num_visible) >= P", "2 * int(plan.num_visible) >= P + 1")),
             dict(geom_variants=mutated(_geom_variants, "2 * int(plan.num_visible) >= P", "2 * int(plan.num_visible) >= P - 1")),
             dict(geom_variants=mutated(_geom_variants, "r0 == 0 and", "r0 == 1 and")),
             dict(effective=mutated(N.effective_binned_ranks, "if not (int(plan.chunks_filtered) >> c) & 1", "if not (int(plan.chunks_filtered) >> c) & 2")),
             dict(prefix=mutated(N.binned_prefix, "plan.chunk_rank_begin[plan.chunks_run]", "plan.chunk_rank_begin[plan.chunks_run - 1]")),
             dict(first_capacity=mutated(N.first_chunk_capacity, "(1 << 20)", "(1 << 20) + 1")),
             dict(first_capacity=mutated(N.first_chunk_capacity, "first // 4", "first // 5")),
             dict(first_capacity=mutated(N.first_chunk_capacity, "plan.num_chunks > 1", "plan.num_chunks > 2"))]
    for i, m in enumerate(moved):
        assert plan_differences(host, N, plans, **{**args, **m}), f"moved rule {i} ({list(m)[0]}) went unnoticed"
    print(f"{len(moved)} moved rules, each found")


# ---- the live filter and the merge of the remaining chunks -------------------------------------------------------------------------

def filter_ref(c, n, n_max, open_now, slab, off):
    pays = n >= 65_536 and n_max // 32 + 2 * n + 4 <= n_max
    closed = open_now * 2 < slab
    return [int(pays), int(closed), int(c > 0 and pays and closed and not off)]


def merge_ref(p, c, emitted, open_now, stuck, slab, capacity, enabled):
    """What the plan step in front of chunk c does (csrc/gsr_dispatch.h merge_rest), restated: (the program's output line, the plan
    after it)."""
    rb, imax, kend = list(p.chunk_rank_begin), list(p.chunk_instances_max), list(p.chunk_key_end)
    k, last = int(p.num_chunks), int(p.num_chunks) - 1
    status, need, ends, deltas = 0, 0, [0], [0]
    if enabled and 0 < c < last and c >= p.chunks_sorted and stuck > 0 and open_now * 2 < slab:
        m_max, m_n = sum(imax[c:last + 1]), rb[last + 1] - rb[c]
        if m_n >= 65_536 and m_max // 32 + 2 * m_n + 4 <= m_max and m_max <= 0xFFFFFFFF:
            if emitted + m_max > capacity:
                status, need = 2, emitted + m_max
            else:
                base = lambda j: max(kend[j - 1], NEAR)
                ends = [rb[j + 1] - rb[c] for j in range(c, last + 1)]
                deltas = [base(j) - base(c) for j in range(c, last + 1)]
                status, k = 1, c + 1
                rb[c + 1], kend[c], imax[c] = rb[last + 1], kend[last], m_max
    return [status, need, k, rb[c + 1], kend[c], imax[c], len(ends)] + ends + deltas


def merge_cases(N):
    """(plan, c, emitted, open, stuck, slab, capacity, enabled): hand-made plans at every edge of the rule, then random ones."""
    out = []
    slab = 1000
    for rest, avg in ((65_536, 40), (65_535, 40)):                             # the filter's least size, split over two chunks
        p = make_plan(N, [3000, 30_000, rest - 30_000], [400, avg, avg], 1, key_ends=[NEAR - 9, NEAR + 500, 0])
        out.append((p, 1, 77, 499, 1, slab, 1 << 40, True))
    p3 = lambda **kw: make_plan(N, [3000, 70_000, 200_000, 100_000], [400, 40, 9, 3], 1, **kw)
    for open_now, tiles in ((499, 1000), (500, 1000), (499, 999), (500, 1001)):   # open * 2 < slab, by one and by two
        out.append((p3(), 1, 5, open_now, 3, tiles, 1 << 40, True))
    for stuck in (0, 1):
        out.append((p3(), 1, 5, 10, stuck, slab, 1 << 40, True))
    m_max = 70_000 * 40 + 200_000 * 9 + 100_000 * 3
    for capacity in (m_max + 5, m_max + 4):                                    # emitted + m_max > capacity: refused, the plan untouched
        out.append((p3(), 1, 5, 10, 1, slab, capacity, True))
    out.append((p3(), 1, 5, 10, 1, slab, 1 << 40, False))                      # switched off
    out.append((p3(chunks_sorted=2), 1, 5, 10, 1, slab, 1 << 40, True))       # a re-run: chunk 1 is sorted already
    out.append((p3(chunks_sorted=2), 2, 5, 10, 1, slab, 1 << 40, True))
    out.append((p3(), 0, 0, 10, 1, slab, 1 << 40, True))                       # never in front of the first chunk
    out.append((p3(), 3, 5, 10, 1, slab, 1 << 40, True))                       # nor of the last
    # m_max / 32 + 2 n + 4 <= m_max at its edge: n = 65 536 Gaussians in two chunks, bounds that sum to B and B - 1
    B = next(b for b in range(2 * 65_536, 3 * 65_536) if b // 32 + 2 * 65_536 + 4 <= b)
    for total in (B, B - 1):
        p = make_plan(N, [3000, 30_000, 35_536], [400, 1, 1], 1)
        p.chunk_instances_max[1], p.chunk_instances_max[2] = 30_000, total - 30_000
        out.append((p, 1, 0, 10, 1, slab, 1 << 40, True))
    for total in (0xFFFFFFFF, 0x100000000):                                    # the merged bound fits 32 bits, or not
        p = make_plan(N, [3000, 300_000, 400_000], [400, 1, 1], 1)
        p.chunk_instances_max[1], p.chunk_instances_max[2] = 1 << 31, total - (1 << 31)
        out.append((p, 1, 0, 10, 1, slab, 1 << 40, True))
    rng = random.Random(5)
    for p in random_plans(N, 150, 13):
        for c in range(0, min(int(p.num_chunks), MAXC - 1)):
            m_max = sum(p.chunk_instances_max[c:p.num_chunks])
            out.append((p, c, rng.choice([0, 1000]), rng.choice([0, 499, 500, 0xFFFFFFFF]), rng.choice([0, 1, 50]), slab,
                        rng.choice([1 << 40, m_max + 1000, m_max + 999, m_max]), rng.random() < 0.9))
    return out


def merge_differences(host, cases, ref):
    lines = []
    for p, c, emitted, open_now, stuck, slab, capacity, enabled in cases:
        lines += [f"plan {plan_line(p)}", f"merge {c} {emitted} {open_now} {stuck} {slab} {capacity} {int(enabled)}"]
    rows = host(lines)
    return [(plan_line(case[0]), case[1:], row, ref(*case)) for case, row in zip(cases, rows) if row != ref(*case)]


def test_merge_rest_and_live_filter_agree_with_their_restatement(host, native):
    cases = merge_cases(native)
    assert merge_differences(host, cases, merge_ref) == []
    status = [merge_ref(*case)[0] for case in cases]
    assert all(status.count(s) >= 5 for s in (0, 1, 2)), [status.count(s) for s in (0, 1, 2)]
    # the filter's own test: both of its parts at their edges, in front of the first chunk, switched off
    B = next(b for b in range(2 * 65_536, 3 * 65_536) if b // 32 + 2 * 65_536 + 4 <= b)
    fc = [(c, n, n_max, open_now, tiles, off) for c in (0, 1) for n, n_max in ((65_536, B), (65_536, B - 1), (65_535, B), (1_000_000, 30_000_000))
          for open_now, tiles in ((499, 1000), (500, 1000), (499, 999), (0xFFFFFFFF, 1000)) for off in (0, 1)]
    rows = host([f"filter {c} {n} {n_max} {o} {slab} {off}" for c, n, n_max, o, slab, off in fc])
    assert rows == [filter_ref(*case) for case in fc]
    # ... and the three one-line rules that have no mirror of their own, at their edges
    lines = [f"small {n} {n_max} {f}" for n, n_max, f in ((2, 8, 0), (2, 9, 0), (2, 8, 1), (0, 0, 0))]
    lines += [f"wide {n} {n_max} {f}" for n, n_max, f in ((10, 479, 0), (10, 480, 0), (10, 480, 1))]
    lines += [f"order {n} {f}" for n, f in ((16_384, 0), (16_385, 0), (16_384, 1))]
    assert host(lines) == [[1], [0], [0], [0], [0], [1], [0], [1], [0], [0]]
    print(f"{len(cases)} merge steps ({status.count(1)} merged, {status.count(2)} refused), {len(fc)} filter decisions")


def test_selfcheck_a_merge_threshold_moved_by_one_is_found(host, native):
    cases = merge_cases(native)
    extra = {"NEAR": NEAR}
    for old, new in (("m_n >= 65_536", "m_n >= 65_537"), ("m_n >= 65_536", "m_n >= 65_535"), ("open_now * 2 < slab", "open_now * 2 < slab + 1"),
                     ("open_now * 2 < slab", "open_now * 2 < slab - 1"), ("2 * m_n + 4 <= m_max", "2 * m_n + 5 <= m_max"),
                     ("2 * m_n + 4 <= m_max", "2 * m_n + 3 <= m_max"), ("emitted + m_max > capacity", "emitted + m_max > capacity + 1"),
                     ("emitted + m_max > capacity", "emitted + m_max >= capacity"), ("m_max <= 0xFFFFFFFF", "m_max <= 0xFFFFFFFE"),
                     ("m_max <= 0xFFFFFFFF", "m_max <= 0x100000000"), ("stuck > 0", "stuck > 1"), ("0 < c < last", "0 < c <= last"),
                     ("0 < c < last", "0 <= c < last"), ("c >= p.chunks_sorted", "c > p.chunks_sorted"), ("max(kend[j - 1], NEAR)", "max(kend[j - 1], NEAR + 1)")):
        assert merge_differences(host, cases, mutated(merge_ref, old, new, extra)), f"{old} -> {new} went unnoticed"
