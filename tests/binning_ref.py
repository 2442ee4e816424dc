"""Exact host reference of the progressive tile binning, and the checker that holds the device's lists to it.

The enumeration and the comparison run in C++ (tests/host_harness.cpp: hh_bin_reference, hh_bin_check), compiled without FMA
contraction: a cfg5n frame has ~23 M instances.  The reference reads the device's own per-Gaussian state (records, depth order,
chunk plan), so what it tests is the binning: which (Gaussian, tile) instances each chunk emits, in which order, with which
quadrant bits, and where the ranges put them.

Tolerance.  The device contracts to FMA and this reference does not, so a culling decision right at its cut-off may go either
way.  Every decision reports its margin (distance to the cut-off relative to the magnitudes that enter it); the device may decide
it differently only where that margin is <= TOL.  Those boundary mismatches are counted and capped (boundary_cap); any other
difference is a fault.

Also here: a Python mirror of the per-chunk dispatch of launch_chunk_binning (csrc/gsr_binning.hip) and of the live-filter
rule (csrc/gsr_api.hip), which names the path ("cell") each chunk took.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-5                       # relative decision margin inside which host and device may disagree
MAX_CHUNKS = 8
FAULTS = ("list", "quad", "range", "closed")


def boundary_cap(n_instances: int) -> int:
    return 8 + int(1e-6 * n_instances)


def build_harness(out_dir: str) -> C.CDLL:
    """tests/host_harness.cpp as a shared library: g++ (else ROCm's clang++), no FMA contraction."""
    cxx = shutil.which("g++") or next((p for p in ("/opt/rocm/llvm/bin/clang++", shutil.which("clang++")) if p and os.path.exists(p)), None)
    assert cxx, "no host C++ compiler"
    so = os.path.join(out_dir, "libhost_harness_bin.so")
    subprocess.check_call([cxx, "-O2", "-fPIC", "-shared", "-std=c++17", "-ffp-contract=off", "-o", so,
                           os.path.join(HERE, "host_harness.cpp")])
    lib = C.CDLL(so)
    lib.hh_bin_reference.restype = C.c_int64
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def reference(hh, Gx, Gy, ty0, ty1, rec, order, rank_begin, bbox, tol=TOL) -> dict:
    """Expected per-(chunk, tile) lists.  rec [P, 12] float32 device records; order the depth order; rank_begin [n_chunks + 1];
    bbox[c]: chunk c's quadrant bits come from quadrant_mask_bbox (team and gather paths), else quadrant_mask_q (flat)."""
    rec = np.ascontiguousarray(rec, np.float32)
    order = np.ascontiguousarray(order, np.int32)
    rb = np.ascontiguousarray(rank_begin, np.int32)
    n_chunks = rb.size - 1
    bb = np.ascontiguousarray(np.asarray(bbox, np.uint8).reshape(n_chunks))
    n = hh.hh_bin_reference(Gx, Gy, ty0, ty1, rec.shape[0], _p(rec), _p(order), n_chunks, _p(rb), _p(bb), C.c_float(tol))
    offs = np.zeros(n_chunks * Gx * Gy + 1, np.int64)
    gid, quad, flags, margin = np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.float32)
    hh.hh_bin_reference_get(_p(offs), _p(gid), _p(quad), _p(flags), _p(margin))
    return dict(offs=offs, gid=gid, quad=quad, flags=flags, margin=margin, n_chunks=n_chunks, Tn=Gx * Gy)


def ref_list(ref, c, t):
    """(gid, quad, flags) of the expected list of chunk c, tile t."""
    i = c * ref["Tn"] + t
    a, b = ref["offs"][i], ref["offs"][i + 1]
    return ref["gid"][a:b], ref["quad"][a:b], ref["flags"][a:b]


def last_chunk_per_tile(n_contrib_enc, W, H):
    """Largest chunk holding the last contributor of a pixel of each tile (-1: none).  last_enc = (chunk + 1) << 26 | position."""
    enc = np.asarray(n_contrib_enc, np.int64)
    c = (enc >> 26) - 1
    Gx, Gy = (W + 15) // 16, (H + 15) // 16
    pad = np.full((Gy * 16, Gx * 16), -1, np.int64)
    pad[:H, :W] = c
    return pad.reshape(Gy, 16, Gx, 16).max(axis=(1, 3)).reshape(-1).astype(np.int32)


def check(hh, ranges, words, t_begin, t_end, last_chunk=None) -> dict:
    """Compares device ranges [n_chunks, Tn, 2] and words (Gaussian | quadrant mask << 28) with the reference held by the last
    reference() call.  Returns counts: compared, faults by kind (FAULTS), boundary mismatches, closed tiles, first fault."""
    rng = np.ascontiguousarray(ranges, np.uint32)
    w = np.ascontiguousarray(words, np.uint32)
    lc = None if last_chunk is None else np.ascontiguousarray(last_chunk, np.int32)
    st = np.zeros(12, np.int64)
    mm = C.c_float(0.0)
    hh.hh_bin_check(_p(rng), _p(w) if w.size else None, C.c_int64(w.size), int(t_begin), int(t_end), None if lc is None else _p(lc),
                    _p(st), C.byref(mm))
    rep = dict(compared=int(st[0]), list=int(st[1]), quad=int(st[2]), range=int(st[3]), closed=int(st[4]),
               boundary_in=int(st[5]), boundary_quad=int(st[6]), closed_tiles=int(st[7]), lists=int(st[8]), emitted=int(st[9]),
               max_margin=float(mm.value), first_fault=None)
    if st[10] >= 0:
        Tn = rng.shape[1]
        rep["first_fault"] = (FAULTS[int(st[11]) - 1], int(st[10]) // Tn, int(st[10]) % Tn)
    return rep


def assert_clean(rep, label=""):
    faults = {k: rep[k] for k in FAULTS if rep[k]}
    assert not faults, f"{label}: binning faults {faults}, first {rep['first_fault']}"
    nb = rep["boundary_in"] + rep["boundary_quad"]
    assert nb <= boundary_cap(rep["compared"]), f"{label}: {nb} boundary mismatches > cap {boundary_cap(rep['compared'])}"


def check_depth_order(rec, order, rank_begin, key_end, chunks_run, filtered_mask, V):
    """Chunks partition the visible keys by chunk_key_end; every binned chunk is strictly sorted by (key, index) — a filtered
    chunk only in its live front part, so there it is checked as a permutation of its keys' range."""
    keys = np.asarray(rec)[:, 9].view(np.uint32).astype(np.int64)
    order = np.asarray(order, np.int64)
    assert np.unique(order[:V]).size == V
    for c in range(len(rank_begin) - 1):
        b0, b1 = int(rank_begin[c]), int(rank_begin[c + 1])
        k = keys[order[b0:b1]]
        lo = int(key_end[c - 1]) if c else -1
        assert b1 > b0 and k.min() > lo and k.max() <= int(key_end[c]), c
        if c < chunks_run and not (filtered_mask >> c) & 1:
            ck = k * (1 << 32) + order[b0:b1]
            assert np.all(np.diff(ck) > 0), f"chunk {c} not strictly sorted by (key, index)"


# ---- the dispatch of launch_chunk_binning, restated
def chunk_cells(plan, Gx, Gy, ty0, ty1, no_gather=False):
    """One dict per chunk that ran: n, n_max, path (flat | team1 | team4 | team16), list build (sort | gather-fused |
    gather-unfused), carried gid and sort passes, filtered, merged."""
    Tn = Gx * Gy
    tile_bits = max(int(Tn - 1).bit_length(), 1)
    passes = (tile_bits + 7) // 8
    slab = (ty1 - ty0) * Gx
    out = []
    for c in range(plan.chunks_run):
        n = int(plan.chunk_rank_begin[c + 1]) - int(plan.chunk_rank_begin[c])
        n_max = int(plan.chunk_instances_max[c])
        filtered = bool((plan.chunks_filtered >> c) & 1)
        avg = n_max // n
        flat = avg < 24 and not filtered
        team = 1 if filtered else 16 if avg >= 1024 else 4 if avg >= 96 else 1
        scratch = n_max // 64 + 1 + 9 * n + 4
        gather = (not flat and not filtered and not no_gather and n < (1 << 26) and n * slab <= 24 * n_max + (1 << 22)
                  and scratch <= n_max)
        carry = n_max >= (4 << 20) and not gather
        # a merged chunk (gsr_api.hip) is the last one; the plan keeps the planned chunks' bounds behind it
        merged = (filtered and c == plan.num_chunks - 1 and plan.num_chunks < MAX_CHUNKS
                  and int(plan.chunk_instances_max[plan.num_chunks]) > 0)
        out.append(dict(c=c, n=n, n_max=n_max, path="flat" if flat else f"team{team}",
                        build=("gather-fused" if n <= 16384 else "gather-unfused") if gather else "sort",
                        carry=carry, passes=passes, filtered=filtered, merged=merged, bbox=not flat))
    return out


def cell_names(cell, slab=False):
    """The coverage cells one chunk reaches."""
    names = {cell["path"], cell["build"], f"{cell['path']}/{cell['build']}"}
    if cell["build"] == "sort":
        names.add(f"carry-{cell['passes']}pass" if cell["carry"] else "sort-gather-table")
    if cell["filtered"]:
        names.add("filtered")
    if cell["merged"]:
        names.add("merged")
    if slab:
        names.add("slab")
    return names
