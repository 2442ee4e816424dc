"""Sparse Adam against the dense step, on the GPU, in one process (DESIGN.md section 14 holds the table this prints).

Step legs: the five tensors of a degree-3 model ([P,3] [P,16,3] [P,1] [P,3] [P,4]) at P = 1 M (cfg3's store) and 5 M (cfg5n's);
FusedAdam.step() and SparseFusedAdam.step(mask) alternate, each timed with device events around enough steps to fill --window
seconds, --repeats times.  Visible fractions 1, 0.5, 0.1, 0.01, each as a random mask and as one contiguous run.  Bytes come from
the model of DESIGN.md section 14, computed here from the shapes and the mask: dense 28 B per element; sparse 28 B per element of
every 128-byte line that holds at least one visible row, plus the mask bytes (an upper estimate).

Training legs (--train-iters, 0 = skip): train_loop.train on cfg3 as bench.py --full --train-loop sets it up, once with the default
optimizer and once with optimizer_type = "sparse_adam", on the arc cameras (which keep most of the cloud in the frustum) and on the
same arc with a narrow field of view (a minority of the cloud)."""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd")]
import torch  # noqa: E402

LINE_FLOATS = 32            # a 128-byte line


def shapes(P, M=16):
    return [(P, 3), (P, M, 3), (P, 1), (P, 3), (P, 4)]


def dense_bytes(P, M=16):
    return 28 * sum(P * (s[1] if len(s) == 2 else s[1] * s[2]) for s in shapes(P, M))


def sparse_bytes(mask, M=16, mask_elem_bytes=1):
    """The bytes model: per tensor of width w, the elements of every 128-byte line with a visible row under it, times 28 B; plus the
    mask.  Tensors start on a line (the allocator's alignment)."""
    P = mask.shape[0]
    seen_before = torch.cat((torch.zeros(1, dtype=torch.int64, device=mask.device), mask.to(torch.int64).cumsum(0)))
    total = P * mask_elem_bytes
    for s in shapes(P, M):
        w = s[1] if len(s) == 2 else s[1] * s[2]
        n = P * w
        lines = torch.arange((n + LINE_FLOATS - 1) // LINE_FLOATS, dtype=torch.int64, device=mask.device)
        first, last = lines * LINE_FLOATS, torch.clamp(lines * LINE_FLOATS + LINE_FLOATS - 1, max=n - 1)
        touched = seen_before[last // w + 1] - seen_before[first // w] > 0
        total += 28 * int((last - first + 1)[touched].sum())
    return total


def make_mask(P, fraction, layout, gen, dev):
    if fraction >= 1.0:
        return torch.ones(P, dtype=torch.bool, device=dev)
    if layout == "random":
        return (torch.rand(P, generator=gen) < fraction).to(dev)
    m = torch.zeros(P, dtype=torch.bool, device=dev)
    n = int(round(P * fraction))
    a = (P - n) // 3 | 1                       # an odd start: the run's ends fall inside float4s of the narrow tensors
    m[a:a + n] = True
    return m


def timed_steps(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n          # seconds per step


def step_legs(P, dev, window, repeats, fractions):
    from fused_adam import FusedAdam, SparseFusedAdam
    gen = torch.Generator().manual_seed(P)
    names = ("xyz", "f_dc", "opacity", "scaling", "rotation")

    def build(cls):
        ps = [torch.randn(s, device=dev).requires_grad_(True) for s in shapes(P)]
        groups = []
        for name, p in zip(names, ps):
            groups.append({"params": [p], "lr": 1e-4, "name": name, **({"head_cols": 1, "tail": "f_rest"} if name == "f_dc" else {})})
            if name == "f_dc":
                groups.append({"params": [], "lr": 5e-6, "name": "f_rest"})
        return ps, cls(groups, lr=0.0, eps=1e-15)
    (dp, dense), (sp, sparse) = build(FusedAdam), build(SparseFusedAdam)
    for p in dp + sp:
        p.grad = torch.randn_like(p) * 1e-3
    dense_step = lambda: dense.step()
    for _ in range(5):                           # warm-up: code objects, the moments' allocation
        dense_step()
        sparse.step(visibility=torch.ones(P, dtype=torch.bool, device=dev))
    torch.cuda.synchronize()
    rows, dense_all = [], []
    for layout in ("random", "run"):
        for f in fractions:
            mask = make_mask(P, f, layout, gen, dev)
            sparse_step = lambda: sparse.step(visibility=mask)
            nd = max(3, int(window / timed_steps(dense_step, 5)))
            ns = max(3, int(window / timed_steps(sparse_step, 5)))
            td, ts = [], []
            for _ in range(repeats):             # alternating legs
                td.append(timed_steps(dense_step, nd))
                ts.append(timed_steps(sparse_step, ns))
            dense_all += td
            bd, bs = dense_bytes(P), sparse_bytes(mask)
            t_d, t_s = sorted(td)[len(td) // 2], sorted(ts)[len(ts) // 2]
            rows.append({"P": P, "mask": layout, "fraction": f, "visible_rows": int(mask.sum()),
                         "dense_us": round(1e6 * t_d, 1), "dense_us_min_max": [round(1e6 * min(td), 1), round(1e6 * max(td), 1)],
                         "sparse_us": round(1e6 * t_s, 1), "sparse_us_min_max": [round(1e6 * min(ts), 1), round(1e6 * max(ts), 1)],
                         "dense_model_bytes": bd, "sparse_model_bytes": bs, "model_bytes_ratio": round(bs / bd, 4),
                         "time_ratio": round(t_s / t_d, 4), "dense_TBps": round(bd / t_d * 1e-12, 3),
                         "sparse_model_TBps": round(bs / t_s * 1e-12, 3), "steps_per_window": [nd, ns]})
            print(json.dumps(rows[-1]), flush=True)
    spread = {"P": P, "dense_windows": len(dense_all), "dense_us_min": round(1e6 * min(dense_all), 1),
              "dense_us_max": round(1e6 * max(dense_all), 1), "dense_spread_percent": round(100 * (max(dense_all) / min(dense_all) - 1), 2)}
    print(json.dumps(spread), flush=True)
    del dense, sparse, dp, sp
    gc.collect()
    torch.cuda.empty_cache()
    return rows, spread


def train_legs(iters, dev, tanfovy, label):
    """cfg3 as bench.py's --train-loop leg: 8 arc cameras, targets from a second cloud, densification every 100 iterations."""
    from dataclasses import replace

    import scene_synth as S
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    cfg = S.CONFIGS["cfg3"]
    cams = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], 8, tanfovy=tanfovy)]
    bg = torch.zeros(3, device=dev)
    truth = GaussianModel(cfg["D"])
    truth.adopt_scene(S.make_scene(cfg["P"], cfg["W"], cfg["H"], cfg["D"], 30), device=dev)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    del truth
    out = {"cameras": label, "tanfovy": tanfovy, "iterations": iters}
    warm = 20
    for kind in ("default", "sparse_adam", "default", "sparse_adam"):       # twice each, alternating: the second pair is reported
        gm = GaussianModel(cfg["D"])
        gm.adopt_scene(S.make_config("cfg3")[0], device=dev)
        opt = replace(OptimizationDefaults(), densify_from_iter=0, optimizer_type=kind)
        gm.training_setup(opt)
        with torch.no_grad():
            seen = [float((render(c, gm, Pipe(), bg)["radii"] > 0).float().mean()) for c in cams]
        out["visible_fraction_start_mean"] = round(sum(seen) / len(seen), 4)
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm, scene_extent=6.0)
        gc.collect()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm + iters, first_iter=warm + 1, scene_extent=6.0)
        torch.cuda.synchronize(dev)
        ms = 1e3 * (time.perf_counter() - t0) / iters
        out.setdefault(kind + "_ms_per_it_runs", []).append(round(ms, 3))
        out[kind + "_gaussians_end"] = int(gm._xyz.shape[0])
        with torch.no_grad():
            seen = [float((render(c, gm, Pipe(), bg)["radii"] > 0).float().mean()) for c in cams]
        out[kind + "_visible_fraction_end_mean"] = round(sum(seen) / len(seen), 4)
        del gm
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1_000_000, 5_000_000])
    ap.add_argument("--fractions", type=float, nargs="*", default=[1.0, 0.5, 0.1, 0.01])
    ap.add_argument("--window", type=float, default=0.3, help="seconds of steps per timed window")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--train-iters", type=int, default=300, help="iterations of each training leg (0: skip them)")
    ap.add_argument("--narrow-tanfovy", type=float, default=0.15, help="tan(fovy / 2) of the narrow-view training leg (cfg3: 0.5)")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_adam_bench.py measures on the GPU: no device found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "steps": [], "dense_spread": [], "train": []}
    for P in a.sizes:
        rows, spread = step_legs(P, dev, a.window, a.repeats, a.fractions)
        result["steps"] += rows
        result["dense_spread"].append(spread)
    if a.train_iters > 0:
        result["train"].append(train_legs(a.train_iters, dev, 0.5, "cfg3 arc (bench.py --train-loop)"))
        result["train"].append(train_legs(a.train_iters, dev, a.narrow_tanfovy, "cfg3 arc, narrow field of view"))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({"sparse_adam_bench": "done", "rows": len(result["steps"]), "train_legs": len(result["train"])}))


if __name__ == "__main__":
    main()
