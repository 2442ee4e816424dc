"""The bilateral grid's launches on the GPU, in one process (DESIGN.md section 17 holds the table this prints).

Kernel legs at 1080p and 4K with the default grid [N, 12, 8, 16, 16] (--images grids), each the median of --repeats alternated
windows timed with device events:
  forward     gsr_bilagrid_forward against bilagrid.slice_apply_torch (grid_sample on a 5-D input and the affine product), in us and
              as a share of the HBM rate from the 24 B / pixel model (12 B read, 12 B written)
  fwd + bwd   forward, then both gradients from a fixed upstream, native against torch autograd (48 B / pixel of images beside the
              partial sums: 12 + 12 forward, 24 read and 12 written backward, less what the cache keeps)
  tv          total_variation_loss forward + backward, native against the torch ops
Training legs (--train-iters, 0 = skip): train_loop.train on cfg3 and cfg3n as bench.py --train-loop sets them up, densification
off, opt.bilateral_grid off against on, twice each, alternating; ms per iteration.  --profile adds one pass of the "on" leg under
the library's per-kernel events (gsr_profile_enable) and prints the bilateral grid's kernels' ms per iteration."""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd")]
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # float4 copy rate of the part
FWD_BYTES = 24                     # per pixel


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternated(fns, window, repeats):
    """{name: (median, min, max) seconds per call} of the callables, their windows alternating."""
    counts = {k: max(3, int(window / timed(f, 3))) for k, f in fns.items()}
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            runs[k].append(timed(f, counts[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in runs.items()}


def us(t):
    return {"us": round(1e6 * t[0], 1), "us_min_max": [round(1e6 * t[1], 1), round(1e6 * t[2], 1)]}


def pair(t):
    return {"native": us(t["native"]), "torch": us(t["torch"]), "speedup": round(t["torch"][0] / t["native"][0], 2)}


def kernel_legs(H, W, N, dev, window, repeats):
    from diff_gaussian_rasterization import bilagrid
    gen = torch.Generator().manual_seed(H)
    eye = torch.eye(4)[:3].reshape(1, 12, 1, 1, 1)
    grids = (eye + 0.3 * torch.randn(N, 12, 8, 16, 16, generator=gen)).to(dev).requires_grad_(True)
    image = (torch.rand(3, H, W, generator=gen) * 1.3 - 0.1).to(dev).requires_grad_(True)
    go = torch.randn(3, H, W, generator=gen).to(dev)
    idx = N // 2
    out = {"H": H, "W": W, "N": N}

    def fwd(native):
        def f():
            with torch.no_grad():
                bilagrid.slice_apply(grids, image, idx, native=native)
        return f

    def both(native):
        def f():
            grids.grad = image.grad = None
            bilagrid.slice_apply(grids, image, idx, native=native).backward(go)
        return f

    def tv(native):
        def f():
            grids.grad = None
            bilagrid.total_variation_loss(grids, native=native).backward()
        return f
    for name, make in (("forward", fwd), ("forward_backward", both), ("tv_forward_backward", tv)):
        fns = {"native": make(True), "torch": make(False)}
        for f in fns.values():
            f()
        out[name] = pair(alternated(fns, window, repeats))
        if name == "forward":
            t = out[name]["native"]["us"] * 1e-6
            out[name]["native_TBps"] = round(FWD_BYTES * H * W / t * 1e-12, 3)
            out[name]["native_share_of_hbm_rate"] = round(FWD_BYTES * H * W / t / HBM_BYTES_PER_S, 3)
        print(json.dumps({f"{H}x{W}": {name: out[name]}}), flush=True)
    return out


def train_legs(cfg_name, iters, dev, profile):
    from dataclasses import replace

    from diff_gaussian_rasterization import _native

    import scene_synth as S
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    cfg = S.CONFIGS[cfg_name]
    cams = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], 8)]
    bg = torch.zeros(3, device=dev)
    truth = GaussianModel(cfg["D"])
    truth.adopt_scene(S.make_config(cfg_name)[0], device=dev)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    del truth
    out = {"config": cfg_name, "iterations": iters}
    warm = 20
    for kind, profiled in [(k, False) for k in ("off", "on") * 2] + ([("on", True)] if profile else []):
        gm = GaussianModel(cfg["D"])
        gm.adopt_scene(S.make_config(cfg_name)[0], device=dev)
        opt = replace(OptimizationDefaults(), densify_from_iter=10 ** 9, densify_until_iter=0, bilateral_grid=kind == "on")
        gm.training_setup(opt)
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm, scene_extent=6.0)
        gc.collect()
        torch.cuda.synchronize(dev)
        if profiled:
            _native.profile_enable(True)
        t0 = time.perf_counter()
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm + iters, first_iter=warm + 1, scene_extent=6.0,
              bilagrid=getattr(gm, "bilagrid", None))
        torch.cuda.synchronize(dev)
        ms = round(1e3 * (time.perf_counter() - t0) / iters, 3)
        if profiled:
            prof = _native.profile_read(64)
            _native.profile_enable(False)
            out["on_profiled"] = {"ms_per_it": ms, "bilagrid_kernel_ms_per_it": {k: round(v[0] / iters, 4) for k, v in prof.items()
                                                                                  if k.startswith("bilagrid")}}
        else:
            out.setdefault(kind + "_ms_per_it_runs", []).append(ms)
        del gm
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps({"train": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8, help="grids in the tensor (N)")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-iters", type=int, default=200, help="iterations of each training leg (0: skip them)")
    ap.add_argument("--profile", action="store_true", help="also one training pass with the grid under the library's per-kernel events")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bilagrid_bench.py measures on the GPU: no device found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0),
              "kernels": [kernel_legs(H, W, a.images, dev, a.window, a.repeats) for H, W in ((1080, 1920), (2160, 3840))]}
    if a.train_iters > 0:
        result["train"] = [train_legs(c, a.train_iters, dev, a.profile) for c in ("cfg3", "cfg3n")]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({"bilagrid_bench": "done"}))


if __name__ == "__main__":
    main()
