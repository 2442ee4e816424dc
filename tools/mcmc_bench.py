"""The MCMC strategy's launches on the GPU, in one process (DESIGN.md section 16 holds the table this prints).

Kernel legs at P = 1 M (--size), each the median of --repeats alternated windows timed with device events:
  noise       gsr_mcmc_inject_noise against the torch composition of the same rule (mcmc.position_noise_torch + add_), in us and as
              a share of the HBM rate from the 68 B / Gaussian model (56 B read, 12 B written)
  reg grads   gsr_mcmc_reg_grads against the same torch ops (48 B / Gaussian: 16 B of raw tensors and 16 B of gradients read, 16 B written)
  relocation  compute_relocation + relocate_rows over the model's five tensors with moments, n = 1 % and 10 % of P
Training legs (--train-iters, 0 = skip): train_loop.train on cfg3 as bench.py --train-loop sets it up, densify_from_iter = 0,
strategy "default" against "mcmc" (mcmc_cap_max = 1.05 x the starting P) and against "mcmc" with both lambdas and the noise scale at
zero (the same launches on a scene that evolves without them), twice each, alternating; ms per iteration.  --profile adds one pass
per leg under the library's per-kernel events (gsr_profile_enable) and prints the largest kernels' ms per iteration."""
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
NOISE_BYTES, REG_BYTES = 68, 48    # per Gaussian


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


def kernel_legs(P, dev, window, repeats):
    from diff_gaussian_rasterization import mcmc
    gen = torch.Generator().manual_seed(P)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    xyz, scaling, rotation = r(P, 3), r(P, 3) * 1.5 - 4.0, r(P, 4)
    opacity = (torch.rand(P, 1, generator=gen) * 12 - 8).to(dev)          # o from 3e-4 to 0.98: the gate is open on about a third
    noise = r(P, 3)
    out = {"P": P}
    c = 5e5 * 1.6e-4

    def native_noise():
        mcmc.inject_position_noise(xyz, scaling, rotation, opacity, noise, c)

    def torch_noise():
        xyz.add_(mcmc.position_noise_torch(scaling, rotation, opacity, noise, c))
    for f in (native_noise, torch_noise):
        f()
    t = alternated({"native": native_noise, "torch": torch_noise}, window, repeats)
    out["noise"] = {"native": us(t["native"]), "torch": us(t["torch"]), "speedup": round(t["torch"][0] / t["native"][0], 2),
                    "model_bytes": NOISE_BYTES * P, "native_TBps": round(NOISE_BYTES * P / t["native"][0] * 1e-12, 3),
                    "native_share_of_hbm_rate": round(NOISE_BYTES * P / t["native"][0] / HBM_BYTES_PER_S, 3)}
    print(json.dumps({"noise": out["noise"]}), flush=True)

    g_o, g_s = torch.zeros(P, 1, device=dev), torch.zeros(P, 3, device=dev)

    def native_reg():
        mcmc.add_regularizer_grads(opacity, scaling, 0.01, 0.01, g_o, g_s)

    def torch_reg():
        mcmc.add_regularizer_grads(opacity, scaling, 0.01, 0.01, g_o, g_s, native=False)
    for f in (native_reg, torch_reg):
        f()
    t = alternated({"native": native_reg, "torch": torch_reg}, window, repeats)
    out["reg_grads"] = {"native": us(t["native"]), "torch": us(t["torch"]), "speedup": round(t["torch"][0] / t["native"][0], 2),
                        "model_bytes": REG_BYTES * P, "native_TBps": round(REG_BYTES * P / t["native"][0] * 1e-12, 3),
                        "native_share_of_hbm_rate": round(REG_BYTES * P / t["native"][0] / HBM_BYTES_PER_S, 3)}
    print(json.dumps({"reg_grads": out["reg_grads"]}), flush=True)

    features = r(P, 16, 3)
    tensors = [(p, torch.zeros_like(p), torch.zeros_like(p), role) for p, role in
               ((xyz, "copy"), (features, "copy"), (opacity, "opacity"), (scaling, "scaling"), (rotation, "copy"))]
    out["relocation"] = []
    for share in (0.01, 0.1):
        n = int(P * share)
        perm = torch.randperm(P, generator=gen)
        dead, alive = perm[:n].to(dev), perm[n:].to(dev)
        sampled = alive[torch.randint(0, P - n, (n,), generator=gen).to(dev)]
        state = {}

        def rule():
            state["new"] = mcmc.compute_relocation(opacity, scaling, sampled, 0.005)

        def rows():
            mcmc.relocate_rows(tensors, sampled, dead, *state["new"])
        rule()
        rows()
        t = alternated({"rule": rule, "rows": rows}, window, repeats)
        row_bytes = n * (4 * (59 + 59 + 4 + 2 * 59) + 16)     # per relocated row: 59 floats read, 59 written to the dead row, 4 to the source, 2 x 59 of moments zeroed; two indices
        out["relocation"].append({"n": n, "share_of_P": share, "rule": us(t["rule"]), "rows": us(t["rows"]),
                                  "rows_model_bytes": row_bytes, "rows_TBps": round(row_bytes / t["rows"][0] * 1e-12, 3)})
        print(json.dumps({"relocation": out["relocation"][-1]}), flush=True)
    return out


LEGS = {"default": dict(densify_strategy="default"), "mcmc": dict(densify_strategy="mcmc"),
        "mcmc_inert": dict(densify_strategy="mcmc", mcmc_opacity_reg=0.0, mcmc_scale_reg=0.0, mcmc_noise_lr=0.0)}


def train_legs(iters, dev, profile):
    from dataclasses import replace

    from diff_gaussian_rasterization import _native

    import scene_synth as S
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, OptimizationDefaults
    from train_loop import train
    cfg = S.CONFIGS["cfg3"]
    cams = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], 8)]
    bg = torch.zeros(3, device=dev)
    truth = GaussianModel(cfg["D"])
    truth.adopt_scene(S.make_scene(cfg["P"], cfg["W"], cfg["H"], cfg["D"], 30), device=dev)
    with torch.no_grad():
        targets = [render(c, truth, Pipe(), bg)["render"].clone() for c in cams]
    del truth
    out = {"iterations": iters, "P_start": cfg["P"]}
    warm = 20
    for kind, profiled in [(k, False) for k in tuple(LEGS) * 2] + [(k, True) for k in LEGS if profile]:
        gm = GaussianModel(cfg["D"])
        gm.adopt_scene(S.make_config("cfg3")[0], device=dev)
        opt = replace(OptimizationDefaults(), densify_from_iter=0, mcmc_cap_max=int(1.05 * cfg["P"]), **LEGS[kind])
        gm.training_setup(opt)
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm, scene_extent=6.0)
        gc.collect()
        torch.cuda.synchronize(dev)
        if profiled:
            _native.profile_enable(True)
        t0 = time.perf_counter()
        train(gm, cams, targets, opt, Pipe(), bg, iterations=warm + iters, first_iter=warm + 1, scene_extent=6.0)
        torch.cuda.synchronize(dev)
        ms = round(1e3 * (time.perf_counter() - t0) / iters, 3)
        if profiled:
            prof = _native.profile_read(64)
            _native.profile_enable(False)
            out[kind + "_profiled"] = {"ms_per_it": ms, "kernel_sum_ms_per_it": round(sum(v[0] for v in prof.values()) / iters, 3),
                                       "kernel_ms_per_it": {k: round(v[0] / iters, 4) for k, v in
                                                            sorted(prof.items(), key=lambda kv: -kv[1][0])[:14]}}
        else:
            out.setdefault(kind + "_ms_per_it_runs", []).append(ms)
            out[kind + "_gaussians_end"] = int(gm._xyz.shape[0])
            out[kind + "_at_or_under_min_opacity_end"] = int((torch.sigmoid(gm._opacity.detach()) <= opt.mcmc_min_opacity).sum())
        del gm
        gc.collect()
        torch.cuda.empty_cache()
    print(json.dumps({"train": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=1_000_000)
    ap.add_argument("--window", type=float, default=0.3, help="seconds of calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--train-iters", type=int, default=300, help="iterations of each training leg (0: skip them)")
    ap.add_argument("--profile", action="store_true", help="also one training pass per leg under the library's per-kernel events")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mcmc_bench.py measures on the GPU: no device found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "kernels": kernel_legs(a.size, dev, a.window, a.repeats)}
    if a.train_iters > 0:
        result["train"] = train_legs(a.train_iters, dev, a.profile)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({"mcmc_bench": "done"}))


if __name__ == "__main__":
    main()
