"""The error-weighted blend statistics' cost on the GPU, in one process (DESIGN.md section 22 holds the table this prints).  Per
workload (cfg3: the saturating frame; cfg3n: the ordinary one), with a colour per Gaussian as input so that every leg renders the same
frame, and a seeded uniform error map E:

  kernel   the blend forward's launches of a statistics frame without and with the fourth total, and the fold, from the library's
           per-kernel events (gsr_profile_enable; scopes render_fwd_contrib, render_fwd_contrib_error, contrib_error_fold), us per frame
  frame    whole calls, medians of --repeats alternated windows timed with device events: the plain statistics frame, the error frame
           (fold included), and the forward + backward under dL/dpix = (E, 0, 0) with colors_precomp the only leaf - the way the
           error sum could be had without the feature
  fold     gsr_contrib_error_fold alone at --fold-gaussians Gaussians against its bytes model (24 B read + 20 B written each)
  model    GaussianModel.error_stats over --views cameras of the workload's scene (a plain render, the map and an error frame per
           camera), wall clock, ms in all and per camera
  train    (cfg3 only) train() iterations over a densification window with opt.densify_error_views = --views against 0, wall clock
           per iteration, refinements every opt.densification_interval iterations included

One JSON line per leg."""
import argparse
import json
import math
import os
import random
import sys
import time
from dataclasses import replace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

from contrib_bench import alternated, us  # noqa: E402


def workload(name, dev, window, repeats, frames):
    import scene_synth as S
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _native
    from diff_gaussian_rasterization.contrib import ErrorStats
    scene, cam = S.make_config(name)
    cam = cam.to(dev)
    a = {k: v.to(dev).contiguous() for k, v in scene.activated().items() if k != "shs"}
    P = scene.P
    H, W = int(cam.image_height), int(cam.image_width)
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(P)).to(dev)
    E = torch.rand(H, W, generator=torch.Generator().manual_seed(P + 1)).to(dev)
    rs = GaussianRasterizationSettings(H, W, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5), torch.zeros(3, device=dev), 1.0,
                                       cam.world_view_transform, cam.full_proj_transform, scene.sh_degree, cam.camera_center, False, False)
    means2D = torch.zeros(P, 3, device=dev)
    stats = ErrorStats(P, dev)
    leaf = colors.clone().requires_grad_(True)
    up = torch.zeros(3, H, W, device=dev)
    up[0] = E

    def contrib():
        with torch.no_grad():
            GaussianRasterizer(rs, contributions=stats)(means2D=means2D, colors_precomp=colors, **a)

    def error():
        with torch.no_grad():
            GaussianRasterizer(rs, contributions=stats, pixel_error=E)(means2D=means2D, colors_precomp=colors, **a)

    def forward_backward():
        leaf.grad = None
        GaussianRasterizer(rs)(means2D=means2D, colors_precomp=leaf, **a)[0].backward(up)
    forward_backward()
    contrib()
    stats.reset()
    error()
    torch.cuda.synchronize()
    agree = float((stats.error_sum - leaf.grad[:, 0].double()).abs().max())
    out = {"workload": name, "P": P, "gaussians_with_error": int((stats.error_sum_q32 > 0).sum()), "error_sum_vs_gradient_max_abs": agree,
           "error_sum_max": float(stats.error_sum.max())}

    kernel = {}
    for label, f, scopes in (("contrib", contrib, ("render_fwd_contrib",)), ("error", error, ("render_fwd_contrib_error", "contrib_error_fold"))):
        _native.profile_enable(True)
        for _ in range(frames):
            f()
        prof = _native.profile_read(64)
        _native.profile_enable(False)
        for scope in scopes:
            ms, launches = prof.get(scope, (0.0, 0))
            kernel[scope] = {"us_per_frame": round(1e3 * ms / frames, 1), "launches_per_frame": launches / frames}
    kernel["extra_blend_us_per_frame"] = round(kernel["render_fwd_contrib_error"]["us_per_frame"] - kernel["render_fwd_contrib"]["us_per_frame"], 1)
    out["kernel"] = kernel
    print(json.dumps({"workload": name, "kernel": kernel}), flush=True)

    t = alternated({"contrib": contrib, "error": error, "forward_backward": forward_backward}, window, repeats)
    out["frame"] = {k: us(v) for k, v in t.items()}
    out["frame"]["error_over_contrib"] = round(t["error"][0] / t["contrib"][0], 3)
    out["frame"]["forward_backward_over_error"] = round(t["forward_backward"][0] / t["error"][0], 3)
    print(json.dumps({"workload": name, "frame": out["frame"]}), flush=True)
    return out, scene


def fold_leg(dev, P, window, repeats):
    from diff_gaussian_rasterization.contrib import ErrorStats
    stats = ErrorStats(P, dev)
    stats.error_frame_q32.random_(0, 2 ** 36)
    t = alternated({"fold": stats.fold}, window, repeats)["fold"]
    nbytes = 44 * P
    out = {"gaussians": P, **us(t), "bytes_model": nbytes, "GB_per_s": round(nbytes / t[0] * 1e-9, 1)}
    print(json.dumps({"fold": out}), flush=True)
    return out


def _model_and_views(name, scene, dev, views):
    import scene_synth as S
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    cfg = S.CONFIGS[name]
    gm = GaussianModel(cfg["D"])
    gm.adopt_scene(scene, device=dev)
    cams = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], views)]
    bg = torch.zeros(3, device=dev)
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():       # targets: the model's own views, disturbed (an error map that is neither empty nor saturated)
        targets = [(render(c, gm, Pipe(), bg)["render"] + 0.2 * (torch.rand(3, cfg["H"], cfg["W"], generator=g).to(dev) - 0.5)).clamp(0, 1)
                   for c in cams]
    return gm, cams, targets, bg


def model_leg(name, scene, dev, views):
    gm, cams, targets, bg = _model_and_views(name, scene, dev, views)
    gm.error_stats(cams[:2], targets[:2])           # warm-up: workspaces of this shape
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = gm.error_stats(cams, targets)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    out = {"workload": name, "views": views, "P": gm.get_xyz.shape[0], "error_stats_ms": round(1e3 * dt, 1),
           "ms_per_view": round(1e3 * dt / views, 3), "gaussians_with_error": int((stats.error_sum_q32 > 0).sum())}
    print(json.dumps({"model": out}), flush=True)
    return out


def train_leg(name, scene, dev, views, iterations):
    from gaussian_params import Pipe
    from scene import OptimizationDefaults
    from train_loop import train
    out = {"workload": name, "iterations": iterations}
    for label, n in (("off", 0), ("error", views), ("off_again", 0), ("error_again", views)):
        gm, cams, targets, bg = _model_and_views(name, scene, dev, views)
        opt = replace(OptimizationDefaults(), densify_from_iter=0, densify_until_iter=10 ** 9, densify_error_views=n)
        gm.training_setup(opt)
        random.seed(3)
        torch.manual_seed(3)
        train(gm, cams, targets, opt, Pipe(), bg, iterations=5, scene_extent=5.0)       # warm-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        train(gm, cams, targets, opt, Pipe(), bg, iterations=iterations, first_iter=6, scene_extent=5.0)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out[label] = {"densify_error_views": n, "ms_per_iteration": round(1e3 * dt / (iterations - 5), 3), "P_end": gm.get_xyz.shape[0],
                      "refinements": sum(1 for it in range(6, iterations + 1) if it % opt.densification_interval == 0)}
        del gm
        torch.cuda.empty_cache()
    print(json.dumps({"train": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg3,cfg3n")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timing window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20, help="frames per profiled kernel leg")
    ap.add_argument("--views", type=int, default=10, help="cameras of the model and train legs (0: skip both)")
    ap.add_argument("--fold-gaussians", type=int, default=1_000_000, help="Gaussians of the fold leg (0: skip)")
    ap.add_argument("--train-iterations", type=int, default=305, help="iterations of the train leg (0: skip)")
    ap.add_argument("--out", default=None, help="also write everything as one JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"workloads": [], "model": [], "train": []}
    for name in args.workloads.split(","):
        out, scene = workload(name, dev, args.window, args.repeats, args.frames)
        result["workloads"].append(out)
        if args.views > 0:
            result["model"].append(model_leg(name, scene, dev, args.views))
            if name == "cfg3" and args.train_iterations > 0:
                result["train"].append(train_leg(name, scene, dev, args.views, args.train_iterations))
        del scene
        torch.cuda.empty_cache()
    if args.fold_gaussians > 0:
        result["fold"] = fold_leg(dev, args.fold_gaussians, args.window, args.repeats)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
