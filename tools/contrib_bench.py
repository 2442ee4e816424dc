"""The blend statistics' cost on the GPU, in one process (DESIGN.md section 21 holds the table this prints).  Per workload (cfg3: the
saturating frame; cfg3n: the ordinary one), with a colour per Gaussian as input so that every leg renders the same frame:

  kernel   the blend forward's launches of a frame without and with the statistics, from the library's per-kernel events
           (gsr_profile_enable; scopes render_fwd and render_fwd_contrib), us per frame
  frame    whole calls, medians of --repeats alternated windows timed with device events: the plain forward under no_grad, the
           statistics frame, and (b) the forward + backward under dL/dpix = (1, 0, 0) with colors_precomp the only leaf - the way
           weight_sum alone could be had without the feature (blend backward, row reduction and geometry backward included)
  model    GaussianModel.contribution_stats over --cameras cameras of the workload's scene, wall clock, ms in all and per camera

One JSON line per leg."""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd")]
import torch  # noqa: E402


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


def workload(name, dev, window, repeats, frames):
    import scene_synth as S
    from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer, _native
    from diff_gaussian_rasterization.contrib import ContributionStats
    scene, cam = S.make_config(name)
    cam = cam.to(dev)
    a = {k: v.to(dev).contiguous() for k, v in scene.activated().items() if k != "shs"}
    P = scene.P
    colors = torch.rand(P, 3, generator=torch.Generator().manual_seed(P)).to(dev)
    rs = GaussianRasterizationSettings(cam.image_height, cam.image_width, math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5),
                                       torch.zeros(3, device=dev), 1.0, cam.world_view_transform, cam.full_proj_transform, scene.sh_degree,
                                       cam.camera_center, False, False)
    means2D = torch.zeros(P, 3, device=dev)
    stats = ContributionStats(P, dev)
    leaf = colors.clone().requires_grad_(True)
    up = torch.zeros(3, cam.image_height, cam.image_width, device=dev)
    up[0] = 1.0

    def plain():
        with torch.no_grad():
            GaussianRasterizer(rs)(means2D=means2D, colors_precomp=colors, **a)

    def contrib():
        with torch.no_grad():
            GaussianRasterizer(rs, contributions=stats)(means2D=means2D, colors_precomp=colors, **a)

    def forward_backward():
        leaf.grad = None
        GaussianRasterizer(rs)(means2D=means2D, colors_precomp=leaf, **a)[0].backward(up)
    for f in (plain, contrib, forward_backward):
        f()
    torch.cuda.synchronize()
    agree = float((stats.weight_sum - leaf.grad[:, 0].double()).abs().max())
    composited = int((stats.count > 0).sum())

    out = {"workload": name, "P": P, "composited_gaussians": composited, "weight_sum_vs_gradient_max_abs": agree}
    kernel = {}
    for label, f, scope in (("plain", plain, "render_fwd"), ("contrib", contrib, "render_fwd_contrib")):
        _native.profile_enable(True)
        for _ in range(frames):
            f()
        prof = _native.profile_read(64)
        _native.profile_enable(False)
        ms, launches = prof.get(scope, (0.0, 0))
        kernel[label] = {"scope": scope, "us_per_frame": round(1e3 * ms / frames, 1), "launches_per_frame": launches / frames}
    kernel["extra_us_per_frame"] = round(kernel["contrib"]["us_per_frame"] - kernel["plain"]["us_per_frame"], 1)
    out["kernel"] = kernel
    print(json.dumps({"workload": name, "kernel": kernel}), flush=True)

    t = alternated({"plain": plain, "contrib": contrib, "forward_backward": forward_backward}, window, repeats)
    out["frame"] = {k: us(v) for k, v in t.items()}
    out["frame"]["contrib_over_plain"] = round(t["contrib"][0] / t["plain"][0], 3)
    out["frame"]["forward_backward_over_contrib"] = round(t["forward_backward"][0] / t["contrib"][0], 3)
    print(json.dumps({"workload": name, "frame": out["frame"]}), flush=True)
    return out, scene


def model_leg(name, scene, dev, cameras):
    import scene_synth as S
    from scene import GaussianModel
    cfg = S.CONFIGS[name]
    gm = GaussianModel(cfg["D"])
    gm.adopt_scene(scene, device=dev)
    cams = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], cameras)]
    gm.significance(gm.contribution_stats(cams[:2]))   # warm-up: workspaces of this shape, the sort's first call
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    stats = gm.contribution_stats(cams)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t1 = time.perf_counter()
    scores = gm.significance(stats)
    torch.cuda.synchronize()
    out = {"workload": name, "cameras": cameras, "P": gm.get_xyz.shape[0], "contribution_stats_ms": round(1e3 * dt, 1),
           "ms_per_camera": round(1e3 * dt / cameras, 3), "significance_ms": round(1e3 * (time.perf_counter() - t1), 2),
           "composited_gaussians": int((stats.count > 0).sum()), "scores_positive": int((scores > 0).sum())}
    print(json.dumps({"model": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workloads", default="cfg3,cfg3n")
    ap.add_argument("--window", type=float, default=0.25, help="seconds per timing window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=20, help="frames per profiled kernel leg")
    ap.add_argument("--cameras", type=int, default=100, help="cameras of the model leg (0: skip)")
    ap.add_argument("--out", default=None, help="also write everything as one JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    result = {"workloads": [], "model": []}
    for name in args.workloads.split(","):
        out, scene = workload(name, dev, args.window, args.repeats, args.frames)
        result["workloads"].append(out)
        if args.cameras > 0:
            result["model"].append(model_leg(name, scene, dev, args.cameras))
        del scene
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
