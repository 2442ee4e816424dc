"""Cost of the depth-distortion ops: each op forward and forward + backward against its torch twin and against its
bytes model, and a training step with the distortion term off and on, alternated in one process.  Nothing here is a gate.

Device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  The bytes models are the
compulsory traffic of csrc/gsr_distortion.hip: depth_moments 12 B in + 12 B out per Gaussian forward, 24 + 12 backward; distortion_map
12 in + 4 out per pixel forward, 16 + 16 backward; the loss 12 in forward, 12 in + 16 out backward; each against the rate of a device
copy of as many bytes.  A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss, backward;
with the term on the frame is render_with_distortion's (depth, alpha and the moments beside the colour) and distortion_loss joins the
loss.  "ops" are the depth moments and the loss (forward + backward) on stored maps; the rest of the difference is what the frame's
blend costs more with the depth, alpha and extra channels than without them.

    python tools/distortion_bench.py [--P 1000000] [--sizes 1080x1920 2160x3840] [--configs cfg3 cfg3n] [--reps 30]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

BYTES = {"depth_moments": (24, 24 + 36), "distortion_map": (16, 16 + 32), "distortion_loss": (12, 12 + 28)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "2160x3840"])
    ap.add_argument("--configs", nargs="*", default=["cfg3", "cfg3n"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import distortion_ref as DR
    import scene_synth as S
    from diff_gaussian_rasterization import distortion as DM
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_with_distortion
    from loss_utils import training_loss
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("distortion_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
    dev = torch.device("cuda:0")

    def events(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return [e0.elapsed_time(e1) for e0, e1 in ev]

    def alternated(fns, n):
        """{variant: (median, min, max)} of the variants' times in ms, taken in alternated windows of 5."""
        for fn in fns.values():
            events(fn, 3)
        times = {k: [] for k in fns}
        for _ in range(max(n // 5, 1)):
            for k, fn in fns.items():
                times[k] += events(fn, 5)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}

    def show(t):
        return f"{1e3 * t[0]:.1f} us ({1e3 * t[1]:.1f} .. {1e3 * t[2]:.1f})"

    def copy_rate(nbytes):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        events(lambda: dst.copy_(src), 3)
        return 2 * src.numel() / (statistics.median(events(lambda: dst.copy_(src), 20)) * 1e-3)

    def report(name, n, unit, fwd, both):
        for label, fn, nbytes in (("forward", fwd, n * BYTES[name][0]), ("forward + backward", both, n * BYTES[name][1])):
            m = alternated({"hip": lambda: fn(True), "twin": lambda: fn(False)}, a.reps)
            rate, cr = nbytes / (m["hip"][0] * 1e-3), copy_rate(nbytes)
            print(f"{name} {label} {unit}: HIP {show(m['hip'])}, twin {show(m['twin'])}, ratio {m['twin'][0] / m['hip'][0]:.1f}; "
                  f"{nbytes / 1e6:.0f} MB by the bytes model -> {rate / 1e12:.2f} TB/s, {100 * rate / cr:.0f} % of the copy rate ({cr / 1e12:.2f} TB/s)")

    # ---- depth_moments
    means, V, g = (torch.as_tensor(v).to(dev) for v in DR.make_gaussians(a.P))
    ml = means.clone().requires_grad_(True)

    def g_fwd(native):
        with torch.no_grad():
            DM.depth_moments(means, V, native=native)

    def g_both(native):
        ml.grad = None
        DM.depth_moments(ml, V, native=native).backward(g)
    report("depth_moments", a.P, f"P={a.P}", g_fwd, g_both)

    # ---- the maps
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator().manual_seed(H + W)
        alpha = 0.3 + 0.6 * torch.rand(H, W, generator=gen)
        alpha[torch.rand(H, W, generator=gen) < 0.02] = 0.0                    # holes
        mean = torch.rand(H, W, generator=gen)
        mom = torch.stack((alpha * mean, alpha * (mean * mean + 0.01), torch.zeros(H, W))).to(dev)
        alpha, gD = alpha[None].to(dev), torch.randn(1, H, W, generator=gen).to(dev)
        Ml, al = (t.clone().requires_grad_(True) for t in (mom, alpha))

        def m_fwd(native):
            with torch.no_grad():
                DM.distortion_map(mom, alpha, native=native)

        def m_both(native):
            Ml.grad = al.grad = None
            DM.distortion_map(Ml, al, native=native).backward(gD)

        def l_fwd(native):
            with torch.no_grad():
                DM.distortion_loss(mom, alpha, native=native)

        def l_both(native):
            Ml.grad = al.grad = None
            DM.distortion_loss(Ml, al, native=native).backward()
        report("distortion_map", H * W, f"{H}x{W}", m_fwd, m_both)
        report("distortion_loss", H * W, f"{H}x{W}", l_fwd, l_both)

    # ---- a training step
    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene_c, cam = S.make_config(name)
        scene_c, cam = scene_c.to(dev), cam.to(dev)
        model = GaussianModel(scene_c.sh_degree)
        model.adopt_scene(scene_c, device=dev)
        params = list(model._t.values())
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 100)).to(dev)
        bg, pipe = torch.zeros(3, device=dev), Pipe()
        with torch.no_grad():
            pkg = render_with_distortion(cam, model, pipe, bg, with_map=False)
            maps = {k: pkg[k].clone() for k in ("extra", "alpha")}

        def step(on):
            for p in params:
                p.grad = None
            if on:
                pkg = render_with_distortion(cam, model, pipe, bg, with_map=False)
                loss = training_loss(pkg["render"], gt) + 100.0 * DM.distortion_loss(pkg["extra"], pkg["alpha"])
            else:
                loss = training_loss(render(cam, model, pipe, bg)["render"], gt)
            loss.backward()

        def aux():
            for p in params:
                p.grad = None
            training_loss(render(cam, model, pipe, bg, depth_alpha=True)["render"], gt).backward()

        def ops():
            for p in params:
                p.grad = None
            leaves = [maps[k].requires_grad_(True) for k in ("extra", "alpha")]
            for t in leaves:
                t.grad = None
            rows = DM.depth_moments(model.get_xyz, cam.world_view_transform)
            (DM.distortion_loss(*leaves) + 0.0 * rows.sum()).backward()
        m = alternated({"off": lambda: step(False), "on": lambda: step(True), "aux": aux, "ops": ops}, a.reps)
        off, on, ax, op = m["off"][0], m["on"][0], m["aux"][0], m["ops"][0]
        print(f"{name}: step with lambda_dist off {off:.3f} ms ({m['off'][1]:.3f} .. {m['off'][2]:.3f}), on {on:.3f} ms "
              f"({m['on'][1]:.3f} .. {m['on'][2]:.3f}), difference {on - off:+.3f} ms ({100 * (on / off - 1):+.1f} %): the ops (moments, "
              f"loss, both ways) {op:.3f} ms, the frame's channels {on - off - op:.3f} ms; the same step on an aux frame (depth and alpha, "
              f"no extra colours, no term) {ax:.3f} ms ({m['aux'][1]:.3f} .. {m['aux'][2]:.3f})")


if __name__ == "__main__":
    main()
