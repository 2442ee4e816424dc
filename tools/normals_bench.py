"""Cost of the normal-map ops: each op forward and forward + backward against its torch twin and against its
bytes model, and a training step with the normal-consistency term off and on, alternated in one process.  Nothing here is a gate.

Device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  The bytes models are the
compulsory traffic of csrc/gsr_normals.hip: gaussian_normals 40 B in + 12 B out per Gaussian forward, 52 + 16 backward;
depth_to_normal 8 + 12 per pixel forward, 20 + 8 backward; the loss 20 in forward, 20 in + 20 out backward; each against the rate of
a device copy of as many bytes.  A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss,
backward; with the term on, render_normals and normal_consistency_loss beside it.  "ops" are the per-Gaussian normals and the loss
(forward + backward) on stored maps; the rest of the difference is the extra frame.

    python tools/normals_bench.py [--P 1000000] [--sizes 1080x1920 2160x3840] [--configs cfg3 cfg3n] [--reps 30]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

BYTES = {"gaussian_normals": (52, 52 + 68), "depth_to_normal": (20, 20 + 28), "normal_consistency_loss": (20, 20 + 40)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--sizes", nargs="+", default=["1080x1920", "2160x3840"])
    ap.add_argument("--configs", nargs="*", default=["cfg3", "cfg3n"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import normals_ref as NR
    import scene_synth as S
    from diff_gaussian_rasterization import normals as NM
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_normals
    from loss_utils import training_loss
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("normals_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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

    # ---- gaussian_normals
    s, q, m, g = (torch.as_tensor(v).to(dev) for v in NR.make_gaussians(a.P))
    V, c = (torch.as_tensor(v).to(dev) for v in NR.make_camera())
    ql = q.clone().requires_grad_(True)

    def g_fwd(native):
        with torch.no_grad():
            NM.gaussian_normals(s, q, m, V, c, native=native)

    def g_both(native):
        ql.grad = None
        NM.gaussian_normals(s, ql, m, V, c, native=native).backward(g)
    report("gaussian_normals", a.P, f"P={a.P}", g_fwd, g_both)

    # ---- the maps
    for size in a.sizes:
        H, W = (int(v) for v in size.split("x"))
        gen = torch.Generator().manual_seed(H + W)
        z = 3.0 + torch.rand(H, W, generator=gen)
        alpha = (0.3 + 0.6 * torch.rand(H, W, generator=gen))
        alpha[torch.rand(H, W, generator=gen) < 0.02] = 0.0                    # holes
        depth, alpha = (z * alpha)[None].to(dev), alpha[None].to(dev)
        N, gn = torch.randn(3, H, W, generator=gen).to(dev), torch.randn(3, H, W, generator=gen).to(dev)
        dl, al, Nl = (t.clone().requires_grad_(True) for t in (depth, alpha, N))
        tx, ty = 0.5 * W / H, 0.5

        def d_fwd(native):
            with torch.no_grad():
                NM.depth_to_normal(depth, alpha, tx, ty, native=native)

        def d_both(native):
            dl.grad = al.grad = None
            NM.depth_to_normal(dl, al, tx, ty, native=native).backward(gn)

        def l_fwd(native):
            with torch.no_grad():
                NM.normal_consistency_loss(N, depth, alpha, tx, ty, native=native)

        def l_both(native):
            dl.grad = al.grad = Nl.grad = None
            NM.normal_consistency_loss(Nl, dl, al, tx, ty, native=native).backward()
        report("depth_to_normal", H * W, f"{H}x{W}", d_fwd, d_both)
        report("normal_consistency_loss", H * W, f"{H}x{W}", l_fwd, l_both)

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
        tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        with torch.no_grad():
            maps = {k: v.clone() for k, v in render_normals(cam, model, pipe).items() if k in ("normal", "depth", "alpha")}

        def step(on):
            for p in params:
                p.grad = None
            loss = training_loss(render(cam, model, pipe, bg)["render"], gt)
            if on:
                mp = render_normals(cam, model, pipe)
                loss = loss + 0.05 * NM.normal_consistency_loss(mp["normal"], mp["depth"], mp["alpha"], tx, ty)
            loss.backward()

        def ops():
            for p in params:
                p.grad = None
            leaves = [maps[k].requires_grad_(True) for k in ("normal", "depth", "alpha")]
            for t in leaves:
                t.grad = None
            n = NM.gaussian_normals(model.get_scaling, model.get_rotation, model.get_xyz, cam.world_view_transform, cam.camera_center)
            (NM.normal_consistency_loss(*leaves, tx, ty) + 0.0 * n.sum()).backward()
        m = alternated({"off": lambda: step(False), "on": lambda: step(True), "ops": ops}, a.reps)
        off, on, op = m["off"][0], m["on"][0], m["ops"][0]
        print(f"{name}: step with lambda_normal off {off:.3f} ms ({m['off'][1]:.3f} .. {m['off'][2]:.3f}), on {on:.3f} ms "
              f"({m['on'][1]:.3f} .. {m['on'][2]:.3f}), difference {on - off:+.3f} ms ({100 * (on / off - 1):+.1f} %): the ops (getters, "
              f"normals, loss, both ways) {op:.3f} ms, the extra frame {on - off - op:.3f} ms")


if __name__ == "__main__":
    main()
