"""Cost of the 3D smoothing filter: the filter computation and its application against their torch twins, and a training step with
the model's filter off against the same step with it on, alternated in one process.  Nothing here is a gate.

compute_filter_3d at P Gaussians and C cameras: the HIP path (two launches) against the twin's loop over the cameras (upstream's
compute_3D_filter), wall clock around a synchronised call (the call holds its one host synchronisation).
apply_filter_3d (raw) forward and forward + backward: device events, against the twin, with the bytes model of
csrc/gsr_filter3d.hip (forward 20 B in + 16 B out per Gaussian, backward 36 + 16) and the rate of a device copy of as many bytes.
A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss, backward.

    python tools/filter3d_bench.py [--P 1000000] [--cameras 100 300] [--configs cfg3 cfg3n] [--reps 20]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))

import torch  # noqa: E402

FWD_BYTES, BWD_BYTES = 20 + 16, 36 + 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, nargs="+", default=[100, 300])
    ap.add_argument("--configs", nargs="*", default=["cfg3", "cfg3n"])
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import scene_synth as S
    from diff_gaussian_rasterization.filter3d import apply_filter_3d, compute_filter_3d
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("filter3d_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
    dev = torch.device("cuda:0")
    med = statistics.median

    def wall(fn, n):
        out = []
        for _ in range(n):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            out.append(1e3 * (time.perf_counter() - t0))
        return out

    def events(fn, n):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for e0, e1 in ev:
            e0.record()
            fn()
            e1.record()
        torch.cuda.synchronize(dev)
        return [e0.elapsed_time(e1) for e0, e1 in ev]

    def alternated(fns, timer, n):
        """Medians of the variants' times, taken in alternated windows of 5."""
        for fn in fns.values():
            timer(fn, 2)
        times = {k: [] for k in fns}
        for _ in range(max(n // 5, 1)):
            for k, fn in fns.items():
                times[k] += timer(fn, 5)
        return {k: med(v) for k, v in times.items()}

    scene = S.make_scene(a.P, 1920, 1080, 0, 3, zmin=0.5).to(dev)
    for C in a.cameras:
        cams = [c.to(dev) for c in S.arc_cameras(1920, 1080, C)]
        m = alternated({"hip": lambda: compute_filter_3d(scene.means3D, cams), "twin": lambda: compute_filter_3d(scene.means3D, cams, native=False)},
                       wall, min(a.reps, 10))
        print(f"compute_filter_3d P={a.P} C={C}: HIP {m['hip']:.3f} ms (camera table built on the host included), twin's camera loop "
              f"{m['twin']:.3f} ms, ratio {m['twin'] / m['hip']:.1f}")
    filt = compute_filter_3d(scene.means3D, [c.to(dev) for c in S.arc_cameras(1920, 1080, 8)])
    leaves = [scene.opacity_logits.clone().requires_grad_(True), scene.log_scales.clone().requires_grad_(True)]
    g_o, g_s = torch.randn_like(leaves[0]), torch.randn_like(leaves[1])

    def fwd(native):
        with torch.no_grad():
            apply_filter_3d(*leaves, filt, raw=True, native=native)

    def both(native):
        for t in leaves:
            t.grad = None
        torch.autograd.backward(apply_filter_3d(*leaves, filt, raw=True, native=native), (g_o, g_s))

    src = torch.empty(a.P * (FWD_BYTES + BWD_BYTES) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    copy_rate = 2 * src.numel() / (med(events(lambda: dst.copy_(src), 20)) * 1e-3)
    for label, fn, nbytes in (("forward", fwd, a.P * FWD_BYTES), ("forward + backward", both, a.P * (FWD_BYTES + BWD_BYTES))):
        m = alternated({"hip": lambda: fn(True), "twin": lambda: fn(False)}, events, a.reps)
        rate = nbytes / (m["hip"] * 1e-3)
        print(f"apply_filter_3d {label} P={a.P}: HIP {1e3 * m['hip']:.1f} us, twin {1e3 * m['twin']:.1f} us, ratio {m['twin'] / m['hip']:.1f}; "
              f"{nbytes / 1e6:.0f} MB by the bytes model -> {rate / 1e12:.2f} TB/s, {100 * rate / copy_rate:.0f} % of the copy rate "
              f"({copy_rate / 1e12:.2f} TB/s)")
    # the kernels' own times: 50 launches back to back through the binding between one pair of events (the calls above carry
    # torch's autograd and allocator around a single launch, and a pair of events around one short kernel its own microseconds)
    from diff_gaussian_rasterization import _native as N
    from diff_gaussian_rasterization.filter3d import camera_table
    o, s = leaves[0].detach(), leaves[1].detach()
    table, focal_max = camera_table([c.to(dev) for c in S.arc_cameras(1920, 1080, a.cameras[-1])], dev)

    def burst(fn):
        return lambda: [fn() for _ in range(50)]
    for kernel, fn, nbytes in (
            ("filter3d_apply_fwd<raw>", lambda: N.filter3d_apply_forward(o, s, filt, True), a.P * FWD_BYTES),
            ("filter3d_apply_bwd<raw>", lambda: N.filter3d_apply_backward(o, s, filt, True, g_o, g_s, (True, True)), a.P * BWD_BYTES),
            ("filter3d_apply_fwd<activated>", lambda: N.filter3d_apply_forward(o, s, filt, False), a.P * FWD_BYTES)):
        events(burst(fn), 2)
        us = 1e3 * med(events(burst(fn), 5)) / 50
        rate = nbytes / (us * 1e-6)
        print(f"  {kernel}: {us:6.1f} us per launch, {nbytes / 1e6:.0f} MB by the bytes model -> {rate / 1e12:.2f} TB/s, "
              f"{100 * rate / copy_rate:.0f} % of the copy rate")
    N.profile_enable(True)
    for _ in range(5):
        N.filter3d_compute(scene.means3D, table, focal_max)
    prof = N.profile_read(128)
    N.profile_enable(False)
    ms, cnt = prof["filter3d_min_depth"]
    print(f"  filter3d_min_depth: {1e3 * ms / cnt:6.1f} us per launch (the library's per-kernel profile, {cnt} launches, C = {a.cameras[-1]}: "
          f"{a.P * a.cameras[-1] / (ms / cnt * 1e-3) / 1e12:.2f} T (Gaussian, camera) pairs/s)")
    ms, cnt = prof["filter3d_finish"]
    print(f"  filter3d_finish: {1e3 * ms / cnt:6.1f} us per launch ({cnt} launches)")
    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene_c, cam = S.make_config(name)
        scene_c, cam = scene_c.to(dev), cam.to(dev)
        model = GaussianModel(scene_c.sh_degree)
        model.adopt_scene(scene_c, device=dev)
        model.compute_3D_filter([cam])
        filt_c = model.filter_3D
        params = list(model._t.values())
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 100)).to(dev)
        bg = torch.zeros(3, device=dev)

        def step(on):
            model.filter_3D = filt_c if on else None
            for p in params:
                p.grad = None
            training_loss(render(cam, model, Pipe(), bg)["render"], gt).backward()
        m = alternated({"off": lambda: step(False), "on": lambda: step(True)}, events, a.reps)
        print(f"{name}: step with the filter off {m['off']:.3f} ms, on {m['on']:.3f} ms, difference {m['on'] - m['off']:+.3f} ms "
              f"({100 * (m['on'] / m['off'] - 1):+.1f} %; the filtered model is another scene: larger splats)")


if __name__ == "__main__":
    main()
