"""Cost of absgrad: a training step with pipe.absgrad off against the same step with it on, alternated in one process, and the
blend backward (render_bwd against render_bwd_abs) and the row reduction from the library's per-kernel profile.

A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss, backward.  Both variants are
warmed up first; the timed steps alternate in blocks of 5 (device events around each step); the per-kernel table comes from
separate steps with the library's profiler on (it synchronises, so it is kept out of the step times).  Prints medians, the spread
(min .. max) of each variant, and the overhead.

    python tools/absgrad_bench.py [--configs cfg3 cfg3n] [--steps 40] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["cfg3", "cfg3n"])
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import scene_synth as S
    from diff_gaussian_rasterization import _native as N
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("absgrad_bench needs a GPU: there is nothing to time without one")
    dev = torch.device("cuda:0")
    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene, cam = S.make_config(name)
        scene, cam = scene.to(dev), cam.to(dev)
        model = GaussianModel(scene.sh_degree)
        model.adopt_scene(scene, device=dev)
        params = list(model._t.values())
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 100)).to(dev)
        pipes = {False: Pipe(), True: Pipe()}
        pipes[True].absgrad = True
        bg = torch.zeros(3, device=dev)

        def step(on):
            for p in params:
                p.grad = None
            out = render(cam, model, pipes[on], bg)
            training_loss(out["render"], gt).backward()
            return out["viewspace_points"]

        def timed(on, n):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for e0, e1 in ev:
                e0.record()
                step(on)
                e1.record()
            torch.cuda.synchronize(dev)
            return [e0.elapsed_time(e1) for e0, e1 in ev]

        for on in (False, True):
            timed(on, a.warmup)
        times = {False: [], True: []}
        for _ in range(max(a.steps // 5, 1)):              # alternate in blocks of 5 steps
            for on in (False, True):
                times[on] += timed(on, 5)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{name}: step {med[False]:.3f} ms ({min(times[False]):.3f} .. {max(times[False]):.3f}), absgrad step {med[True]:.3f} ms "
              f"({min(times[True]):.3f} .. {max(times[True]):.3f}), overhead {100 * (med[True] / med[False] - 1):+.2f} % "
              f"(medians of {len(times[False])} alternated steps)")
        vsp = step(True)
        torch.cuda.synchronize(dev)
        g, ab = vsp.grad[:, :2].norm(dim=1), vsp.absgrad[:, :2].norm(dim=1)
        live = g > 0
        print(f"  median |absgrad| / |grad| over {int(live.sum())} Gaussians with a gradient: {float((ab[live] / g[live]).median()):.2f}")
        prof = {}
        for _ in range(3):                                 # profiled steps, alternated too
            for on in (False, True):
                N.profile_enable(True)
                timed(on, 5)
                for k, (ms, cnt) in N.profile_read(64).items():
                    t = prof.setdefault((on, k), [0.0, 0])
                    t[0] += ms
                    t[1] += cnt
                N.profile_enable(False)
        for on in (False, True):
            print(f"  per-kernel, absgrad {'on' if on else 'off'} (ms per step, 15 profiled steps):")
            rows = sorted(((k, v) for (o, k), v in prof.items() if o == on), key=lambda kv: -kv[1][0])
            for k, (ms, cnt) in rows:
                if k.startswith(("render_bwd", "reduce_rows", "screen_absgrad", "geom_bwd")):
                    print(f"    {k:24s} {ms / 15:8.4f}   launches/step {cnt / 15:.1f}")


if __name__ == "__main__":
    main()
