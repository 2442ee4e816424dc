"""Cost of the depth + alpha maps: a colour-only training step against a colour + depth + alpha step, alternated in one process.

A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss on the colour, plus for the aux
variant an L1 on alpha (against the ground truth's alpha) and on depth (against a constant), then backward.  Prints the median
step time of each variant, the overhead, and the library's per-kernel profile table for each.

    python tools/depth_alpha_bench.py [--configs cfg3 cfg3n] [--steps 30] [--warmup 5]
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
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import scene_synth as S
    from diff_gaussian_rasterization import _native as N
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from loss_utils import training_loss
    from scene import GaussianModel
    dev = torch.device("cuda:0")
    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene, cam = S.make_config(name)
        scene, cam = scene.to(dev), cam.to(dev)
        model = GaussianModel(scene.sh_degree)
        model.adopt_scene(scene, device=dev)
        params = list(model._t.values())
        gen = torch.Generator().manual_seed(cfg["seed"] + 100)
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=gen).to(dev)
        gt_alpha = (torch.rand(1, cfg["H"], cfg["W"], generator=gen) > 0.3).float().to(dev)
        pipe, bg = Pipe(), torch.zeros(3, device=dev)

        def step(aux):
            for p in params:
                p.grad = None
            out = render(cam, model, pipe, bg, depth_alpha=aux)
            loss = training_loss(out["render"], gt)
            if aux:
                loss = loss + (out["alpha"] - gt_alpha).abs().mean() + 0.1 * (out["depth"] - 3.0).abs().mean()
            loss.backward()

        def timed(aux, n):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for e0, e1 in ev:
                e0.record()
                step(aux)
                e1.record()
            torch.cuda.synchronize(dev)
            return [e0.elapsed_time(e1) for e0, e1 in ev]

        for aux in (False, True):
            timed(aux, a.warmup)
        times = {False: [], True: []}
        for _ in range(a.steps // 5):                     # alternate in blocks of 5 steps
            for aux in (False, True):
                times[aux] += timed(aux, 5)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{name}: colour-only step {med[False]:.3f} ms, colour + depth + alpha step {med[True]:.3f} ms, "
              f"overhead {100 * (med[True] / med[False] - 1):+.1f} % (medians of {len(times[False])} alternated steps)")
        for aux in (False, True):
            N.profile_enable(True)
            timed(aux, 5)
            prof = N.profile_read()
            N.profile_enable(False)
            print(f"  per-kernel, {'colour + depth + alpha' if aux else 'colour only'} (ms per step):")
            for k, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
                print(f"    {k:24s} {ms / 5:8.3f}   launches/step {cnt / 5:.1f}")


if __name__ == "__main__":
    main()
