"""Cost of the camera gradients: a training step with plain camera tensors against the same step with viewmatrix, projmatrix and
campos requiring grad, alternated in one process.

A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss, backward.  Prints the median
step time of each variant, the overhead, and the library's per-kernel profile table for each (the two new launches have scopes of
their own: camera_bwd, camera_reduce).

    python tools/camera_grad_bench.py [--configs cfg3 cfg3n] [--steps 30] [--warmup 5]
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
        cam_on = cam.to(dev)
        cam_on.world_view_transform = cam.world_view_transform.clone().requires_grad_(True)
        cam_on.full_proj_transform = cam.full_proj_transform.clone().requires_grad_(True)
        cam_on.camera_center = cam.camera_center.clone().requires_grad_(True)
        cam_leaves = (cam_on.world_view_transform, cam_on.full_proj_transform, cam_on.camera_center)
        model = GaussianModel(scene.sh_degree)
        model.adopt_scene(scene, device=dev)
        params = list(model._t.values())
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 100)).to(dev)
        pipe, bg = Pipe(), torch.zeros(3, device=dev)

        def step(on):
            for p in params + list(cam_leaves):
                p.grad = None
            training_loss(render(cam_on if on else cam, model, pipe, bg)["render"], gt).backward()

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
        for _ in range(a.steps // 5):                     # alternate in blocks of 5 steps
            for on in (False, True):
                times[on] += timed(on, 5)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{name}: step without camera gradients {med[False]:.3f} ms, with {med[True]:.3f} ms, "
              f"overhead {100 * (med[True] / med[False] - 1):+.1f} % (medians of {len(times[False])} alternated steps)")
        for on in (False, True):
            N.profile_enable(True)
            timed(on, 5)
            prof = N.profile_read()
            N.profile_enable(False)
            print(f"  per-kernel, {'with' if on else 'without'} camera gradients (ms per step):")
            for k, (ms, cnt) in sorted(prof.items(), key=lambda kv: -kv[1][0]):
                print(f"    {k:24s} {ms / 5:8.3f}   launches/step {cnt / 5:.1f}")


if __name__ == "__main__":
    main()
