"""Cost of the anti-aliasing switch: a training step with pipe.antialiasing off against the same step with it on, alternated in one
process, and the two kernels' own times against a bytes model.

A step is render() (scene.GaussianModel, the raw-parameter route bench.py times), the training loss, backward.  Prints per config
the median step time of each variant and their difference (device events), then aa_fwd / aa_bwd from the library's per-kernel
profile with the bytes each moves and the HBM rate that amounts to.  Nothing here is a gate.

Bytes model (csrc/gsr_antialias.hip): the forward reads mean 12 + scale 12 + quaternion 16 + opacity 4 = 44 B per Gaussian and
writes 4.  The backward reads the incoming gradient (4 B) of every Gaussian; for a row with a non-zero gradient it reads the other
44 B too; it writes 44 B (mean 12, opacity 4, scale 12, quaternion 16) for every row, zeros included.  The share of rows with a
gradient is measured from the opacity's gradient of one step.

    python tools/antialias_bench.py [--configs cfg3 cfg3n] [--steps 30] [--warmup 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))

import torch  # noqa: E402

FWD_READ, FWD_WRITE = 44, 4
BWD_READ_ALWAYS, BWD_READ_LIVE, BWD_WRITE = 4, 44, 44


def model_bytes(P, live):
    """(forward bytes, backward bytes) for P Gaussians of which `live` carry a non-zero incoming gradient."""
    return P * (FWD_READ + FWD_WRITE), P * (BWD_READ_ALWAYS + BWD_WRITE) + live * BWD_READ_LIVE


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
    if not torch.cuda.is_available():
        raise SystemExit("antialias_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
    dev = torch.device("cuda:0")
    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene, cam = S.make_config(name)
        scene, cam = scene.to(dev), cam.to(dev)
        model = GaussianModel(scene.sh_degree)
        model.adopt_scene(scene, device=dev)
        params = list(model._t.values())
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=torch.Generator().manual_seed(cfg["seed"] + 100)).to(dev)
        bg = torch.zeros(3, device=dev)
        pipes = {False: Pipe(), True: Pipe()}
        pipes[True].antialiasing = True

        def step(on):
            for p in params:
                p.grad = None
            training_loss(render(cam, model, pipes[on], bg)["render"], gt).backward()

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
        for _ in range(max(a.steps // 5, 1)):             # alternate in blocks of 5 steps
            for on in (False, True):
                times[on] += timed(on, 5)
        med = {k: statistics.median(v) for k, v in times.items()}
        print(f"{name}: step with the switch off {med[False]:.3f} ms, on {med[True]:.3f} ms, difference {med[True] - med[False]:+.3f} ms "
              f"({100 * (med[True] / med[False] - 1):+.1f} %; medians of {len(times[False])} alternated steps)")
        N.profile_enable(True)
        timed(True, 5)
        prof = N.profile_read(128)
        N.profile_enable(False)
        # rows of the compensation's backward that ran the chain: the compensated logit's gradient is non-zero exactly where the
        # input logit's is (dlogit'/dlogit > 0)
        live = int((model._opacity.grad != 0).sum())
        P = int(model._xyz.shape[0])
        for kernel, nbytes in zip(("aa_fwd", "aa_bwd"), model_bytes(P, live)):
            ms, cnt = prof[kernel]
            assert cnt == 5, (kernel, cnt)
            print(f"  {kernel}: {1e3 * ms / cnt:8.1f} us per launch, {nbytes / 1e6:7.1f} MB by the bytes model "
                  f"({live} of {P} rows with a gradient) -> {nbytes / (ms / cnt * 1e-3) / 1e12:.2f} TB/s")


if __name__ == "__main__":
    main()
