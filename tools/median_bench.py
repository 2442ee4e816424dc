"""Cost of the median depth map: the blend forward and backward kernels of the aux variant against the median
variant on one frame, and the whole step (frame, upstream gradients on colour, depth and alpha - and on the median - backward), the two
alternated in one process.  Nothing here is a gate.

Steps: device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  Kernels: the library's
own per-kernel timing (gsr_profile_enable) summed over a frame's launches of a scope, one frame per sample, the two variants' frames
alternated; a figure is the median over the frames with its min .. max.  The frame is render() on scene.GaussianModel (the
raw-parameter route bench.py times) with depth_alpha=True.

    python tools/median_bench.py [--configs cfg3 cfg3n] [--reps 30]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["cfg3", "cfg3n"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import scene_synth as S
    from diff_gaussian_rasterization import _native
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("median_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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
        for fn in fns.values():
            events(fn, 3)
        times = {k: [] for k in fns}
        for _ in range(max(n // 5, 1)):
            for k, fn in fns.items():
                times[k] += events(fn, 5)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}

    def scope_ms(fn, scopes):
        """{scope: total ms of its launches in one call of fn}"""
        _native.profile_enable(True)
        try:
            fn()
            torch.cuda.synchronize(dev)
            read = _native.profile_read(128)
        finally:
            _native.profile_enable(False)
        return {s: read[s][0] if s in read else float("nan") for s in scopes}

    for name in a.configs:
        cfg = S.CONFIGS[name]
        scene_c, cam = S.make_config(name)
        scene_c, cam = scene_c.to(dev), cam.to(dev)
        model = GaussianModel(scene_c.sh_degree)
        model.adopt_scene(scene_c, device=dev)
        params = list(model._t.values())
        gen = torch.Generator().manual_seed(cfg["seed"] + 100)
        gt = torch.rand(3, cfg["H"], cfg["W"], generator=gen).to(dev)
        gz, ga, gm = (torch.rand(1, cfg["H"], cfg["W"], generator=gen).to(dev) - 0.5 for _ in range(3))
        bg, pipe = torch.zeros(3, device=dev), Pipe()

        # an aux frame and a median frame with the same colour, depth and alpha gradients (+ the median map's)
        def frame(med):
            for p in params:
                p.grad = None
            pkg = render(cam, model, pipe, bg, depth_alpha=True, median_depth=True) if med else render(cam, model, pipe, bg, depth_alpha=True)
            outs, ups = [pkg["render"], pkg["depth"], pkg["alpha"]], [gt, gz, ga]
            if med:
                outs, ups = outs + [pkg["median_depth"]], ups + [gm]
            torch.autograd.backward(outs, ups)
        for med in (False, True):
            frame(med)
        pairs = (("render_fwd_aux", "render_fwd_median"), ("render_bwd_aux", "render_bwd_median"))
        samples = {s: [] for pair in pairs for s in pair}
        for _ in range(max(a.reps // 2, 5)):
            for med in (False, True):
                for s, v in scope_ms(lambda: frame(med), [pair[med] for pair in pairs]).items():
                    samples[s].append(v)
        for aux_s, med_s in pairs:
            ma, mm = statistics.median(samples[aux_s]), statistics.median(samples[med_s])
            print(f"{name}: {aux_s} {1e3 * ma:.1f} us ({1e3 * min(samples[aux_s]):.1f} .. {1e3 * max(samples[aux_s]):.1f}), "
                  f"{med_s} {1e3 * mm:.1f} us ({1e3 * min(samples[med_s]):.1f} .. {1e3 * max(samples[med_s]):.1f}), "
                  f"difference {1e3 * (mm - ma):+.1f} us ({100 * (mm / ma - 1):+.1f} %)")
        m = alternated({"aux": lambda: frame(False), "median": lambda: frame(True)}, a.reps)
        f = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"
        print(f"{name}: whole step, aux frame {f(m['aux'])}; median frame {f(m['median'])}: "
              f"{m['median'][0] - m['aux'][0]:+.3f} ms ({100 * (m['median'][0] / m['aux'][0] - 1):+.1f} %)")


if __name__ == "__main__":
    main()
