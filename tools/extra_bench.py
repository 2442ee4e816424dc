"""Cost of the extra-colour channels: the blend forward and backward kernels of the aux variant against the ext
variant on one frame, and a training step with the normal-consistency term on - the two-frame path (render + render_normals) against
the one-frame path (render_with_normals) - alternated in one process.  Nothing here is a gate.

Steps: device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  Kernels: the library's
own per-kernel timing (gsr_profile_enable) summed over a frame's launches of a scope, one frame per sample, the two variants'
frames alternated; a figure is the median over the frames with its min .. max.  A step is the frame(s) (scene.GaussianModel, the
raw-parameter route bench.py times), the training loss plus 0.05 x normal_consistency_loss, backward.

    python tools/extra_bench.py [--configs cfg3 cfg3n] [--reps 30]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["cfg3", "cfg3n"])
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    import scene_synth as S
    from diff_gaussian_rasterization import _native
    from diff_gaussian_rasterization import normals as NM
    from gaussian_params import Pipe
    from gaussian_renderer import render, render_normals, render_with_normals
    from loss_utils import training_loss
    from scene import GaussianModel
    if not torch.cuda.is_available():
        raise SystemExit("extra_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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
        gz, ga = (torch.rand(1, cfg["H"], cfg["W"], generator=gen).to(dev) - 0.5 for _ in range(2))
        bg, pipe = torch.zeros(3, device=dev), Pipe()
        tx, ty = math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5)
        P = model.get_xyz.shape[0]
        extra = (torch.rand(P, 3, generator=gen) * 2 - 1).to(dev)

        # ---- the blend kernels: an aux frame and an ext frame with the same colour, depth and alpha gradients (+ the extra map's)
        def frame(ext):
            for p in params:
                p.grad = None
            t = extra.clone().requires_grad_(True) if ext else None
            pkg = render(cam, model, pipe, bg, depth_alpha=True, extra_colors=t)
            outs, ups = [pkg["render"], pkg["depth"], pkg["alpha"]], [gt, gz, ga]
            if ext:
                outs, ups = outs + [pkg["extra"]], ups + [gt]
            torch.autograd.backward(outs, ups)
        for ext in (False, True):
            frame(ext)
        pairs = (("render_fwd_aux", "render_fwd_ext"), ("render_bwd_aux", "render_bwd_ext"), ("reduce_rows_aux", "reduce_rows_ext"))
        samples = {s: [] for pair in pairs for s in pair}
        for _ in range(max(a.reps // 2, 5)):
            for ext in (False, True):
                for s, v in scope_ms(lambda: frame(ext), [pair[ext] for pair in pairs]).items():
                    samples[s].append(v)
        for aux_s, ext_s in pairs:
            ma, me = statistics.median(samples[aux_s]), statistics.median(samples[ext_s])
            print(f"{name}: {aux_s} {1e3 * ma:.1f} us ({1e3 * min(samples[aux_s]):.1f} .. {1e3 * max(samples[aux_s]):.1f}), "
                  f"{ext_s} {1e3 * me:.1f} us ({1e3 * min(samples[ext_s]):.1f} .. {1e3 * max(samples[ext_s]):.1f}), "
                  f"difference {1e3 * (me - ma):+.1f} us ({100 * (me / ma - 1):+.1f} %)")

        # ---- a training step with the normal term on
        def step(mode):
            for p in params:
                p.grad = None
            if mode == "one":
                mp = render_with_normals(cam, model, pipe, bg)
                image = mp["render"]
            else:
                image = render(cam, model, pipe, bg)["render"]
                mp = render_normals(cam, model, pipe) if mode == "two" else None
            loss = training_loss(image, gt)
            if mp is not None:
                loss = loss + 0.05 * NM.normal_consistency_loss(mp["normal"], mp["depth"], mp["alpha"], tx, ty)
            loss.backward()
        m = alternated({"off": lambda: step("off"), "two": lambda: step("two"), "one": lambda: step("one")}, a.reps)
        f = lambda t: f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"
        print(f"{name}: step with lambda_normal off {f(m['off'])}; on, two frames {f(m['two'])}; on, one frame (normal_in_frame) {f(m['one'])}: "
              f"one frame against two {m['one'][0] - m['two'][0]:+.3f} ms ({100 * (m['one'][0] / m['two'][0] - 1):+.1f} %), "
              f"the term costs {m['two'][0] - m['off'][0]:+.3f} ms in two frames, {m['one'][0] - m['off'][0]:+.3f} ms in one")


if __name__ == "__main__":
    main()
