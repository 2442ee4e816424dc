"""Cost of TSDF fusion and mesh extraction: `integrate` and `extract_mesh` against their torch twins and against
their bytes models, and `extract_mesh(pc, cameras)` end to end.  Nothing here is a gate.

Device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  The scene of the op figures is
synthetic: a 1080p depth map of the sphere of radius 0.6 in a volume over [-1,1]^3, seen by a camera outside the volume and by one
inside it (tests/tsdf_ref.py sphere_frame).  The bytes model of `integrate` is the compulsory traffic of csrc/gsr_tsdf.hip: 40 B per
updated voxel (five floats read and written), 0 per skipped voxel, plus the maps once (20 B per pixel); the updated voxels are counted
from the weights.  `extract_mesh` reads tsdf and weight once in each of its two passes over the volume (16 B per voxel) and writes the
mesh; its time includes the one host readback.  Each native figure is set against the rate of a device copy of as many bytes.  The
end-to-end figure renders N cameras of a bench.py configuration with depth_alpha=True, fuses them into a 512^3 volume around the scene
and extracts the mesh.

    python tools/tsdf_bench.py [--sizes 256 512] [--reps 30] [--config cfg3n] [--cameras 100] [--no-twin]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[256, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--config", default="cfg3n")
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--no-twin", action="store_true")
    a = ap.parse_args()
    import scene_synth as S
    import tsdf_ref as TR
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, mesh
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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
            events(fn, 2)
        times = {k: [] for k in fns}
        for _ in range(max(n // 5, 1)):
            for k, fn in fns.items():
                times[k] += events(fn, 5)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}

    def show(t):
        return f"{t[0]:.3f} ms ({t[1]:.3f} .. {t[2]:.3f})"

    def copy_rate(nbytes):
        src = torch.empty(max(nbytes // 2, 1 << 20), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        events(lambda: dst.copy_(src), 3)
        return 2 * src.numel() / (statistics.median(events(lambda: dst.copy_(src), 20)) * 1e-3)

    def against_copy(label, nbytes, t_ms):
        rate, cr = nbytes / (t_ms * 1e-3), copy_rate(nbytes)
        return f"{label}: {nbytes / 1e6:.1f} MB by the bytes model -> {rate / 1e12:.3f} TB/s, {100 * rate / cr:.0f} % of the copy rate ({cr / 1e12:.2f} TB/s)"

    cams = {"outside": TR.look_at((1.9, -1.2, 0.9), (0.05, 0.0, -0.1), roll=0.35), "inside": TR.look_at((0.12, 0.07, -0.21), (-0.4, 0.3, -0.9), roll=-0.2)}
    frames = {k: TR.sphere_frame(V, W, H, holes=True) for k, V in cams.items()}
    t = lambda x: torch.as_tensor(x).to(dev).contiguous()
    maps = {k: (t(fr.depth)[None], t(fr.alpha)[None], t(fr.color), t(fr.V)) for k, fr in frames.items()}
    for n in a.sizes:
        vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), 5 * 2.0 / (n - 1), device=dev)
        for k, fr in frames.items():
            def fuse(native, k=k, fr=fr):
                vol.integrate(*maps[k], fr.tanfovx, fr.tanfovy, alpha_min=fr.alpha_min, depth_max=fr.depth_max, native=native)
            before = vol.weight.clone()
            fuse(True)
            updated = int((vol.weight != before).sum())
            m = alternated({"hip": lambda: fuse(True)} if a.no_twin else {"hip": lambda: fuse(True), "twin": lambda: fuse(False)}, a.reps)
            line = f"integrate {n}^3, 1080p, camera {k}: {updated} of {n ** 3} voxels updated ({100 * updated / n ** 3:.1f} %); HIP {show(m['hip'])}"
            if not a.no_twin:
                line += f", twin {show(m['twin'])}, ratio {m['twin'][0] / m['hip'][0]:.1f}"
            print(line)
            print("    " + against_copy("integrate", 40 * updated + 20 * H * W, m["hip"][0]))
        # the volume now holds both cameras' frames many times over: the running means are what one pass of each left
        def extract(native):
            return vol.extract_mesh(native=native)
        v, f, _ = extract(True)
        m = alternated({"hip": lambda: extract(True)} if a.no_twin else {"hip": lambda: extract(True), "twin": lambda: extract(False)}, min(a.reps, 10))
        line = f"extract_mesh {n}^3: V = {v.shape[0]}, F = {f.shape[0]}; HIP {show(m['hip'])}"
        if not a.no_twin:
            line += f", twin {show(m['twin'])}, ratio {m['twin'][0] / m['hip'][0]:.1f}"
        print(line)
        print("    " + against_copy("extract_mesh", 16 * n ** 3 + 24 * v.shape[0] + 12 * f.shape[0], m["hip"][0]))
        del vol
        torch.cuda.empty_cache()

    # ---- end to end
    cfg = S.CONFIGS[a.config]
    scene, _ = S.make_config(a.config)
    model = GaussianModel(scene.sh_degree)
    model.adopt_scene(scene.to(dev), device=dev)
    cameras = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], a.cameras)]
    bg, pipe = torch.zeros(3, device=dev), Pipe()
    bounds = ((-4.0, -4.0, 0.5), (4.0, 4.0, 8.5))                                  # a cube of side 8 around the scene: 512^3 voxels of 1/64
    with torch.no_grad():
        render(cameras[0], model, pipe, bg, depth_alpha=True)
    runs = []
    for _ in range(3):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        v, f, _ = mesh.extract_mesh(model, cameras, pipe, bg, bounds=bounds)
        torch.cuda.synchronize(dev)
        runs.append((time.perf_counter() - t0) * 1e3)

    def frames_only():
        with torch.no_grad():
            for cam in cameras:
                render(cam, model, pipe, bg, depth_alpha=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    frames_only()
    torch.cuda.synchronize(dev)
    t_frames = (time.perf_counter() - t0) * 1e3
    print(f"extract_mesh(pc, cameras) at {a.config}, {a.cameras} cameras, 512^3: V = {v.shape[0]}, F = {f.shape[0]}; "
          f"{statistics.median(runs):.1f} ms ({min(runs):.1f} .. {max(runs):.1f}) wall, of which the {a.cameras} depth_alpha frames alone take {t_frames:.1f} ms")


if __name__ == "__main__":
    main()
