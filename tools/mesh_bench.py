"""Cost of mesh cleaning: `face_components` and `clean_mesh` (with its readback) against their torch twins, against
their bytes model and - for orientation only - against scipy's connected_components on the host with the copy included.  Nothing here
is a gate.

Device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  The meshes: the surface-nets
mesh of the analytic sphere of radius 0.6 in a volume over [-1,1]^3 at the given sizes (one closed component), and the mesh
`scene.mesh.extract_mesh` gives for N cameras of a bench.py configuration in a 512^3 volume (one large surface and many small pieces);
clean_mesh runs with keep_largest=1.  The bytes model is the compulsory traffic of csrc/gsr_mesh.hip as DESIGN section 27 counts it:
face_components 8 V + 48 F (the start; per face its three indices twice, three parent words, a root, a label and a size), the cleaning
stages 3 V + 20.25 F + 8 V' + 43 F' more (V', F': kept), the gathers of positions and colours 76 V'.  The union-find's extra parent
traffic (longer chains, retries) is what the fraction of the copy rate shows.

    python tools/mesh_bench.py [--sizes 256 512] [--reps 30] [--config cfg3n] [--cameras 100] [--no-twin] [--no-scene]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[256, 512])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--config", default="cfg3n")
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--no-twin", action="store_true")
    ap.add_argument("--no-scene", action="store_true")
    a = ap.parse_args()
    from diff_gaussian_rasterization.meshops import clean_mesh, face_components
    from diff_gaussian_rasterization.tsdf import TSDFVolume
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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
        rate, cr = nbytes / (t_ms * 1e-3), copy_rate(int(nbytes))
        return f"{label}: {nbytes / 1e6:.1f} MB by the bytes model -> {rate / 1e12:.3f} TB/s, {100 * rate / cr:.0f} % of the copy rate ({cr / 1e12:.2f} TB/s)"

    def scipy_ms(faces, V):
        """connected_components over the vertices on the host, the copy of the faces included (wall time, median of 3); None without scipy."""
        try:
            import scipy.sparse as sp
            from scipy.sparse.csgraph import connected_components
        except ImportError:
            return None
        runs = []
        for _ in range(3):
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f = faces.cpu().numpy().astype(np.int64)
            rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
            n, _ = connected_components(sp.coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(V, V)), directed=False)
            runs.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(runs), n

    def measure(what, v, f, c):
        V, F = v.shape[0], f.shape[0]
        variants = lambda fn: {"hip": lambda: fn(True)} if a.no_twin else {"hip": lambda: fn(True), "twin": lambda: fn(False)}
        labels, sizes = face_components(f, V, native=True)
        pieces = int((sizes > 0).sum())
        out = clean_mesh(v, f, c, keep_largest=1, native=True)
        Vk, Fk = out[0].shape[0], out[1].shape[0]
        print(f"{what}: V = {V}, F = {F}, {pieces} components; keep_largest=1 keeps V' = {Vk}, F' = {Fk}")
        m = alternated(variants(lambda native: face_components(f, V, native=native)), a.reps)
        line = f"    face_components: HIP {show(m['hip'])}"
        if not a.no_twin:
            line += f", twin {show(m['twin'])}, ratio {m['twin'][0] / m['hip'][0]:.1f}"
        sc = scipy_ms(f, V)
        print(line + (f"; scipy on the host with the copy {sc[0]:.1f} ms ({sc[1]} vertex components, unused vertices among them)" if sc else "; scipy: not installed"))
        comp_bytes = 8 * V + 48 * F
        print("    " + against_copy("face_components", comp_bytes, m["hip"][0]))
        m = alternated(variants(lambda native: clean_mesh(v, f, c, keep_largest=1, native=native)), min(a.reps, 10) if not a.no_twin else a.reps)
        line = f"    clean_mesh (keep_largest=1, readback included): HIP {show(m['hip'])}"
        if not a.no_twin:
            line += f", twin {show(m['twin'])}, ratio {m['twin'][0] / m['hip'][0]:.1f}"
        print(line)
        print("    " + against_copy("clean_mesh", comp_bytes + 3 * V + 20.25 * F + 8 * Vk + 43 * Fk + 76 * Vk, m["hip"][0]))

    for n in a.sizes:
        vol = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), 5 * 2.0 / (n - 1), device=dev)
        ax = torch.linspace(-1.0, 1.0, n, device=dev)
        r = torch.sqrt(ax.view(n, 1, 1) ** 2 + ax.view(1, n, 1) ** 2 + ax.view(1, 1, n) ** 2)
        vol.tsdf.copy_(((r - 0.6) / vol.sdf_trunc).clamp(-1, 1))
        vol.weight.fill_(1.0)
        del r
        v, f, c = vol.extract_mesh(native=True)
        del vol
        torch.cuda.empty_cache()
        measure(f"sphere {n}^3", v, f, c)

    if a.no_scene:
        return
    import scene_synth as S
    from gaussian_params import Pipe
    from scene import GaussianModel, mesh
    cfg = S.CONFIGS[a.config]
    scene, _ = S.make_config(a.config)
    model = GaussianModel(scene.sh_degree)
    model.adopt_scene(scene.to(dev), device=dev)
    cameras = [cam.to(dev) for cam in S.arc_cameras(cfg["W"], cfg["H"], a.cameras)]
    bounds = ((-4.0, -4.0, 0.5), (4.0, 4.0, 8.5))                                  # tools/tsdf_bench.py's cube: 512^3 voxels of 1/64
    v, f, c = mesh.extract_mesh(model, cameras, Pipe(), torch.zeros(3, device=dev), bounds=bounds)
    del model
    torch.cuda.empty_cache()
    measure(f"{a.config}, {a.cameras} cameras, 512^3", v, f, c)


if __name__ == "__main__":
    main()
