"""Cost of the sparse TSDF volume against the dense one: `integrate` and `extract_mesh` of SparseTSDFVolume beside
TSDFVolume's on the same frames in the same process, `allocate` and `commit`, the bricks and bytes the pool takes, and
`extract_mesh(pc, cameras, sparse=...)` end to end.  Nothing here is a gate.

Device events around a call, in alternated windows of 5; every figure is a median with its min .. max.  The scene of the op figures is
tools/tsdf_bench.py's: a 1080p depth map of the sphere of radius 0.6 in a volume over [-1,1]^3, seen by a camera outside the volume and
by one inside it; the sparse volume allocates both frames before it fuses either (two passes).  The bytes model of the sparse
`integrate` is the dense one's compulsory traffic - 40 B per updated voxel, the maps once (20 B per pixel) - plus 12 B of brick
coordinates per allocated brick; the updated voxels are counted from the weights.  `commit` is timed on the host around the call (it
holds the one readback), on a fresh volume each time.  The sizes of --sparse-only run without a dense volume (1024^3 would take
21.5 GB).  The end-to-end figures render N cameras of a bench.py configuration and fuse them at --e2e resolutions: dense, sparse in two
passes and sparse streaming where a dense volume fits (<= 512), sparse two-pass alone above.

    python tools/tsdf_sparse_bench.py [--sizes 256 512] [--sparse-only 1024] [--reps 30] [--config cfg3n] [--cameras 100] [--e2e 512 1024]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

W, H = 1920, 1080


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--sparse-only", nargs="*", type=int, default=[1024])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--config", default="cfg3n")
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--e2e", nargs="*", type=int, default=[512, 1024])
    a = ap.parse_args()
    import scene_synth as S
    import tsdf_ref as TR
    from diff_gaussian_rasterization.tsdf import SparseTSDFVolume, TSDFVolume
    from gaussian_params import Pipe
    from gaussian_renderer import render
    from scene import GaussianModel, mesh
    if not torch.cuda.is_available():
        raise SystemExit("tsdf_sparse_bench needs a GPU: a time taken elsewhere says nothing about the kernels")
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
    grid = lambda n: ((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), 5 * 2.0 / (n - 1))

    def allocate(vol, k):
        fr, (d, al, _, V) = frames[k], maps[k]
        vol.allocate(d, al, V, fr.tanfovx, fr.tanfovy, alpha_min=fr.alpha_min, depth_max=fr.depth_max)

    def integrate(vol, k):
        fr = frames[k]
        vol.integrate(*maps[k], fr.tanfovx, fr.tanfovy, alpha_min=fr.alpha_min, depth_max=fr.depth_max)

    for n in list(a.sizes) + list(a.sparse_only):
        with_dense = n in a.sizes
        commits = []
        for _ in range(5):                                                       # allocate both frames, then one commit, on fresh volumes
            sp = SparseTSDFVolume(*grid(n), device=dev)
            for k in frames:
                allocate(sp, k)
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            sp.commit()
            torch.cuda.synchronize(dev)
            commits.append((time.perf_counter() - t0) * 1e3)
        m = alternated({k: (lambda k=k: allocate(sp, k)) for k in frames}, a.reps)
        sp._pending = False                                                      # (the timed allocates marked what is allocated already)
        sp._marks.zero_()
        dense_bytes = 20 * n ** 3
        pool_bytes = 20 * 512 * sp.capacity + 8 * sp.brick_table.numel() + 20 * sp.capacity
        print(f"sparse {n}^3: {sp.num_bricks} of {sp.brick_table.numel()} bricks allocated by the two frames; pool {pool_bytes / 1e6:.1f} MB with its "
              f"tables, {100 * pool_bytes / dense_bytes:.1f} % of the dense volume's {dense_bytes / 1e6:.1f} MB")
        print(f"    allocate 1080p: " + ", ".join(f"camera {k} {show(m[k])}" for k in frames)
              + f"; commit {statistics.median(commits):.3f} ms ({min(commits):.3f} .. {max(commits):.3f}) on the host, readback included")
        dn = TSDFVolume(*grid(n), device=dev) if with_dense else None
        for k in frames:
            before = sp.weight.clone()
            integrate(sp, k)
            updated = int((sp.weight != before).sum())
            if with_dense:
                integrate(dn, k)
            fns = {"sparse": lambda k=k: integrate(sp, k)}
            if with_dense:
                fns["dense"] = lambda k=k: integrate(dn, k)
            m = alternated(fns, a.reps)
            line = f"integrate {n}^3, 1080p, camera {k}: {updated} voxels updated ({100 * updated / n ** 3:.1f} % of the grid); sparse {show(m['sparse'])}"
            if with_dense:
                line += f", dense {show(m['dense'])}, dense / sparse {m['dense'][0] / m['sparse'][0]:.2f}"
            print(line)
            print("    " + against_copy("sparse integrate", 40 * updated + 20 * H * W + 12 * sp.num_bricks, m["sparse"][0]))
        fns = {"sparse": lambda: sp.extract_mesh()}
        if with_dense:
            fns["dense"] = lambda: dn.extract_mesh()
        v, f, _ = sp.extract_mesh()
        m = alternated(fns, min(a.reps, 10))
        line = f"extract_mesh {n}^3: V = {v.shape[0]}, F = {f.shape[0]}; sparse {show(m['sparse'])}"
        if with_dense:
            dv, df, _ = dn.extract_mesh()
            line += f", dense {show(m['dense'])} (V = {dv.shape[0]}, F = {df.shape[0]}), dense / sparse {m['dense'][0] / m['sparse'][0]:.2f}"
        print(line)
        del sp, dn
        torch.cuda.empty_cache()

    # ---- end to end
    if not a.e2e:
        return
    cfg = S.CONFIGS[a.config]
    scene, _ = S.make_config(a.config)
    model = GaussianModel(scene.sh_degree)
    model.adopt_scene(scene.to(dev), device=dev)
    cameras = [c.to(dev) for c in S.arc_cameras(cfg["W"], cfg["H"], a.cameras)]
    bg, pipe = torch.zeros(3, device=dev), Pipe()
    bounds = ((-4.0, -4.0, 0.5), (4.0, 4.0, 8.5))                                  # tools/tsdf_bench.py's cube of side 8 around the scene
    with torch.no_grad():
        render(cameras[0], model, pipe, bg, depth_alpha=True)
    for res in a.e2e:
        variants = {"sparse two-pass": dict(sparse=True), "sparse streaming": dict(sparse=True, two_pass=False)}
        if res <= 512:
            variants = {"dense": dict(sparse=False), **variants}
        else:
            variants.pop("sparse streaming")
        for name, kw in variants.items():
            runs = []
            for _ in range(3):
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                v, f, _ = mesh.extract_mesh(model, cameras, pipe, bg, bounds=bounds, resolution=res, **kw)
                torch.cuda.synchronize(dev)
                runs.append((time.perf_counter() - t0) * 1e3)
            print(f"extract_mesh(pc, cameras) at {a.config}, {a.cameras} cameras, {res}^3, {name}: V = {v.shape[0]}, F = {f.shape[0]}; "
                  f"{statistics.median(runs):.1f} ms ({min(runs):.1f} .. {max(runs):.1f}) wall")
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
