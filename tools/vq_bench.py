"""The vector-quantisation kernels on the GPU, in one process (DESIGN.md section 18 holds the table this prints).

At P rows of D columns (--points, --dim; default 1 M x 45, the SH degree 3 rest table) and each K of --codes, the median of
--repeats alternated windows timed with device events, with min .. max:
  assign   gsr_vq_assign against vq.assign_torch (addmm + min over chunks of P whose P x K block is at most 1 GiB), in ms, and the
           native leg as TFLOP/s from the 2 P K D model and as a share of the 157 TFLOP/s f32 matrix peak
  update   gsr_vq_update against vq.update_codebook_torch (bincount + index_add_), in ms, and the native leg's bytes (x read once,
           idx read, codebook read and written: 4 P D + 4 P + 8 K D) against the HBM copy rate
--files (default on) also compresses a --points Gaussian SH degree 3 model with the largest K and prints the archive's size beside
the PLY's, and the seconds the whole compress() took."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "structured-gaussian-splatting_amd")]
import torch  # noqa: E402

HBM_BYTES_PER_S = 6.29e12          # float4 copy rate of the part
F32_MATRIX_FLOPS = 157e12          # v_mfma_f32_32x32x2_f32 peak


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / n


def alternated(fns, window, repeats):
    """{name: (median, min, max) seconds per call} of the callables, their windows alternating."""
    counts = {k: max(3, int(window / timed(f, 3))) for k, f in fns.items()}
    runs = {k: [] for k in fns}
    for _ in range(repeats):
        for k, f in fns.items():
            runs[k].append(timed(f, counts[k]))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in runs.items()}


def ms(t):
    return {"ms": round(1e3 * t[0], 3), "ms_min_max": [round(1e3 * t[1], 3), round(1e3 * t[2], 3)]}


def pair(t):
    return {"native": ms(t["native"]), "torch": ms(t["torch"]), "speedup": round(t["torch"][0] / t["native"][0], 2)}


def legs(P, D, K, dev, window, repeats):
    from diff_gaussian_rasterization import vq
    gen = torch.Generator().manual_seed(K)
    centres = torch.randn(max(K // 8, 1), D, generator=gen) * 0.1
    x = (centres[torch.randint(len(centres), (P,), generator=gen)] + 0.03 * torch.randn(P, D, generator=gen)).to(dev)
    x = (x - x.mean(0)).contiguous()
    cb = x[torch.randperm(P, generator=gen)[:K].to(dev)].contiguous()
    out = {"P": P, "D": D, "K": K}
    fns = {"native": lambda: vq.assign(x, cb, native=True), "torch": lambda: vq.assign_torch(x, cb)}
    idx = fns["native"]()[0]
    out["assign_differs_from_torch_at"] = int((idx != fns["torch"]()[0]).sum())       # near-ties the two orders of evaluation break differently
    out["assign"] = pair(alternated(fns, window, repeats))
    t = out["assign"]["native"]["ms"] * 1e-3
    out["assign"]["native_TFLOPs"] = round(2.0 * P * K * D / t * 1e-12, 1)
    out["assign"]["native_share_of_f32_matrix_peak"] = round(2.0 * P * K * D / t / F32_MATRIX_FLOPS, 3)
    print(json.dumps({f"K={K}": {"assign": out["assign"]}}), flush=True)
    fns = {"native": lambda: vq.update_codebook(x, idx, cb, native=True), "torch": lambda: vq.update_codebook_torch(x, idx, cb)}
    for f in fns.values():
        f()
    out["update"] = pair(alternated(fns, window, repeats))
    t = out["update"]["native"]["ms"] * 1e-3
    nbytes = 4.0 * P * D + 4.0 * P + 8.0 * K * D
    out["update"]["native_TBps"] = round(nbytes / t * 1e-12, 3)
    out["update"]["native_share_of_hbm_rate"] = round(nbytes / t / HBM_BYTES_PER_S, 3)
    print(json.dumps({f"K={K}": {"update": out["update"]}}), flush=True)
    return out


def file_sizes(P, K, dev):
    import scene_synth as S
    from scene.gaussian_model import GaussianModel
    m = GaussianModel(3)
    m.adopt_scene(S.make_scene(P, 1920, 1080, 3, 1), device=dev)
    with tempfile.TemporaryDirectory() as d:
        ply, gsq = os.path.join(d, "model.ply"), os.path.join(d, "model.gsq")
        m.save_ply(ply)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        m.save_compressed(gsq, sh_clusters=K, generator=torch.Generator().manual_seed(0))
        dt = time.perf_counter() - t0
        out = {"P": P, "sh_clusters": K, "ply_bytes": os.path.getsize(ply), "compressed_bytes": os.path.getsize(gsq),
               "save_compressed_s": round(dt, 2)}
    out["ratio"] = round(out["ply_bytes"] / out["compressed_bytes"], 2)
    print(json.dumps({"files": out}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=45)
    ap.add_argument("--codes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--window", type=float, default=0.5, help="seconds of calls per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-files", dest="files", action="store_false", help="skip the compressed file against its PLY")
    ap.add_argument("--out", default=None, help="also write the result as JSON to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vq_bench.py measures on the GPU: no device found")
    dev = "cuda:0"
    result = {"device": torch.cuda.get_device_name(0), "kernels": [legs(a.points, a.dim, K, dev, a.window, a.repeats) for K in a.codes]}
    if a.files:
        result["files"] = file_sizes(a.points, max(a.codes), dev)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1)
    print(json.dumps({"vq_bench": "done"}))


if __name__ == "__main__":
    main()
