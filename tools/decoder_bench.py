"""Cost of the latent structured model's decoder: forward + backward with every gradient wanted, the HIP path
(csrc/gsr_decoder.hip: one launch forward, k_decoder_bwd + k_decoder_reduce backward) against the torch decoder the model runs with
native_decode=False (scene.latent_gaussian_model.Decoder: the module call itself), alternated in one process; and one whole
LatentGaussianModel step (decode + compose + render() + fused loss + backward) at 1920x1080 with the decoder either way.

Device time by events around each step.  30 warm-up steps and 300 timed steps per path, alternated in blocks of 10, in each of
two fresh processes (started one after the other by this tool); the report is the median and p10-p90 over both processes' steps.
Per shape it also prints the library's own per-kernel times (decoder_fwd / decoder_bwd / decoder_reduce scopes) against the bytes
the op has to move:
    forward    read the input row, write the decoder row                                   4 B (IN + OUT)
    backward   read the input row and the incoming gradient, write d latents              4 B (IN + L + OUT) + the weights
prints one JSON line per shape and one for the model step at the end.

    python tools/decoder_bench.py [--shapes 125000,8,1,0 125000,8,16,0 125000,8,1,1 125000,8,16,1] [--steps 300] [--warmup 30]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))
BLOCK = 10


def timed(torch, fn, n):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def alternate(torch, paths, steps, warmup):
    """{name: step function} -> {name: [ms]}: warm every path, then blocks of BLOCK steps of each in turn."""
    for fn in paths.values():
        timed(torch, fn, warmup)
    times = {k: [] for k in paths}
    for _ in range(max(steps // BLOCK, 1)):
        for k, fn in paths.items():
            times[k] += timed(torch, fn, BLOCK)
    return times


def child(a):
    import torch
    from diff_gaussian_rasterization import _native as N
    from diff_gaussian_rasterization.decoder import decode_structures
    from scene.latent_gaussian_model import Decoder, LatentGaussianModel, positional_embedding
    assert torch.cuda.is_available(), "decoder_bench measures on a GPU: there is no CPU figure to report"
    dev = torch.device("cuda:0")
    out = []
    for shape in a.shapes:
        B, K, M, pos = (int(x) for x in shape.split(","))
        L, OUT, P0 = 32, K * (11 + 3 * M), 63 if pos else 0
        IN = L + P0
        torch.manual_seed(7)
        dec = Decoder(L, 32, OUT, P0).to(dev)
        latents = torch.randn(B, L, device=dev, requires_grad=True)
        emb = positional_embedding(torch.randn(B, 3, device=dev)) if pos else None
        G = torch.randn(B, OUT, device=dev)
        params = [dec.lin0.weight, dec.lin0.bias, dec.lin1.weight, dec.lin1.bias, dec.lin2.weight, dec.lin2.bias]
        leaves = [latents] + params
        hip = lambda: torch.autograd.grad(decode_structures(latents, *params, pos_emb=emb, native=True), leaves, G)
        ref = lambda: torch.autograd.grad(dec(latents, emb), leaves, G)
        for x, y in zip(hip(), ref()):                       # the same gradients first
            assert (x - y).abs().max() <= 1e-3 * y.abs().max().clamp_min(1e-6), "the two paths disagree"
        times = alternate(torch, dict(hip=hip, torch=ref), a.steps, a.warmup)
        N.profile_enable(True)
        timed(torch, hip, BLOCK)
        prof = N.profile_read()
        N.profile_enable(False)
        out.append(dict(kind="decoder", B=B, K=K, M=M, pos=pos, IN=IN, OUT=OUT, times=times,
                        kernels={k: prof[k][0] / BLOCK for k in ("decoder_fwd", "decoder_bwd", "decoder_reduce")}))
    if a.model_steps > 0:
        import scene_synth as S
        from gaussian_params import Pipe
        from gaussian_renderer import render
        from loss_utils import training_loss
        W, H, B, K = 1920, 1080, 125_000, 8
        torch.manual_seed(5)
        m = LatentGaussianModel(0, S.make_scene(B, W, H, 0, 5, zmin=1.0).means3D.to(dev), gaussians_per_structure=K)
        with torch.no_grad():
            m.structure_scales.fill_(-5.0)
        cam, bg = S.make_camera(W, H).to(dev), torch.tensor([0.1, 0.2, 0.3], device=dev)
        target = (S.make_grad_image(W, H, 3) * 0.5 + 0.5).to(dev)

        def step(native):
            def run():
                m.native_decode = native
                m.zero_grad(set_to_none=True)
                m()
                training_loss(render(cam, m, Pipe(), bg)["render"], target, 0.2).backward()
            return run

        times = alternate(torch, dict(hip=step(True), torch=step(False)), a.model_steps, a.warmup)
        out.append(dict(kind="lgm_step", B=B, K=K, M=1, width=W, height=H, times=times))
    print("CHILD " + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["125000,8,1,0", "125000,8,16,0", "125000,8,1,1", "125000,8,16,1"],
                    help="B,K,M,pos quadruples (pos: 1 = with the 63-dim positional embedding)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--model-steps", type=int, default=100, help="timed steps per path of the whole model step (0: skip it)")
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--processes", type=int, default=2)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    runs = []
    for _ in range(a.processes):                             # fresh processes, one after the other
        text = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], text=True)
        runs.append(json.loads([line for line in text.splitlines() if line.startswith("CHILD ")][-1][6:]))
    q = lambda v: statistics.quantiles(v, n=10)
    results = []
    for rows in zip(*runs):
        r = {k: v for k, v in rows[0].items() if k not in ("times", "kernels")}
        for path in ("hip", "torch"):
            t = [x for row in rows for x in row["times"][path]]
            r[path + "_ms_median"], r[path + "_ms_p10"], r[path + "_ms_p90"] = statistics.median(t), q(t)[0], q(t)[-1]
            r[path + "_ms_median_per_process"] = [statistics.median(row["times"][path]) for row in rows]
        r["steps"] = len(t)
        r["speedup"] = r["torch_ms_median"] / r["hip_ms_median"]
        line = (f"HIP {r['hip_ms_median']:.3f} ms (p10 {r['hip_ms_p10']:.3f}, p90 {r['hip_ms_p90']:.3f})   torch "
                f"{r['torch_ms_median']:.3f} ms (p10 {r['torch_ms_p10']:.3f}, p90 {r['torch_ms_p90']:.3f})   x{r['speedup']:.2f}")
        if r["kind"] == "decoder":
            B, IN, OUT = r["B"], r["IN"], r["OUT"]
            weights = 4 * (32 * IN + 32 * 32 + OUT * 32 + 64 + OUT)
            r["bytes_fwd"], r["bytes_bwd"] = 4 * B * (IN + OUT), 4 * B * (IN + 32 + OUT) + weights
            for k in ("decoder_fwd", "decoder_bwd", "decoder_reduce"):
                r[k + "_ms"] = statistics.mean(row["kernels"][k] for row in rows)
            r["fwd_GBps"] = r["bytes_fwd"] / r["decoder_fwd_ms"] / 1e6
            r["bwd_GBps"] = r["bytes_bwd"] / (r["decoder_bwd_ms"] + r["decoder_reduce_ms"]) / 1e6
            print(f"decoder B={B} K={r['K']} M={r['M']} pos={r['pos']} (IN={IN}, OUT={OUT}): forward+backward  {line}")
            print(f"  kernels: decoder_fwd {r['decoder_fwd_ms'] * 1e3:.1f} us = {r['fwd_GBps']:.0f} GB/s of {r['bytes_fwd'] / 1e6:.1f} MB;  "
                  f"decoder_bwd {r['decoder_bwd_ms'] * 1e3:.1f} us + decoder_reduce {r['decoder_reduce_ms'] * 1e3:.1f} us = "
                  f"{r['bwd_GBps']:.0f} GB/s of {r['bytes_bwd'] / 1e6:.1f} MB")
        else:
            print(f"LGM step B={r['B']} K={r['K']} M={r['M']} at {r['width']}x{r['height']}: {line}")
        results.append(r)
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
