"""Cost of the latent structured model's composition: compose_structures forward + backward, the HIP path (csrc/gsr_structured.hip,
one launch each way) against the torch composition of the same tree (native=False), alternated in one process.

Device time by events around each forward + backward (every output receives a gradient, every input wants one: the training
case).  Prints, per shape, the median and the spread of both paths, the library's own per-kernel times (structured_fwd /
structured_bwd scopes) and the rate they achieve against the bytes the algorithm has to move:
    forward   per child: read D floats of the decoder row, write 11 + 3 M              -> 4 (2 D) bytes (+ 44 B per structure)
    backward  per child: read the 11 + 3 M incoming gradients and the row's 4 quaternion floats, write D -> 4 (2 D + 4) bytes
                         (+ 44 B read and 44 B written per structure)
prints one JSON line per shape at the end.

    python tools/structured_bench.py [--shapes 125000,8,1 125000,8,16] [--steps 200] [--warmup 20]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "structured-gaussian-splatting_amd"))

import torch  # noqa: E402


def bytes_model(B, K, M):
    D, P = 11 + 3 * M, B * K
    return 4 * (P * 2 * D + 11 * B), 4 * (P * (2 * D + 4) + 22 * B)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["125000,8,1", "125000,8,16"], help="B,K,M triples")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    from diff_gaussian_rasterization import _native as N
    from diff_gaussian_rasterization.structured import compose_structures
    assert torch.cuda.is_available(), "structured_bench measures on a GPU: there is no CPU figure to report"
    dev = torch.device("cuda:0")
    results = []
    for shape in a.shapes:
        B, K, M = (int(x) for x in shape.split(","))
        D, P = 11 + 3 * M, B * K
        g = torch.Generator().manual_seed(7)
        inputs = [torch.randn(*s, generator=g).to(dev).requires_grad_(True) for s in ((B, K * D), (B, 3), (B, 1), (B, 3), (B, 4))]
        grads = [torch.randn(*s, generator=g).to(dev) for s in ((P, 3), (P, 1), (P, 3), (P, 4), (P, M, 3))]

        def step(native):
            outs = compose_structures(*inputs, K, M, native=native)
            return torch.autograd.grad(outs, inputs, grads)

        def timed(native, n):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
            for e0, e1 in ev:
                e0.record()
                step(native)
                e1.record()
            torch.cuda.synchronize(dev)
            return [e0.elapsed_time(e1) for e0, e1 in ev]

        # same results first (rotation to fp32 rounding, the rest bit for bit), then warm both paths
        # (a child whose product has |q_w| at rounding level may take the other sign on either path: a handful of rows at most)
        for x, y in zip(step(True), step(False)):
            off = ((x - y).abs() > 1e-4 * y.abs().clamp_min(1.0)).float().mean().item()
            assert off <= 1e-5, f"the two paths disagree on {off:.2e} of a gradient's elements"
        for native in (True, False):
            timed(native, a.warmup)
        times = {True: [], False: []}
        block = 10
        for _ in range(max(a.steps // block, 1)):                  # alternate in blocks of 10 steps
            for native in (True, False):
                times[native] += timed(native, block)
        N.profile_enable(True)
        timed(True, block)
        prof = N.profile_read()
        N.profile_enable(False)
        k_fwd, k_bwd = prof["structured_fwd"][0] / block, prof["structured_bwd"][0] / block
        b_fwd, b_bwd = bytes_model(B, K, M)
        q = lambda v: statistics.quantiles(v, n=10)
        r = dict(B=B, K=K, M=M, P=P, steps=len(times[True]),
                 hip_ms_median=statistics.median(times[True]), hip_ms_p10=q(times[True])[0], hip_ms_p90=q(times[True])[-1],
                 torch_ms_median=statistics.median(times[False]), torch_ms_p10=q(times[False])[0], torch_ms_p90=q(times[False])[-1],
                 kernel_fwd_ms=k_fwd, kernel_bwd_ms=k_bwd, bytes_fwd=b_fwd, bytes_bwd=b_bwd,
                 fwd_GBps=b_fwd / k_fwd / 1e6, bwd_GBps=b_bwd / k_bwd / 1e6)
        r["speedup"] = r["torch_ms_median"] / r["hip_ms_median"]
        results.append(r)
        print(f"B={B} K={K} M={M} (P={P}): forward+backward  HIP {r['hip_ms_median']:.3f} ms (p10 {r['hip_ms_p10']:.3f}, p90 {r['hip_ms_p90']:.3f})"
              f"   torch {r['torch_ms_median']:.3f} ms (p10 {r['torch_ms_p10']:.3f}, p90 {r['torch_ms_p90']:.3f})   x{r['speedup']:.1f}")
        print(f"  kernels: structured_fwd {k_fwd * 1e3:.1f} us = {r['fwd_GBps']:.0f} GB/s of {b_fwd / 1e6:.1f} MB;  "
              f"structured_bwd {k_bwd * 1e3:.1f} us = {r['bwd_GBps']:.0f} GB/s of {b_bwd / 1e6:.1f} MB")
    for r in results:
        print(json.dumps(r))


if __name__ == "__main__":
    main()
