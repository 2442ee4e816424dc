"""Vector quantisation of a [P, D] table: Lloyd's assignment step, the centroid update and the k-means loop over them (the
codebook of scene/compression.py; gsplat's compression strategy, Compact3D and LightGaussian cluster the higher-order SH rows this
way).  DESIGN section 18; C ABI: include/gsrast.h gsr_vq_*.

Device tensors run the HIP kernels (csrc/gsr_vq.hip): the assignment is a fused exact-f32 MFMA product + argmin that never writes
the P x K distances, the update a stable sort and one wave per code, so the same inputs give the same bits.  Host tensors, and
`native=False`, take the same rules as torch ops (the distances in chunks of P; on a device the twin's index_add_ adds in no fixed
order).  `native=True` on host tensors, or on a shape the kernels do not cover, raises: there is no silent fallback.
"""
from __future__ import annotations

import torch

MAX_D = 128                        # gsr_vq_*: 1 <= D <= 128
CHUNK_BYTES = 1 << 30              # assign_torch: a chunk's P x K block of fp32 distances is at most 1 GiB


def _use_native(native, t: torch.Tensor, what: str) -> bool:
    if native is None:
        native = t.is_cuda
    elif native and not t.is_cuda:
        raise RuntimeError(f"{what}: native=True needs device tensors (the HIP kernels have no CPU path)")
    if native and not 1 <= t.shape[1] <= MAX_D:
        raise RuntimeError(f"{what}: D = {t.shape[1]} is outside the kernels' range [1, {MAX_D}] (native=False runs the torch twin)")
    return bool(native)


def _f32c(t: torch.Tensor, what: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError(f"{what}: expected a contiguous float32 tensor, got {t.dtype} (contiguous: {t.is_contiguous()})")
    return t


def _check_shapes(x, codebook, idx, what):
    if x.dim() != 2 or codebook.dim() != 2 or x.shape[1] != codebook.shape[1]:
        raise ValueError(f"{what}: x must be [P, D] and codebook [K, D], got {tuple(x.shape)} and {tuple(codebook.shape)}")
    if codebook.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"{what}: K = {codebook.shape[0]} and D = {x.shape[1]} must be at least 1")
    if x.device != codebook.device:
        raise ValueError(f"{what}: x is on {x.device}, the codebook on {codebook.device}")
    if idx is not None:
        if idx.dtype != torch.int32 or idx.shape != x.shape[:1] or not idx.is_contiguous() or idx.device != x.device:
            raise ValueError(f"{what}: idx must be a contiguous [P] int32 tensor on x's device, got {idx.dtype} {tuple(idx.shape)} on {idx.device}")


def assign_torch(x, codebook):
    """The rule as torch ops: |c|^2 - 2 x.c per (point, code), argmin at the lowest index, + |x|^2 clamped at 0, in chunks of P
    whose P x K block is at most CHUNK_BYTES -> (idx int32 [P], dist2 [P])."""
    _check_shapes(x, codebook, None, "assign_torch")
    P, K = x.shape[0], codebook.shape[0]
    idx = torch.empty(P, dtype=torch.int32, device=x.device)
    dist2 = torch.empty(P, dtype=x.dtype, device=x.device)
    cn = (codebook * codebook).sum(1)
    ct = codebook.t()
    step = max(1, CHUNK_BYTES // (4 * K))
    for b in range(0, P, step):
        xc = x[b:b + step]
        score, j = torch.addmm(cn[None], xc, ct, alpha=-2.0).min(1)
        idx[b:b + step] = j
        dist2[b:b + step] = ((xc * xc).sum(1) + score).clamp_min(0)
    return idx, dist2


def update_codebook_torch(x, idx, codebook):
    """Each code -> the mean of its members (index_add_ and a division); a code without a member keeps its row; an index outside
    [0, K) is no one's member -> (new_codebook [K, D], counts int32 [K])."""
    _check_shapes(x, codebook, idx, "update_codebook_torch")
    K = codebook.shape[0]
    j = idx.long()
    ok = (j >= 0) & (j < K)
    if not bool(ok.all()):
        x, j = x[ok], j[ok]
    counts = torch.bincount(j, minlength=K)
    sums = torch.zeros_like(codebook).index_add_(0, j, x)
    new = torch.where(counts[:, None] > 0, sums / counts.clamp_min(1)[:, None].to(x.dtype), codebook)
    return new, counts.to(torch.int32)


def assign(x, codebook, native=None):
    """x [P, D], codebook [K, D] -> (idx int32 [P], dist2 float32 [P]): the nearest code of every row (ties to the lowest index) and
    its squared distance.  Nothing is written to the inputs."""
    _check_shapes(x, codebook, None, "assign")
    x, codebook = _f32c(x.detach(), "x"), _f32c(codebook.detach(), "codebook")
    if _use_native(native, x, "assign"):
        from . import _native
        return _native.vq_assign(x, codebook)
    return assign_torch(x, codebook)


def update_codebook(x, idx, codebook, native=None):
    """-> (new_codebook [K, D], counts int32 [K]): every code becomes the mean of the rows assigned to it; a code without a member
    keeps its row bit for bit."""
    _check_shapes(x, codebook, idx, "update_codebook")
    x, codebook = _f32c(x.detach(), "x"), _f32c(codebook.detach(), "codebook")
    if _use_native(native, x, "update_codebook"):
        from . import _native
        return _native.vq_update(x, idx, codebook)
    return update_codebook_torch(x, idx, codebook)


def kmeans(x, K, iters=10, generator=None, native=None, init=None):
    """Lloyd's algorithm on the rows of x [P, D] -> (codebook [K', D], idx int32 [P]) with K' = min(K, P).

    The initial codebook is the rows `init` ([K'] int64) or, by default, torch.randperm(P, generator=generator)[:K'] (host
    sampling).  The column mean is subtracted before clustering and added back to the codebook: the |c|^2 - 2 x.c form loses digits
    on a cloud far from the origin.  `iters` rounds of assign + update_codebook, then one more assign, so that idx belongs to the
    codebook that is returned."""
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError(f"kmeans: x must be [P, D] with D >= 1, got {tuple(x.shape)}")
    if int(K) < 1 or int(iters) < 0:
        raise ValueError(f"kmeans: K = {K} must be at least 1 and iters = {iters} at least 0")
    x = _f32c(x.detach(), "x")
    P = x.shape[0]
    Kp = min(int(K), P)
    if P == 0:
        return x.new_zeros(0, x.shape[1]), torch.empty(0, dtype=torch.int32, device=x.device)
    use = _use_native(native, x, "kmeans")
    if init is None:
        init = torch.randperm(P, generator=generator)[:Kp]
    elif init.shape != (Kp,):
        raise ValueError(f"kmeans: init must hold K' = {Kp} row indices, got {tuple(init.shape)}")
    mean = x.mean(0)
    xc = (x - mean).contiguous()
    codebook = xc[init.to(x.device)].contiguous()
    for _ in range(int(iters)):
        idx, _d = assign(xc, codebook, use)
        codebook, _n = update_codebook(xc, idx, codebook, use)
    idx, _d = assign(xc, codebook, use)
    return codebook + mean, idx
