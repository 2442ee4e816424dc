"""The compressed checkpoint of a GaussianModel (gsplat's compression strategy, Compact3D, LightGaussian): a k-means codebook over
the higher-order SH rows, 8-bit affine quantisation of the narrow attributes, positions as they are.  DESIGN section 18.

One np.savez archive, readable with allow_pickle=False:
  version int32, sh_degree int32
  xyz                                    float32 [P, 3]
  f_dc, opacity, scaling, rotation       uint8 [P, C], each with <name>_min / <name>_max float32 [C] (per column)
  codebook float32 [K', 3 (M - 1)], indices uint16 [P] (int32 when K' > 65536)      absent at SH degree 0
A uint8 column decodes as min + q (max - min) / 255: within half a step of the original, and a constant column exactly.  f_rest
decodes as codebook[indices], the rows in the model's own layout ([P, M - 1, 3] flattened).  At SH degree 3 that is 12 + 11 + 2 =
25 bytes per Gaussian plus the codebook, against the PLY's 236.

A device model clusters with the HIP kernels of diff_gaussian_rasterization.vq, a host model with their torch twins.
"""
from __future__ import annotations

import numpy as np
import torch

FORMAT_VERSION = 1
QUANTISED = ("f_dc", "opacity", "scaling", "rotation")
MAX_U16_CODES = 1 << 16


def quantise_u8(v: np.ndarray):
    """v float32 [P, C] -> (q uint8 [P, C], min float32 [C], max float32 [C]): per column, affine, round to nearest (in binary64)."""
    C = v.shape[1]
    if v.shape[0] == 0:
        return np.zeros((0, C), np.uint8), np.zeros(C, np.float32), np.zeros(C, np.float32)
    lo, hi = v.min(0), v.max(0)
    span = hi.astype(np.float64) - lo.astype(np.float64)
    scale = np.divide(255.0, span, out=np.zeros_like(span), where=span > 0)
    q = np.rint((v.astype(np.float64) - lo) * scale).clip(0, 255).astype(np.uint8)
    return q, lo.astype(np.float32), hi.astype(np.float32)


def dequantise_u8(q: np.ndarray, lo: np.ndarray, hi: np.ndarray) -> np.ndarray:
    step = (hi.astype(np.float64) - lo.astype(np.float64)) / 255.0
    return (lo.astype(np.float64) + q.astype(np.float64) * step).astype(np.float32)


def compress(model, sh_clusters=65536, iters=10, generator=None) -> dict:
    """model: a scene.GaussianModel (raw parameters are stored, as save_ply stores them) -> the archive's arrays."""
    from diff_gaussian_rasterization import vq
    P = model._xyz.shape[0]
    host = lambda t: t.detach().reshape(P, -1).cpu().numpy().astype(np.float32)
    out = dict(version=np.int32(FORMAT_VERSION), sh_degree=np.int32(model.max_sh_degree), xyz=host(model._xyz))
    for name, t in (("f_dc", model._features_dc), ("opacity", model._opacity), ("scaling", model._scaling), ("rotation", model._rotation)):
        out[name], out[name + "_min"], out[name + "_max"] = quantise_u8(host(t))
    rest = model._features_rest.detach()
    if rest.shape[1] > 0:
        codebook, idx = vq.kmeans(rest.reshape(P, -1).float().contiguous(), int(sh_clusters), iters=iters, generator=generator)
        out["codebook"] = codebook.cpu().numpy()
        out["indices"] = idx.cpu().numpy().astype(np.uint16 if codebook.shape[0] <= MAX_U16_CODES else np.int32)
    return out


def decompress(d: dict) -> dict:
    """The archive's arrays -> float32 host tensors xyz [P,3], f_dc [P,1,3], f_rest [P,M-1,3], opacity [P,1], scaling [P,3],
    rotation [P,4]."""
    if int(d["version"]) != FORMAT_VERSION:
        raise ValueError(f"compressed checkpoint: format version {int(d['version'])}, this reader knows {FORMAT_VERSION}")
    M = (int(d["sh_degree"]) + 1) ** 2
    xyz = np.asarray(d["xyz"], np.float32)
    P = xyz.shape[0]
    t = {name: dequantise_u8(d[name], d[name + "_min"], d[name + "_max"]) for name in QUANTISED}
    if M > 1:
        codebook, indices = np.asarray(d["codebook"], np.float32), np.asarray(d["indices"]).astype(np.int64)
        if codebook.shape[1] != 3 * (M - 1) or indices.shape != (P,) or (P and not 0 <= indices.min() <= indices.max() < codebook.shape[0]):
            raise ValueError("compressed checkpoint: codebook / indices do not fit the SH degree and the point count")
        rest = codebook[indices] if P else np.zeros((0, 3 * (M - 1)), np.float32)
    else:
        rest = np.zeros((P, 0), np.float32)
    return dict(xyz=torch.from_numpy(xyz.copy()), f_dc=torch.from_numpy(t["f_dc"]).reshape(P, 1, 3),
                f_rest=torch.from_numpy(np.ascontiguousarray(rest)).reshape(P, M - 1, 3), opacity=torch.from_numpy(t["opacity"]).reshape(P, 1),
                scaling=torch.from_numpy(t["scaling"]), rotation=torch.from_numpy(t["rotation"]))


def save_compressed(path, d: dict) -> None:
    with open(path, "wb") as fh:                             # a handle: np.savez would append ".npz" to a bare name
        np.savez(fh, **d)


def load_compressed(path) -> dict:
    with np.load(path, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}
