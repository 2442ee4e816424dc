"""LatentGaussianModel — the reference's structured model (scene/latent_gaussian_model.py, trained by train_lgm.py): B structures,
each with a mean, an opacity logit, a log-scale, a rotation and a latent; a small MLP decodes every latent into K child Gaussians
of D = 11 + 3 M floats, and each child is composed with its structure (means, opacity logits and log-scales are added, the
quaternions normalised, multiplied and standardised).  The composed children are what the rasterizer renders.

Same constructor, parameter and buffer names (checkpoints move both ways through state_dict / load_state_dict), initial values,
decoder and composition rules as the reference class.  Laid out for this package's rasterizer:
  * the decoder is torch ops by default; `native_decode = True` (or None) runs it as ONE HIP launch forward and two backward on
    the same parameters (diff_gaussian_rasterization.decoder.decode_structures);
  * the composition is ONE HIP launch forward and one backward (diff_gaussian_rasterization.structured.compose_structures)
    instead of about twenty torch kernels each way; host tensors take the same rules as torch ops;
  * its results `_xyz, _opacity, _scaling, _rotation` and ONE interleaved SH table `_features` [P,M,3] (`_features_dc` /
    `_features_rest` are views of it) are exactly what render()'s fused raw path consumes (`packed_features`), so no getter and no
    torch.cat runs between the decoder and the rasterizer.
Stands beside scene.GaussianModel rather than on it: that class owns a table of leaf parameters with Adam moments that follow
their rows; here the per-Gaussian tensors are results, recomputed by every forward().
"""
from __future__ import annotations

import os
from typing import Optional

import numpy as np
import torch
from torch import nn

from . import ply_io
from .activations import ActivationCache
from .gaussian_model import SH_C0, inverse_sigmoid, quat_to_rotmat

_HOST_BUFFERS = ("max_sh_degree", "active_sh_degree")


def positional_embedding(xyz: torch.Tensor, multires: int = 10) -> torch.Tensor:
    """[B,3] -> [B, 3 + 6 multires]: the input, then sin and cos of it at the frequencies 2^0 .. 2^(multires-1)."""
    parts = [xyz]
    for f in 2.0 ** torch.linspace(0.0, multires - 1, steps=multires):
        parts += [torch.sin(xyz * f), torch.cos(xyz * f)]
    return torch.cat(parts, -1)


class Decoder(nn.Module):
    """latent (+ positional dims in FRONT of it) -> hidden -> hidden -> out: plain Linear layers with ReLU, the second hidden layer
    with a residual connection; no norm, no dropout, no output activation."""

    def __init__(self, latent_size: int, hidden_size: int, out_size: int, pos_emb_size: int = 0):
        super().__init__()
        self.lin0 = nn.Linear(latent_size + pos_emb_size, hidden_size)
        self.lin1 = nn.Linear(hidden_size, hidden_size)
        self.lin2 = nn.Linear(hidden_size, out_size)

    def forward(self, latents: torch.Tensor, pos_emb: Optional[torch.Tensor] = None) -> torch.Tensor:
        x = latents if pos_emb is None else torch.cat((pos_emb, latents), dim=1)
        x = torch.relu(self.lin0(x))
        x = torch.relu(self.lin1(x) + x)
        return self.lin2(x)


class LatentGaussianModel(nn.Module):
    packed_features = True                                   # _features_dc / _features_rest are views of _features [P,M,3]

    def __init__(self, sh_degree: int, structure_means_init: torch.Tensor, latent_size: int = 32, hidden_size: int = 32,
                 gaussians_per_structure: int = 8, use_positional_embedding: bool = False, positional_embedding_multires=None):
        super().__init__()
        assert structure_means_init.dim() == 2 and structure_means_init.shape[1] == 3, "structure_means_init must be N by 3!"
        self.sh_degree = sh_degree
        self.sh_coeffs = (sh_degree + 1) ** 2
        self.gaussian_parameters_size = 11 + 3 * self.sh_coeffs          # mean, opacity, scale, quaternion | colour
        self.latent_size, self.hidden_size = latent_size, hidden_size
        self.num_structures = len(structure_means_init)
        self.gaussians_per_structure = gaussians_per_structure
        self.use_positional_embedding = use_positional_embedding
        if use_positional_embedding and positional_embedding_multires is None:
            positional_embedding_multires = 10
        self.positional_embedding_multires = positional_embedding_multires

        B, device = self.num_structures, structure_means_init.device
        self.structure_means = nn.Parameter(structure_means_init)
        self.structure_opacities = nn.Parameter(inverse_sigmoid(torch.ones((B, 1), device=device) * 0.1))
        self.structure_scales = nn.Parameter(torch.ones((B, 3), device=device))
        self.structure_rotations = nn.Parameter(torch.randn((B, 4), device=device))
        self.structure_latents = nn.Parameter(torch.randn((B, latent_size), device=device))
        pos = 3 + 6 * positional_embedding_multires if use_positional_embedding else 0
        self.decoder = Decoder(latent_size, hidden_size, self.gaussian_parameters_size * gaussians_per_structure, pos).to(device)
        # in the state_dict, as the reference has them.  The two degrees are read by the host for every frame (render() passes
        # int(active_sh_degree) to the rasterizer): they stay host tensors wherever the module moves (_apply below)
        self.register_buffer("max_sh_degree", torch.tensor(sh_degree, dtype=torch.int))
        self.register_buffer("active_sh_degree", torch.tensor(0, dtype=torch.int))
        self.register_buffer("max_radii2D", torch.empty(0))

        self.freeze_structure_means = self.freeze_structure_scales = False
        self.freeze_structure_rotations = self.freeze_structure_opacities = False
        self.freeze_means = self.freeze_scales = self.freeze_rotations = self.freeze_opacities = False
        self.native_compose = None           # None: the HIP composition for GPU tensors, torch ops for host tensors; False: torch ops
        # False: self.decoder as torch ops; True: the fused HIP decoder (diff_gaussian_rasterization.decoder.decode_structures) on the
        # same parameters, an error where it does not apply; None: the HIP decoder where it applies, torch ops elsewhere
        self.native_decode = False
        self._decoded = self._xyz = self._opacity = self._scaling = self._rotation = self._features = None
        self._acts = ActivationCache()
        self.optimizer = None
        self.percent_dense = 0.0
        self.spatial_lr_scale = 0.0

    def _apply(self, fn, *args, **kwargs):
        host = {k: self._buffers[k] for k in _HOST_BUFFERS}
        super()._apply(fn, *args, **kwargs)
        self._buffers.update(host)
        return self

    def set_freeze_structures_params(self, frozen: bool):
        self.freeze_structure_means = self.freeze_structure_scales = frozen
        self.freeze_structure_rotations = self.freeze_structure_opacities = frozen

    # ---- decode and compose ----------------------------------------------------------------------------------
    def forward(self, latent_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Decodes and composes; the children are left in `_xyz, _opacity, _scaling, _rotation, _features`.  Returns the decoder's
        output as [P, D] (uncomposed), as the reference does."""
        from diff_gaussian_rasterization.structured import compose_structures
        latents = self.structure_latents
        if latent_noise is not None:
            latents = latents + latent_noise.detach()
        pos = None
        if self.use_positional_embedding:
            pos = positional_embedding(self.structure_means.detach(), self.positional_embedding_multires)
        if self.native_decode is False:
            decoded = self.decoder(latents, pos)
        else:
            from diff_gaussian_rasterization.decoder import decode_structures
            d = self.decoder
            decoded = decode_structures(latents, d.lin0.weight, d.lin0.bias, d.lin1.weight, d.lin1.bias, d.lin2.weight, d.lin2.bias,
                                        pos_emb=pos, native=self.native_decode)
        B, K, D = self.num_structures, self.gaussians_per_structure, self.gaussian_parameters_size
        assert tuple(decoded.shape) == (B, K * D)
        held = lambda p, frozen: p.detach() if frozen else p
        # (the reference detaches structure_scales under the OPACITIES flag, and freeze_structure_scales does nothing: mirrored)
        self._xyz, self._opacity, self._scaling, self._rotation, self._features = compose_structures(
            decoded, held(self.structure_means, self.freeze_structure_means),
            held(self.structure_opacities, self.freeze_structure_opacities),
            held(self.structure_scales, self.freeze_structure_opacities),
            held(self.structure_rotations, self.freeze_structure_rotations), K, self.sh_coeffs, native=self.native_compose)
        self._acts.invalidate()
        self._decoded = decoded              # [B, K D] as the composition read it (its .grad, once retained, is dL/d decoder output)
        return decoded.reshape(B * K, D)

    _features_dc = property(lambda s: s._features[:, :1])
    _features_rest = property(lambda s: s._features[:, 1:])

    # ---- what render() reads -----------------------------------------------------------------------------------
    @property
    def get_xyz(self):
        return self._xyz.detach() if self.freeze_means else self._xyz

    @property
    def get_scaling(self):
        s = self._acts.get(0, self._scaling, self._rotation, self._opacity)
        return s.detach() if self.freeze_scales else s

    @property
    def get_rotation(self):
        r = self._acts.get(1, self._scaling, self._rotation, self._opacity)
        return r.detach() if self.freeze_rotations else r

    @property
    def get_opacity(self):
        o = self._acts.get(2, self._scaling, self._rotation, self._opacity)
        return o.detach() if self.freeze_opacities else o

    @property
    def get_features(self):
        return self._features

    def get_covariance(self, scaling_modifier=1):
        L = quat_to_rotmat(self._rotation) @ torch.diag_embed(self.get_scaling * scaling_modifier)
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)

    def oneupSHdegree(self):
        if int(self.active_sh_degree) < int(self.max_sh_degree):
            self.active_sh_degree += 1

    @property
    def device(self):
        return self.structure_means.device

    # ---- training and IO -----------------------------------------------------------------------------------------
    def create_from_pcd(self, pcd, spatial_lr_scale: float, device="cuda"):
        """One structure per point of `pcd` (`.points` [B,3], `.colors` [B,3] in [0,1]): scales from the 3 nearest neighbours,
        identity rotations, opacity 0.1, and latents that start from (0 mean, 0 opacity, 0 scale, the rotation, the SH colour)."""
        from simple_knn._C import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.as_tensor(np.asarray(pcd.points), dtype=torch.float32, device=device)
        rgb = torch.as_tensor(np.asarray(pcd.colors), dtype=torch.float32, device=device)
        B = pts.shape[0]
        d2 = torch.clamp_min(distCUDA2(pts), 1e-7)
        rots = torch.zeros(B, 4, device=device)
        rots[:, 0] = 1
        latents = torch.randn(B, self.latent_size, device=device)
        latents[:, :7] = 0
        latents[:, 7:11] = rots
        latents[:, 11:14] = (rgb - 0.5) / SH_C0
        self.structure_means = nn.Parameter(pts)
        self.structure_scales = nn.Parameter(torch.log(torch.sqrt(d2))[:, None].repeat(1, 3))
        self.structure_rotations = nn.Parameter(rots)
        self.structure_opacities = nn.Parameter(inverse_sigmoid(torch.full((B, 1), 0.1, device=device)))
        self.structure_latents = nn.Parameter(latents)
        self.num_structures = B
        self.decoder.to(device)
        self.max_radii2D = torch.zeros(B * self.gaussians_per_structure, device=device)

    def training_setup(self, training_args):
        self.percent_dense = training_args.percent_dense
        self.optimizer = torch.optim.Adam(self.parameters(), lr=5e-4, eps=1e-15)

    def save_ply(self, path):
        with torch.no_grad():
            self.forward()
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        n = lambda t: t.detach().cpu().numpy()
        ply_io.write_gaussian_ply(path, n(self._xyz), n(self._features_dc), n(self._features_rest), n(self._opacity),
                                  n(self._scaling), n(self._rotation))
