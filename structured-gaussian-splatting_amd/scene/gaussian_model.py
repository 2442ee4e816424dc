"""GaussianModel — host-side mirror of the reference's parameter store (scene/gaussian_model.py), the producer
of the rasterizer's inputs and the consumer of its `means2D.grad` / `radii` outputs.

Same public surface and semantics as the reference class (getters :101-128, create_from_pcd :134-157,
training_setup :159-177, update_learning_rate :179-185, PLY IO :201-266, reset_opacity :220-223,
densify_and_prune :399-413, add_densification_stats :415-417, capture/restore :67-99), organised differently:
the per-Gaussian tensors live in ONE table, and every structural edit (prune, clone, split, opacity reset) goes
through a single `_rebuild` that rewrites parameters and Adam moments together.

Two things are laid out for the rasterizer rather than as the reference has them (the producer
side of the hot path; 0.45 ms of a 1.4 ms training step at 1e6 Gaussians when done as torch ops):
  * `_features_dc` [P,1,3] and `_features_rest` [P,M-1,3] are the two column ranges of ONE leaf tensor `_features`
    [P,M,3], so `get_features` (the reference's torch.cat, 384 MB of traffic per call at P = 1e6, and as much again
    in its backward) is that tensor itself: no copy forward, and the rasterizer's dL/dshs IS its gradient.  The
    optimizer keeps the reference's six named groups; "f_dc" holds `_features` and steps its first column with its
    own lr and the others with the lr of the (parameter-less) group "f_rest" — element for element what Adam on the
    two separate tensors does (fused_adam.py, gsr_adam_step_split).
  * `get_scaling`, `get_rotation`, `get_opacity` share one native evaluation (scene/activations.py: one HIP launch
    forward, one backward, for all three) instead of ~20 torch kernels.
Runs on whatever device the tensors live on (host tensors use the reference's torch ops); the native pieces it
calls (activations, optimizer step, rasterizer, distCUDA2) are HIP-only.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass

import numpy as np
import torch
from torch import nn

from . import ply_io
from .activations import ActivationCache

SH_C0 = 0.28209479177387814
GROUPS = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")       # optimizer group order of the reference
TABLE = ("xyz", "features", "opacity", "scaling", "rotation")              # this class's leaf tensors (features = f_dc | f_rest)


def _pack(t: dict) -> dict:
    """Reference-named tensors (f_dc [n,1,3], f_rest [n,M-1,3]) -> table-named ones (features [n,M,3])."""
    if "features" in t:
        return {k: t[k] for k in TABLE}
    out = {k: t[k] for k in TABLE if k != "features"}
    out["features"] = torch.cat((t["f_dc"], t["f_rest"]), dim=1)
    return out


@dataclass
class OptimizationDefaults:
    """arguments/__init__.py:76-95 (pinned by tests/golden/params.json)."""
    iterations: int = 30_000
    position_lr_init: float = 0.00016
    position_lr_final: float = 0.0000016
    position_lr_delay_mult: float = 0.01
    position_lr_max_steps: int = 30_000
    feature_lr: float = 0.0025
    opacity_lr: float = 0.05
    scaling_lr: float = 0.005
    rotation_lr: float = 0.001
    percent_dense: float = 0.01
    lambda_dssim: float = 0.2
    densification_interval: int = 100
    opacity_reset_interval: int = 3000
    densify_from_iter: int = 500
    densify_until_iter: int = 15_000
    densify_grad_threshold: float = 0.0002
    random_background: bool = False
    optimizer_type: str = "default"           # "sparse_adam": step only the Gaussians the frame saw (fused_adam.SparseFusedAdam)
    densify_absgrad: bool = False             # densification statistics from viewspace_points.absgrad (frames rendered with pipe.absgrad)
    densify_strategy: str = "default"         # "mcmc": relocation, 5 % growth to a cap and position noise (GaussianModel.mcmc_*)
    mcmc_cap_max: int = 1_000_000             # the budget of Gaussians the "mcmc" strategy grows to and then keeps
    mcmc_noise_lr: float = 5e5                # position noise scale, times the xyz learning rate
    mcmc_min_opacity: float = 0.005           # at or below it a Gaussian is dead: relocated onto a live one
    mcmc_opacity_reg: float = 0.01            # lambda of mean(opacity)
    mcmc_scale_reg: float = 0.01              # lambda of mean(scale)
    bilateral_grid: bool = False              # a bilateral grid per training image between render() and the loss (train_loop.train)
    bilateral_grid_shape: tuple = (16, 16, 8)     # (grid_x, grid_y, luma levels)
    bilateral_grid_lr: float = 2e-3           # the grids' Adam; warmed up over 1000 iterations, decayed to 1 % (bilagrid.bilateral_grid_lr)
    bilateral_grid_tv: float = 10.0           # weight of the grids' total variation in the loss
    filter_3d: bool = False                   # Mip-Splatting's 3D smoothing filter, recomputed from the training cameras (train_loop.train)
    significance_prune_iterations: tuple = ()     # at the k-th listed iteration: prune by significance over all training cameras (train_loop.train)
    significance_prune_fraction: float = 0.6      # the fraction of the Gaussians the first listed iteration removes (LightGaussian's 60 %)
    significance_prune_decay: float = 0.6         # the k-th removes fraction * decay ** k
    significance_prune_score: str = "volume_weighted"     # GaussianModel.significance's `score`
    densify_error_views: int = 0                  # > 0: refine by image error, scored over that many sampled cameras (train_loop.train); untuned
    densify_error_growth: float = 0.05            # the budget of a refinement: ceil(growth * P) Gaussians are cloned or split; untuned
    densify_error_score: str = "max"              # "max": the largest single view's error (Revising Densification); "sum": over the views (Taming-3DGS)
    lambda_normal: float = 0.0                    # > 0: weight of the normal-consistency loss, one render_normals frame per iteration (train_loop.train); untuned
    normal_from_iter: int = 7000                  # the first iteration that adds it (2DGS's value, not tuned here)
    depth_ratio: float = 0.0                      # in [0, 1], with lambda_normal > 0: the normal term's depth is (1 - r) mean + r median (render_normals; 2DGS: 1 for bounded scenes); untuned
    normal_in_frame: bool = False                 # True: colour and the normal term's maps from ONE render_with_normals frame (train_loop.train)
    lambda_dist: float = 0.0                      # > 0: weight of the depth-distortion loss, taken from the colour frame itself (render_with_distortion; train_loop.train); untuned
    dist_from_iter: int = 3000                    # the first iteration that adds it (2DGS's value, not tuned here)


def expon_lr(lr_init, lr_final, lr_delay_steps=0, lr_delay_mult=1.0, max_steps=1_000_000):
    """Log-linear interpolation lr_init -> lr_final with an optional warm-up (utils/general_utils.py:29-62;
    pinned by tests/golden/lr.npz)."""
    def at(step):
        if step < 0 or (lr_init == 0.0 and lr_final == 0.0):
            return 0.0
        warm = 1.0
        if lr_delay_steps > 0:
            warm = lr_delay_mult + (1 - lr_delay_mult) * math.sin(0.5 * math.pi * min(max(step / lr_delay_steps, 0), 1))
        t = min(max(step / max_steps, 0), 1)
        return warm * math.exp(math.log(lr_init) * (1 - t) + math.log(lr_final) * t)
    return at


def inverse_sigmoid(x):
    return torch.log(x / (1 - x))


def quat_to_rotmat(q):
    """Normalised quaternion (r,x,y,z) -> R, as utils/general_utils.py:78-99."""
    q = q / q.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                        2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                        2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).view(-1, 3, 3)


class GaussianModel:
    def __init__(self, sh_degree: int):
        self.active_sh_degree = 0
        self.max_sh_degree = sh_degree
        self._t = {k: torch.empty(0) for k in TABLE}
        self._acts = ActivationCache()
        self.max_radii2D = torch.empty(0)
        self.xyz_gradient_accum = torch.empty(0)
        self.denom = torch.empty(0)
        self.optimizer = None
        self.percent_dense = 0.0
        self.spatial_lr_scale = 0.0
        self.freeze_means = self.freeze_scales = self.freeze_rotations = self.freeze_opacities = False
        self.densify_absgrad = False
        self.densify_strategy = "default"
        self.filter_3D = None                                # [P,1] buffer of compute_3D_filter, or None: no 3D smoothing filter

    # ---- the reference's attribute names -------------------------------------------------------------------
    packed_features = True                                   # _features_dc / _features_rest are views of _features
    _xyz = property(lambda s: s._t["xyz"])
    _features = property(lambda s: s._t["features"])
    _features_dc = property(lambda s: s._t["features"][:, :1])
    _features_rest = property(lambda s: s._t["features"][:, 1:])
    _opacity = property(lambda s: s._t["opacity"])
    _scaling = property(lambda s: s._t["scaling"])
    _rotation = property(lambda s: s._t["rotation"])

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
        return self._t["features"]                           # = torch.cat((_features_dc, _features_rest), dim=1), see the header

    # ---- the 3D smoothing filter (diff_gaussian_rasterization/filter3d.py) ------------------------------
    def compute_3D_filter(self, cameras, native=None):
        """filter_3D [P,1] from the training cameras: every Gaussian's minimum depth over the cameras that see it, over the largest
        focal length, times sqrt(0.2).  A buffer: recompute it after every edit that adds, removes or moves Gaussians."""
        from diff_gaussian_rasterization.filter3d import compute_filter_3d
        self.filter_3D = compute_filter_3d(self._xyz.detach(), cameras, native=native)

    def checked_filter_3D(self):
        """filter_3D, or None; a filter that a structural edit left behind is an error, never a quiet unfiltered frame."""
        f = self.filter_3D
        if f is not None and f.shape[0] != self._xyz.shape[0]:
            raise ValueError(f"filter_3D has {f.shape[0]} rows for {self._xyz.shape[0]} Gaussians: the model was edited since; "
                             "call compute_3D_filter(cameras)")
        return f

    def _filtered_raw(self):
        """(logits', log-scales') of the filtered model: what render() hands to forward_raw and what the fused PLY stores."""
        from diff_gaussian_rasterization.filter3d import apply_filter_3d
        opacity = self._opacity.detach() if self.freeze_opacities else self._opacity
        scaling = self._scaling.detach() if self.freeze_scales else self._scaling
        return apply_filter_3d(opacity, scaling, self.checked_filter_3D(), raw=True)

    def _filtered(self, which):
        """The activation of the filtered raw parameters, by the getters' own activation (scene/activations.py): the getter path and
        the raw path render the same numbers.  Nothing is kept: each getter evaluates the filter for itself (the raw path is the one
        a training step takes)."""
        logits, log_scales = self._filtered_raw()
        return ActivationCache().get(which, log_scales, self._rotation.detach(), logits)

    @property
    def get_scaling_with_3D_filter(self):
        return self.get_scaling if self.checked_filter_3D() is None else self._filtered(0)

    @property
    def get_opacity_with_3D_filter(self):
        return self.get_opacity if self.checked_filter_3D() is None else self._filtered(2)

    def get_covariance(self, scaling_modifier=1):
        L = quat_to_rotmat(self._rotation) @ torch.diag_embed(self.get_scaling_with_3D_filter * scaling_modifier)
        S = L @ L.transpose(1, 2)
        return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1)

    def oneupSHdegree(self):
        self.active_sh_degree = min(self.active_sh_degree + 1, self.max_sh_degree)

    @property
    def device(self):
        return self._xyz.device

    # ---- initialisation ------------------------------------------------------------------------------------
    def _adopt(self, tensors: dict):
        tensors = _pack(tensors)
        self._t = {k: nn.Parameter(tensors[k].detach().clone().contiguous().requires_grad_(True)) for k in TABLE}
        self._acts.invalidate()
        self.filter_3D = None                                # a new table: the filter of the old one says nothing about it
        P = self._xyz.shape[0]
        self.max_radii2D = torch.zeros(P, device=self.device)

    def create_from_pcd(self, pcd, spatial_lr_scale: float, device="cuda"):
        """pcd: anything with `.points` [P,3] and `.colors` [P,3] in [0,1] (utils/graphics_utils.py:17-20)."""
        from simple_knn._C import distCUDA2
        self.spatial_lr_scale = spatial_lr_scale
        pts = torch.as_tensor(np.asarray(pcd.points), dtype=torch.float32, device=device)
        rgb = torch.as_tensor(np.asarray(pcd.colors), dtype=torch.float32, device=device)
        P, M = pts.shape[0], (self.max_sh_degree + 1) ** 2
        sh = torch.zeros(P, M, 3, device=device)
        sh[:, 0, :] = (rgb - 0.5) / SH_C0
        d2 = torch.clamp_min(distCUDA2(pts), 1e-7)
        rot = torch.zeros(P, 4, device=device)
        rot[:, 0] = 1
        self._adopt(dict(xyz=pts, f_dc=sh[:, :1], f_rest=sh[:, 1:], scaling=torch.log(torch.sqrt(d2))[:, None].repeat(1, 3),
                         rotation=rot, opacity=inverse_sigmoid(torch.full((P, 1), 0.1, device=device))))

    def adopt_scene(self, scene, device="cuda"):
        """Start from a scene_synth.Scene (raw parameters) instead of a point cloud."""
        self.spatial_lr_scale = 1.0
        self.active_sh_degree = scene.sh_degree
        self._adopt({k: v.to(device) for k, v in dict(
            xyz=scene.means3D, f_dc=scene.shs[:, :1], f_rest=scene.shs[:, 1:], scaling=scene.log_scales,
            rotation=scene.raw_rotations, opacity=scene.opacity_logits).items()})

    def training_setup(self, opt):
        P = self._xyz.shape[0]
        self.percent_dense = opt.percent_dense
        self.densify_absgrad = bool(getattr(opt, "densify_absgrad", False))
        strategy = getattr(opt, "densify_strategy", "default")
        if strategy not in ("default", "mcmc"):
            raise ValueError(f"densify_strategy = {strategy!r}: \"default\" or \"mcmc\"")
        if strategy == "mcmc" and self.densify_absgrad:
            raise ValueError("densify_strategy = \"mcmc\" reads no gradient statistics: densify_absgrad cannot be combined with it")
        self.densify_strategy = strategy
        self.xyz_gradient_accum = torch.zeros(P, 1, device=self.device)
        self.denom = torch.zeros(P, 1, device=self.device)
        lrs = dict(xyz=opt.position_lr_init * self.spatial_lr_scale, f_dc=opt.feature_lr, f_rest=opt.feature_lr / 20.0,
                   opacity=opt.opacity_lr, scaling=opt.scaling_lr, rotation=opt.rotation_lr)
        # the reference's six groups, in its order; "f_dc" carries the interleaved SH table and takes the lr of its columns
        # 1.. from the parameter-less group "f_rest" (see the header)
        groups = []
        for k in GROUPS:
            if k == "f_dc":
                groups.append({"params": [self._t["features"]], "lr": lrs[k], "name": k, "head_cols": 1, "tail": "f_rest"})
            elif k == "f_rest":
                groups.append({"params": [], "lr": lrs[k], "name": k})
            else:
                groups.append({"params": [self._t[k]], "lr": lrs[k], "name": k})
        from fused_adam import FusedAdam, SparseFusedAdam   # torch.optim.Adam's arithmetic and state layout; one HIP launch per step
        kind = getattr(opt, "optimizer_type", "default")
        if kind not in ("default", "sparse_adam"):
            raise ValueError(f"optimizer_type = {kind!r}: \"default\" or \"sparse_adam\"")
        cls = SparseFusedAdam if kind == "sparse_adam" else FusedAdam
        self.optimizer = cls(groups, lr=0.0, eps=1e-15, native=getattr(opt, "fused_adam", True) and self.device.type == "cuda")
        self._xyz_lr = expon_lr(opt.position_lr_init * self.spatial_lr_scale, opt.position_lr_final * self.spatial_lr_scale,
                                lr_delay_mult=opt.position_lr_delay_mult, max_steps=opt.position_lr_max_steps)

    def update_learning_rate(self, iteration):
        for g in self.optimizer.param_groups:
            if g["name"] == "xyz":
                g["lr"] = self._xyz_lr(iteration)
                return g["lr"]

    # ---- one primitive for every structural edit -------------------------------------------------------------
    def _rebuild(self, keep=None, extra=None, replace=None):
        """New parameter table = old rows selected by boolean `keep` (all if None), then `extra` rows appended
        (`extra` names its tensors as the table does, or as the reference does with f_dc / f_rest);
        `replace` = {name: tensor} swaps a whole tensor (fresh Adam moments).  Adam moments follow their rows;
        appended rows start with zero moments (the reference's _prune_optimizer / cat_tensors_to_optimizer /
        replace_tensor_to_optimizer in one pass)."""
        if extra is not None:
            extra = _pack(extra)
        done = set()
        for grp in self.optimizer.param_groups if self.optimizer is not None else []:
            if not grp["params"]:
                continue                                      # "f_rest": its columns live in the "f_dc" group's tensor
            name, old = ("features" if grp["name"] == "f_dc" else grp["name"]), grp["params"][0]
            state = self.optimizer.state.pop(old, None)
            if replace is not None and name in replace:
                new = replace[name]
                if state is not None:
                    state["exp_avg"], state["exp_avg_sq"] = torch.zeros_like(new), torch.zeros_like(new)
            else:
                rows = old.detach() if keep is None else old.detach()[keep]
                add = None if extra is None else extra[name]
                new = rows if add is None else torch.cat((rows, add), 0)
                if state is not None:
                    for m in ("exp_avg", "exp_avg_sq"):
                        kept = state[m] if keep is None else state[m][keep]
                        state[m] = kept if add is None else torch.cat((kept, torch.zeros_like(add)), 0)
            new = nn.Parameter(new.contiguous().requires_grad_(True))
            grp["params"][0] = new
            if state is not None:
                self.optimizer.state[new] = state
            self._t[name] = new
            done.add(name)
        for name in TABLE:
            if name in done:
                continue
            if replace is not None and name in replace:
                rows = replace[name]
            else:
                rows = self._t[name].detach() if keep is None else self._t[name].detach()[keep]
                if extra is not None:
                    rows = torch.cat((rows, extra[name]), 0)
            self._t[name] = nn.Parameter(rows.contiguous().requires_grad_(True))
        self._acts.invalidate()

    def _reset_stats(self):
        P = self._xyz.shape[0]
        self.xyz_gradient_accum = torch.zeros(P, 1, device=self.device)
        self.denom = torch.zeros(P, 1, device=self.device)
        self.max_radii2D = torch.zeros(P, device=self.device)

    def prune_points(self, mask):
        keep = ~mask
        self._rebuild(keep=keep)
        self.xyz_gradient_accum, self.denom, self.max_radii2D = self.xyz_gradient_accum[keep], self.denom[keep], self.max_radii2D[keep]

    def reset_opacity(self):
        if self.checked_filter_3D() is None:
            capped = inverse_sigmoid(torch.min(self.get_opacity.detach(), torch.full_like(self._opacity, 0.01)))
        else:
            # Mip-Splatting's: the FILTERED opacity is capped, then taken back through coef = o' / o.  The cap sits 2^-20 under
            # 0.01, so that the filtered opacity of the reset model stays at or under 0.01 through the roundings of the way back
            from diff_gaussian_rasterization.filter3d import apply_filter_3d
            with torch.no_grad():
                coef = apply_filter_3d(torch.ones_like(self._opacity), self.get_scaling.detach(), self.filter_3D)[0]
                cap = torch.full_like(self._opacity, 0.01 * (1 - 2.0 ** -20))
                # (a scale so far under its filter that coef underflows: 0 / 0 would be a NaN, and logit(0) is -inf)
                tiny = torch.finfo(coef.dtype).tiny
                opacity = torch.min(self.get_opacity_with_3D_filter.detach(), cap) / coef.clamp_min(tiny)
                capped = inverse_sigmoid(opacity.clamp(min=tiny, max=1 - 2.0 ** -23))
        self._rebuild(replace={"opacity": capped})

    def _densify_grad(self, viewspace_point_tensor):
        """The tensor whose row norms the statistics accumulate: .grad, or with densify_absgrad the frame's .absgrad."""
        if not self.densify_absgrad:
            return viewspace_point_tensor.grad
        absgrad = getattr(viewspace_point_tensor, "absgrad", None)
        if absgrad is None:
            raise ValueError("densify_absgrad is on but viewspace_points has no .absgrad: the frame was not rendered with pipe.absgrad "
                             "(or no backward ran)")
        return absgrad

    def add_densification_stats(self, viewspace_point_tensor, update_filter):
        grad = self._densify_grad(viewspace_point_tensor)
        self.xyz_gradient_accum[update_filter] += torch.norm(grad[update_filter, :2], dim=-1, keepdim=True)
        self.denom[update_filter] += 1

    def update_densification_stats(self, viewspace_point_tensor, radii):
        """train.py:127-130 in one native pass (gsr_densify_stats): max_radii2D and add_densification_stats for the
        visible set `radii > 0`, without the four boolean-mask compactions (each a host synchronisation).
        densify_absgrad: the same pass over viewspace_points.absgrad ([P,3], the layout of .grad) instead of .grad."""
        grad = self._densify_grad(viewspace_point_tensor)
        if grad is None or not self.max_radii2D.is_cuda:
            vis = radii > 0
            self.max_radii2D[vis] = torch.max(self.max_radii2D[vis], radii[vis])
            self.add_densification_stats(viewspace_point_tensor, vis)
            return
        from diff_gaussian_rasterization import _native
        with torch.cuda.device(radii.device):
            _native.densify_stats(radii.contiguous(), grad.contiguous(), self.max_radii2D, self.xyz_gradient_accum, self.denom)

    def densify_and_prune(self, max_grad, min_opacity, extent, max_screen_size):
        grads = self.xyz_gradient_accum / self.denom
        grads[grads.isnan()] = 0.0
        big = torch.max(self.get_scaling.detach(), dim=1).values > self.percent_dense * extent
        hot = torch.norm(grads, dim=-1) >= max_grad
        self._densify_hot_and_prune(hot, big, min_opacity, extent, max_screen_size)

    def _densify_hot_and_prune(self, hot, big, min_opacity, extent, max_screen_size):
        """Clone the small and split the large Gaussians of the mask `hot` [P], then prune (densify_and_prune's body, whatever chose
        `hot`)."""
        n_before = hot.shape[0]
        # clone: small Gaussians with a large view-space gradient are duplicated in place
        sel = hot & ~big
        self._rebuild(extra={k: self._t[k].detach()[sel] for k in TABLE})
        n_after_clone = self._xyz.shape[0]
        self._reset_stats()
        # split: large ones are replaced by N = 2 samples from themselves, 1.6x smaller
        N = 2
        sel = torch.zeros(n_after_clone, dtype=torch.bool, device=self.device)
        sel[:n_before] = hot & big
        scale_sel = self.get_scaling.detach()[sel].repeat(N, 1)
        offs = torch.normal(mean=torch.zeros_like(scale_sel), std=scale_sel)
        R = quat_to_rotmat(self._rotation.detach()[sel]).repeat(N, 1, 1)
        new = {k: self._t[k].detach()[sel].repeat(N, *([1] * (self._t[k].dim() - 1))) for k in TABLE}
        new["xyz"] = torch.bmm(R, offs.unsqueeze(-1)).squeeze(-1) + self._xyz.detach()[sel].repeat(N, 1)
        new["scaling"] = torch.log(scale_sel / (0.8 * N))
        self._rebuild(extra=new)
        self._reset_stats()
        self.prune_points(torch.cat((sel, torch.zeros(N * int(sel.sum()), dtype=torch.bool, device=self.device))))
        # prune: transparent, or too large on screen / in the world
        drop = (self.get_opacity.detach() < min_opacity).squeeze(-1)
        if max_screen_size:
            drop = drop | (self.max_radii2D > max_screen_size) | (self.get_scaling.detach().max(dim=1).values > 0.1 * extent)
        self.prune_points(drop)

    # ---- error-based densification (diff_gaussian_rasterization/contrib.py) ----------------------------
    DENSIFY_ERROR_SCORES = ("max", "sum")

    def error_stats(self, cameras, targets, pipe=None, bg=None, views=None, correct=None):
        """The error-weighted blend statistics of this model (an ErrorStats): per chosen camera, under torch.no_grad(), a plain render,
        E = l1_error_map(image, target), and a statistics frame with pixel_error=E.  views: the indices of the cameras to use (None:
        all).  correct(image, idx): what stands between render() and the loss in training (a bilateral grid), applied to the image
        before it is compared.  pipe: default Pipe(); bg: default black."""
        from diff_gaussian_rasterization.contrib import ErrorStats, l1_error_map
        from gaussian_renderer import render
        if len(cameras) != len(targets):
            raise ValueError(f"error_stats: {len(cameras)} cameras, {len(targets)} targets")
        if pipe is None:
            from gaussian_params import Pipe
            pipe = Pipe()
        if bg is None:
            bg = torch.zeros(3, device=self.device)
        views = range(len(cameras)) if views is None else [int(i) for i in views]
        stats = ErrorStats(self._xyz.shape[0], self.device)
        absgrad = getattr(pipe, "absgrad", False)            # (as contribution_stats: these frames have no backward)
        if absgrad:
            pipe.absgrad = False
        try:
            with torch.no_grad():
                for idx in views:
                    image = render(cameras[idx], self, pipe, bg)["render"]
                    if correct is not None:
                        image = correct(image, idx)
                    render(cameras[idx], self, pipe, bg, contributions=stats, pixel_error=l1_error_map(image, targets[idx]))
        finally:
            if absgrad:
                pipe.absgrad = absgrad
        return stats

    def densify_and_prune_by_score(self, scores, count, min_opacity, extent, max_screen_size):
        """densify_and_prune with a budget: the `count` Gaussians of the highest positive score are cloned (small) or split (large),
        then the prune runs as there.  Ties go to the lower index (a stable descending sort: deterministic); a score of 0 (or less) is
        never selected, so fewer than `count` may be."""
        P = self._xyz.shape[0]
        scores = torch.as_tensor(scores).reshape(-1)
        if scores.shape[0] != P:
            raise ValueError(f"densify_and_prune_by_score: {scores.shape[0]} scores for {P} Gaussians")
        scores = scores.to(self.device)
        scores = torch.where(scores > 0, scores, torch.zeros_like(scores))        # (a NaN would sort in front of every number)
        n = min(max(int(count), 0), int((scores > 0).sum()))
        hot = torch.zeros(P, dtype=torch.bool, device=self.device)
        hot[torch.sort(scores, stable=True, descending=True).indices[:n]] = True
        big = torch.max(self.get_scaling.detach(), dim=1).values > self.percent_dense * extent
        self._densify_hot_and_prune(hot, big, min_opacity, extent, max_screen_size)

    # ---- significance pruning (diff_gaussian_rasterization/contrib.py) ---------------------------------
    SIGNIFICANCE_SCORES = ("weight_sum", "weight_max", "volume_weighted")

    def contribution_stats(self, cameras, pipe=None, bg=None):
        """The blend statistics of this model over `cameras`: every camera rendered once under torch.no_grad() (render(...,
        contributions=)), the model's 3D filter applied as in any render.  pipe: default Pipe(); bg: default black."""
        from diff_gaussian_rasterization.contrib import ContributionStats
        from gaussian_renderer import render
        if pipe is None:
            from gaussian_params import Pipe
            pipe = Pipe()
        if bg is None:
            bg = torch.zeros(3, device=self.device)
        stats = ContributionStats(self._xyz.shape[0], self.device)
        absgrad = getattr(pipe, "absgrad", False)            # a training loop's switch: it asks something of the backward, and these
        if absgrad:                                          # frames have none
            pipe.absgrad = False
        try:
            with torch.no_grad():
                for cam in cameras:
                    render(cam, self, pipe, bg, contributions=stats)
        finally:
            if absgrad:
                pipe.absgrad = absgrad
        return stats

    def significance(self, stats, score="volume_weighted", v_pow=0.1):
        """float64 [P]: one score per Gaussian from a ContributionStats of this model.
        "weight_sum": the sum of its blend weights over all pixels of all frames (LightGaussian's global significance without the
        volume term; Mini-Splatting's importance).  "weight_max": its largest single blend weight (RadSplat).
        "volume_weighted": weight_sum * (V / V_ref) ** v_pow with V = prod(get_scaling, 1) and V_ref = sort(V, descending)[int(0.9 P)],
        the volume that 90 % of the Gaussians exceed (LightGaussian's rule; the ratio is not clipped).
        stats.count stays available for rules of the caller's own."""
        if score not in self.SIGNIFICANCE_SCORES:
            raise ValueError(f"significance: score = {score!r}: one of {', '.join(repr(n) for n in self.SIGNIFICANCE_SCORES)}")
        P = self._xyz.shape[0]
        if stats.P != P:
            raise ValueError(f"significance: the statistics hold {stats.P} Gaussians, the model {P}: collect them again after an edit")
        if score == "weight_max":
            return stats.weight_max.double()
        if score == "weight_sum" or P == 0:
            return stats.weight_sum
        V = torch.prod(self.get_scaling.detach().double(), dim=1)
        V_ref = torch.sort(V, descending=True).values[int(0.9 * P)]
        return stats.weight_sum * (V / V_ref) ** float(v_pow)

    def prune_by_significance(self, scores, fraction=None, threshold=None):
        """Remove the least significant Gaussians (prune_points: Adam moments and densification statistics follow their rows; a 3D
        filter goes stale as after any structural edit).  Exactly one of: fraction - the floor(fraction * P) lowest scores, ties to
        the lower index (a stable sort: deterministic); threshold - every score < threshold.  Returns the number of rows removed."""
        if (fraction is None) == (threshold is None):
            raise ValueError("prune_by_significance: exactly one of fraction and threshold")
        P = self._xyz.shape[0]
        scores = torch.as_tensor(scores).reshape(-1)
        if scores.shape[0] != P:
            raise ValueError(f"prune_by_significance: {scores.shape[0]} scores for {P} Gaussians")
        scores = scores.to(self.device)
        if threshold is not None:
            drop = scores < threshold
        else:
            if not 0.0 <= float(fraction) <= 1.0:
                raise ValueError(f"prune_by_significance: fraction = {fraction} outside [0, 1]")
            n = int(math.floor(float(fraction) * P))
            drop = torch.zeros(P, dtype=torch.bool, device=self.device)
            drop[torch.sort(scores, stable=True).indices[:n]] = True
        removed = int(drop.sum())
        if removed:
            self.prune_points(drop)
        return removed

    # ---- the MCMC strategy (diff_gaussian_rasterization/mcmc.py) ---------------------------------------
    MULTINOMIAL_MAX = 2 ** 24                                # torch.multinomial's limit on the number of categories

    def _mcmc_tensors(self):
        """(param, exp_avg, exp_avg_sq, role) of the five leaves; the moments as _rebuild finds them (None before the first step
        and without an optimizer)."""
        roles = {"opacity": "opacity", "scaling": "scaling"}
        out = []
        for name in TABLE:
            st = self.optimizer.state.get(self._t[name]) if self.optimizer is not None else None
            has = st is not None and "exp_avg" in st
            out.append((self._t[name], st["exp_avg"] if has else None, st["exp_avg_sq"] if has else None, roles.get(name, "copy")))
        return out

    def _mcmc_probs(self, rows=None):
        o = torch.sigmoid(self._opacity.detach()).reshape(-1)
        o = o if rows is None else o[rows]
        if o.shape[0] > self.MULTINOMIAL_MAX:
            raise ValueError(f"the MCMC strategy samples with torch.multinomial, which takes at most 2^24 categories: {o.shape[0]} Gaussians")
        return o

    def mcmc_relocate(self, min_opacity, generator=None, native=None):
        """Dead Gaussians (opacity <= min_opacity) become copies of live ones sampled by opacity; the sources take the relocation
        rule's opacity and scale and lose their Adam moments.  P does not change.  Returns the number relocated."""
        from diff_gaussian_rasterization import mcmc
        dead_mask = torch.sigmoid(self._opacity.detach()).reshape(-1) <= min_opacity
        dead, alive = torch.nonzero(dead_mask).reshape(-1), torch.nonzero(~dead_mask).reshape(-1)      # one host synchronisation
        if dead.numel() == 0 or alive.numel() == 0:
            return 0
        sampled = alive[torch.multinomial(self._mcmc_probs(alive), dead.numel(), replacement=True, generator=generator)]
        new_o, new_s = mcmc.compute_relocation(self._opacity, self._scaling, sampled, min_opacity, native=native)
        mcmc.relocate_rows(self._mcmc_tensors(), sampled, dead, new_o, new_s, native=native)
        self._acts.invalidate()
        return int(dead.numel())

    def mcmc_grow(self, cap_max, min_opacity, generator=None, native=None):
        """5 % more Gaussians, up to cap_max: copies of Gaussians sampled by opacity (all rows), sources and copies at the relocation
        rule's opacity and scale; the sources keep their moments, the copies start at zero.  Returns the number added."""
        from diff_gaussian_rasterization import mcmc
        P = self._xyz.shape[0]
        n_new = max(0, min(int(cap_max), int(1.05 * P)) - P)
        if n_new == 0:
            return 0
        sampled = torch.multinomial(self._mcmc_probs(), n_new, replacement=True, generator=generator)
        new_o, new_s = mcmc.compute_relocation(self._opacity, self._scaling, sampled, min_opacity, native=native)
        mcmc.relocate_rows([(p, None, None, role) for p, _, _, role in self._mcmc_tensors()], sampled, None, new_o, new_s, native=native)
        self._rebuild(extra={k: self._t[k].detach()[sampled] for k in TABLE})
        self._reset_stats()
        return n_new

    def mcmc_inject_noise(self, c, noise=None, native=None):
        """xyz += Sigma (noise g(opacity) c): covariance-shaped, opacity-gated position noise; noise = None draws randn_like(_xyz)."""
        from diff_gaussian_rasterization import mcmc
        if noise is None:
            noise = torch.randn_like(self._xyz)
        mcmc.inject_position_noise(self._xyz, self._scaling, self._rotation, self._opacity, noise, c, native=native)

    def mcmc_add_regularizer_grads(self, lambda_opacity, lambda_scale, native=None):
        """Adds the gradient of lambda_opacity mean(opacity) + lambda_scale mean(scale) to _opacity.grad and _scaling.grad (a missing
        .grad starts as zeros).  The loss value is not computed."""
        from diff_gaussian_rasterization import mcmc
        for t in (self._opacity, self._scaling):
            if t.grad is None:
                t.grad = torch.zeros_like(t)
        mcmc.add_regularizer_grads(self._opacity, self._scaling, lambda_opacity, lambda_scale, self._opacity.grad, self._scaling.grad,
                                   native=native)

    # ---- persistence -----------------------------------------------------------------------------------------
    # The checkpoint tuple is the reference's (scene/gaussian_model.py:67-99, saved by train.py as chkpnt*.pth), its optimizer
    # state_dict included: six groups with one tensor each (params 0..5 = xyz, f_dc, f_rest, opacity, scaling, rotation), every
    # group carrying torch.optim.Adam's own keys.  In memory f_dc and f_rest share one table; the two layouts are converted here,
    # at the boundary, so that checkpoints move both ways between this class and the reference's.
    def _optimizer_state_reference_layout(self):
        sd = self.optimizer.state_dict()
        defaults = {k: v for k, v in torch.optim.Adam([torch.zeros(1)], lr=0.0, eps=1e-15).param_groups[0].items() if k != "params"}
        groups, state, new_id = [], {}, 0
        for g in sd["param_groups"]:
            hyper = {**defaults, **{k: v for k, v in g.items() if k not in ("params", "head_cols", "tail")}}
            if g.get("name") == "f_rest":
                continue                                         # emitted together with "f_dc" below
            st = sd["state"].get(g["params"][0]) if g["params"] else None
            if g.get("name") == "f_dc":
                rest = next(x for x in sd["param_groups"] if x.get("name") == "f_rest")
                for hyp, cols in ((hyper, slice(0, 1)), ({**defaults, **{k: v for k, v in rest.items() if k != "params"}}, slice(1, None))):
                    groups.append({**hyp, "params": [new_id]})
                    if st is not None:
                        state[new_id] = {"step": st["step"].clone(), "exp_avg": st["exp_avg"][:, cols].contiguous(),      # (two tensors: own counters)
                                         "exp_avg_sq": st["exp_avg_sq"][:, cols].contiguous()}
                    new_id += 1
                continue
            groups.append({**hyper, "params": [new_id]})
            if st is not None:
                state[new_id] = st
            new_id += 1
        return {"state": state, "param_groups": groups}

    def _load_optimizer_state(self, sd):
        """Accepts the reference's six-tensor layout (what capture() emits, what the reference's own checkpoints hold) and this
        class's packed one (five tensors; checkpoints written by earlier versions of this package)."""
        groups = sd["param_groups"]
        mine = self.optimizer.state_dict()["param_groups"]
        if len(groups) == 6 and all(len(g["params"]) == 1 for g in groups):
            by_name = {g.get("name", GROUPS[i]): g for i, g in enumerate(groups)}
            state, new_groups = {}, []
            for tmpl in mine:
                src = by_name[tmpl["name"]]
                new_groups.append({**{k: v for k, v in src.items() if k != "params"}, **{k: tmpl[k] for k in ("head_cols", "tail") if k in tmpl},
                                   "params": list(tmpl["params"])})
                if not tmpl["params"]:
                    continue
                if tmpl["name"] == "f_dc":
                    dc, rest = sd["state"].get(by_name["f_dc"]["params"][0]), sd["state"].get(by_name["f_rest"]["params"][0])
                    if dc is not None:
                        cat = lambda k: dc[k] if rest is None or rest[k].numel() == 0 else torch.cat((dc[k], rest[k]), dim=1)
                        state[tmpl["params"][0]] = {"step": dc["step"], "exp_avg": cat("exp_avg"), "exp_avg_sq": cat("exp_avg_sq")}
                else:
                    st = sd["state"].get(src["params"][0])
                    if st is not None:
                        state[tmpl["params"][0]] = st
            sd = {"state": state, "param_groups": new_groups}
        self.optimizer.load_state_dict(sd)

    def capture(self):
        return (self.active_sh_degree, self._xyz, self._features_dc, self._features_rest, self._scaling, self._rotation,
                self._opacity, self.max_radii2D, self.xyz_gradient_accum, self.denom, self._optimizer_state_reference_layout(),
                self.spatial_lr_scale)

    def restore(self, model_args, training_args):
        (self.active_sh_degree, xyz, fdc, frest, scaling, rotation, opacity, max_radii, accum, denom, opt_state,
         self.spatial_lr_scale) = model_args
        self._adopt(dict(xyz=xyz, f_dc=fdc, f_rest=frest, scaling=scaling, rotation=rotation, opacity=opacity))
        self.max_radii2D = max_radii
        self.training_setup(training_args)
        self.xyz_gradient_accum, self.denom = accum, denom
        self._load_optimizer_state(opt_state)

    def extract_mesh(self, cameras, pipe, background, **kw):
        """The triangle mesh of the surface `cameras` see: depth maps fused into a TSDF volume, surface nets (scene/mesh.py extract_mesh,
        which takes kw: voxel_size, sdf_trunc, bounds, depth_max, min_weight, depth_ratio (0: the expected depth is fused; 1: the median depth),
        sparse (False; True: a brick-allocated volume), resolution (voxels along the longest side: 512, and 1024 when sparse), two_pass,
        and min_component_faces, keep_largest to clean it) -> (vertices [V,3], faces [F,3] int32, colors [V,3])."""
        from . import mesh
        return mesh.extract_mesh(self, cameras, pipe, background, **kw)

    def save_ply(self, path, fuse_filter=False):
        """Without a 3D filter: the reference's file.  With one: Mip-Splatting's layout, one more property `filter_3D` after rot_3;
        fuse_filter=True (its save_fused_ply): the filtered logits and log-scales in the opacity and scale columns and no filter
        column, the file any viewer shows as the filtered model."""
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        n = lambda t: t.detach().cpu().numpy()
        opacity, scaling, filter_3D = self._opacity, self._scaling, self.checked_filter_3D()
        if filter_3D is not None and fuse_filter:
            from diff_gaussian_rasterization.filter3d import apply_filter_3d
            with torch.no_grad():
                opacity, scaling = apply_filter_3d(opacity, scaling, filter_3D, raw=True)
            filter_3D = None
        ply_io.write_gaussian_ply(path, n(self._xyz), n(self._features_dc), n(self._features_rest), n(opacity),
                                  n(scaling), n(self._rotation), filter_3D=None if filter_3D is None else n(filter_3D))

    def load_ply(self, path, device="cuda"):
        d = ply_io.read_gaussian_ply(path)
        assert d["f_rest"].shape[1] == (self.max_sh_degree + 1) ** 2 - 1, "PLY SH degree does not match the model"
        t = lambda a: torch.tensor(a, dtype=torch.float32, device=device)
        self._adopt(dict(xyz=t(d["xyz"]), f_dc=t(d["f_dc"]), f_rest=t(d["f_rest"]), opacity=t(d["opacity"]),
                         scaling=t(d["scaling"]), rotation=t(d["rotation"])))
        if "filter_3D" in d:
            self.filter_3D = t(d["filter_3D"])
        self.active_sh_degree = self.max_sh_degree

    def save_compressed(self, path, **kw):
        """The vector-quantised checkpoint (scene/compression.py; kw: sh_clusters, iters, generator)."""
        if self.filter_3D is not None:
            raise ValueError("save_compressed: the archive does not store a 3D filter; save_ply(path, fuse_filter=True) writes the "
                             "filtered model, or set filter_3D = None to compress the unfiltered parameters")
        from . import compression
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        compression.save_compressed(path, compression.compress(self, **kw))

    def load_compressed(self, path, device="cuda"):
        from . import compression
        d = compression.load_compressed(path)
        assert int(d["sh_degree"]) == self.max_sh_degree, "the checkpoint's SH degree does not match the model"
        self._adopt({k: v.to(device) for k, v in compression.decompress(d).items()})
        self.active_sh_degree = self.max_sh_degree
