"""render(): host-side mirror of the reference's only caller of the rasterizer
(gaussian_renderer/__init__.py:18-100).  Same arguments, same returned dict, same optional-input
selection (`pipe.compute_cov3D_python`, `pipe.convert_SHs_python`, `override_color`); `pc` is anything
with the reference GaussianModel's getters (get_xyz, get_opacity, get_scaling, get_rotation,
get_features, get_covariance, active_sh_degree, max_sh_degree).

Extension: `pipe.fused_activations` (not a reference flag).  True: render from the model's raw parameters
`_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation` with the activations fused into the HIP kernels
(GaussianRasterizer.forward_raw) — same image, same gradients on the parameters, without the ~30 torch kernels of the getters
and their backward.  Unset (None, the default): that path for this package's scene.GaussianModel (whose SH coefficients are
one interleaved leaf `_features`: raw mode 2), the getters for any other store.  False: always the getters.

`pipe.antialiasing` (upstream's flag; absent or False: off) turns on the rasterizer's opacity compensation for the 0.3 px^2
dilation (diff_gaussian_rasterization.antialias), on the fused path and the getter path alike.

A model whose `filter_3D` is not None (scene.GaussianModel.compute_3D_filter, Mip-Splatting's 3D smoothing filter) is rendered with
its filtered opacities and scales (diff_gaussian_rasterization.filter3d), on both paths; a filter whose row count is not the model's
is a ValueError.

`pipe.absgrad` (gsplat's flag; absent or False: off): after backward() the returned `viewspace_points` also carries `.absgrad`
[P,3], the per-pixel absolute sums of the means2D gradient (diff_gaussian_rasterization, "absgrad"), on both paths; not together
with depth_alpha=True (ValueError).

`contributions` (a diff_gaussian_rasterization.contrib.ContributionStats; None: off): the frame's per-Gaussian blend statistics are
added into it, under torch.no_grad() (a statistics frame has no backward).  Such a frame always goes through the model's getters,
whatever `pipe.fused_activations` says: fusing the activations into the kernels saves the getters' backward, which a statistics
frame does not have, and the two paths round the activations differently in the last bit - so the statistics are the model's and
the camera's, the same bits under either setting of that switch (the image is the one the getter path renders).  The rasterizer
itself takes `contributions` on forward and forward_raw alike.  Not together with depth_alpha=True or pipe.absgrad (ValueError).

`pixel_error` (float32 [H,W] or [1,H,W]; None: off; with a contrib.ErrorStats as `contributions`): the frame also adds every
Gaussian's error-weighted blend total into the ErrorStats and folds it (diff_gaussian_rasterization, "pixel_error"); passed through.

render_normals() (extension) is a frame of its own for the normal-consistency term (diff_gaussian_rasterization.normals): the
Gaussians' view-space normals as precomputed colours, with the depth and alpha maps and the normal map the depth implies.  render()
neither gains nor loses anything by it.

`extra_colors` (extension; with depth_alpha=True; [P,3] float32): three more per-Gaussian values blended inside the colour frame with
the colour's own weights (diff_gaussian_rasterization, "extra_colors"): the dict also holds "extra" [3,H,W], differentiable, on both
paths.  render_with_normals() is the one-frame form of render() + render_normals(): the colour frame carries the Gaussians' view-space
normals as its extra colours, so the four maps of the normal-consistency term come from one frame instead of two.

`median_depth=True` (extension; with depth_alpha=True): the dict also holds "median_depth" [1,H,W], per pixel the depth of the splat at
which the accumulated opacity crosses one half (diff_gaussian_rasterization, "median_depth"), differentiable in that splat's depth, on
both paths.  render_normals(depth_ratio=r) mixes it into the depth the normals are taken from (normals.surface_depth; 2DGS uses r = 1
for bounded scenes, 0 - the default, the expected depth alone - for unbounded ones); not with extra_colors, so render_with_normals()
refuses a non-zero depth_ratio.

render_with_distortion() (extension) is the colour frame with the depth moments (m, m^2, 0) of its own means3D as extra colours, for
the depth-distortion term (diff_gaussian_rasterization.distortion): render()'s dict plus "depth", "alpha", "extra" and "distortion".
"""
import math

import torch

from diff_gaussian_rasterization import GaussianRasterizationSettings, GaussianRasterizer

_C0 = 0.28209479177387814
_C1 = 0.4886025119029199
_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
_C3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
       1.445305721320277, -0.5900435899266435)


def eval_sh(deg: int, sh: torch.Tensor, dirs: torch.Tensor) -> torch.Tensor:
    """SH colour in torch for the `convert_SHs_python` branch; sh [..., C, K], dirs [..., 3]
    (same basis as utils/sh_utils.py:57-112; pinned by tests/golden/sh_eval.npz)."""
    assert 0 <= deg <= 3
    res = _C0 * sh[..., 0]
    if deg > 0:
        x, y, z = dirs[..., 0:1], dirs[..., 1:2], dirs[..., 2:3]
        res = res - _C1 * y * sh[..., 1] + _C1 * z * sh[..., 2] - _C1 * x * sh[..., 3]
        if deg > 1:
            xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
            res = (res + _C2[0] * xy * sh[..., 4] + _C2[1] * yz * sh[..., 5] + _C2[2] * (2.0 * zz - xx - yy) * sh[..., 6]
                   + _C2[3] * xz * sh[..., 7] + _C2[4] * (xx - yy) * sh[..., 8])
            if deg > 2:
                res = (res + _C3[0] * y * (3 * xx - yy) * sh[..., 9] + _C3[1] * xy * z * sh[..., 10]
                       + _C3[2] * y * (4 * zz - xx - yy) * sh[..., 11] + _C3[3] * z * (2 * zz - 3 * xx - 3 * yy) * sh[..., 12]
                       + _C3[4] * x * (4 * zz - xx - yy) * sh[..., 13] + _C3[5] * z * (xx - yy) * sh[..., 14]
                       + _C3[6] * x * (xx - 3 * yy) * sh[..., 15])
    return res


_ZERO_POINTS = {}
_ZERO_BG = {}


def render_normals(viewpoint_camera, pc, pipe, scaling_modifier=1.0, depth_ratio=0.0):
    """The maps of the normal-consistency term (extension; diff_gaussian_rasterization.normals), one frame: the Gaussians' view-space
    normals (the shortest axis, turned to the camera) rendered as precomputed colours over a zero background with depth_alpha=True.
    -> {"normal" [3,H,W] (alpha-weighted, not normalised), "depth", "alpha" [1,H,W], "depth_normal" [3,H,W] (depth_to_normal of the two),
    "viewspace_points", "radii", "visibility_filter"}.  The model's getters are used; a model with a 3D filter renders its filtered
    scales, as render() does, and the same scales choose the axis.  pipe.absgrad raises (depth_alpha=True refuses it).
    depth_ratio (2DGS's; in [0, 1]; 0: the calls made without it): above 0 the frame also renders the median depth, "depth_normal" is
    taken from surface_depth(depth, alpha, median, depth_ratio) - whose z = D / alpha is (1 - r) mean + r median - and the dict also
    holds "median_depth" and "surf_depth" [1,H,W]."""
    from diff_gaussian_rasterization.normals import depth_to_normal, gaussian_normals, surface_depth
    depth_ratio = float(depth_ratio)
    if not 0.0 <= depth_ratio <= 1.0:
        raise ValueError(f"render_normals: depth_ratio {depth_ratio} outside [0, 1]")
    if getattr(pipe, "absgrad", False):
        raise ValueError("render_normals: the frame is rendered with depth_alpha=True, which pipe.absgrad is not supported with (the abs "
                         "blend backward does not carry the depth and alpha gradients): turn pipe.absgrad off for this frame")
    filtered = getattr(pc, "filter_3D", None) is not None
    xyz = pc.get_xyz
    normals = gaussian_normals(pc.get_scaling_with_3D_filter if filtered else pc.get_scaling, pc.get_rotation, xyz,
                               viewpoint_camera.world_view_transform, viewpoint_camera.camera_center)
    key = (xyz.device.type, xyz.device.index)
    bg = _ZERO_BG.get(key)
    if bg is None:
        bg = _ZERO_BG[key] = torch.zeros(3, dtype=torch.float32, device=xyz.device)
    if depth_ratio > 0.0:
        pkg = render(viewpoint_camera, pc, pipe, bg, scaling_modifier, override_color=normals, depth_alpha=True, median_depth=True)
        surf = surface_depth(pkg["depth"], pkg["alpha"], pkg["median_depth"], depth_ratio)
        depth_normal = depth_to_normal(surf, pkg["alpha"], math.tan(viewpoint_camera.FoVx * 0.5), math.tan(viewpoint_camera.FoVy * 0.5))
        return {"normal": pkg["render"], "depth": pkg["depth"], "alpha": pkg["alpha"], "depth_normal": depth_normal,
                "median_depth": pkg["median_depth"], "surf_depth": surf,
                "viewspace_points": pkg["viewspace_points"], "radii": pkg["radii"], "visibility_filter": pkg["visibility_filter"]}
    pkg = render(viewpoint_camera, pc, pipe, bg, scaling_modifier, override_color=normals, depth_alpha=True)
    depth_normal = depth_to_normal(pkg["depth"], pkg["alpha"], math.tan(viewpoint_camera.FoVx * 0.5), math.tan(viewpoint_camera.FoVy * 0.5))
    return {"normal": pkg["render"], "depth": pkg["depth"], "alpha": pkg["alpha"], "depth_normal": depth_normal,
            "viewspace_points": pkg["viewspace_points"], "radii": pkg["radii"], "visibility_filter": pkg["visibility_filter"]}


def render_with_normals(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, depth_ratio=0.0):
    """render() and the maps of render_normals() from ONE frame (extension): the colour frame, on whichever of the raw and getter
    paths render() would take, with depth_alpha=True and the Gaussians' view-space normals as its extra colours.  The normals are
    computed from the very scales and rotations that frame is rendered from (raw log-scales and quaternions on the raw path:
    gaussian_normals takes either), a model's 3D filter included.
    -> render()'s dict (with "depth", "alpha" and "extra") plus "normal" [3,H,W] (= "extra": alpha-weighted, not normalised) and
    "depth_normal" [3,H,W] (depth_to_normal of the depth and alpha maps).  "render" is render()'s, bit for bit; on the getter path
    "normal", "depth" and "alpha" are render_normals()'s, bit for bit.  pipe.absgrad and pipe.compute_cov3D_python raise ValueError,
    and so does a non-zero depth_ratio: the frame carries extra colours, and the ext x median blend kernels are not built (use
    render() + render_normals(depth_ratio=...))."""
    from diff_gaussian_rasterization.normals import depth_to_normal, gaussian_normals
    if float(depth_ratio) != 0.0:
        raise ValueError("render_with_normals: depth_ratio must be 0: the one-frame form carries the normals as extra colours, and the "
                         "median depth is not rendered together with extra colours (the ext x median blend kernels are not built); "
                         "use render() and render_normals(depth_ratio=...)")
    if getattr(pipe, "absgrad", False):
        raise ValueError("render_with_normals: the frame is rendered with depth_alpha=True, which pipe.absgrad is not supported with: "
                         "turn pipe.absgrad off for this frame")
    if pipe.compute_cov3D_python:
        raise ValueError("render_with_normals: the normals are the shortest axes of the scales and rotations the frame is rendered "
                         "from; pipe.compute_cov3D_python renders from precomputed covariances")

    def normals(scales, rotations):
        return gaussian_normals(scales, rotations, pc.get_xyz, viewpoint_camera.world_view_transform, viewpoint_camera.camera_center)

    pkg = _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, None, True, None, None, extra_colors=normals)
    pkg["normal"] = pkg["extra"]
    pkg["depth_normal"] = depth_to_normal(pkg["depth"], pkg["alpha"], math.tan(viewpoint_camera.FoVx * 0.5),
                                          math.tan(viewpoint_camera.FoVy * 0.5))
    return pkg


def render_with_distortion(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, near=0.2, far=100.0, mapping="ndc",
                           with_map=True):
    """render() and the maps of the depth-distortion term from ONE frame (extension; diff_gaussian_rasterization.distortion, DESIGN
    section 29): the colour frame, on whichever of the raw and getter paths render() would take, with depth_alpha=True and
    depth_moments(means3D, world_view_transform, near, far, mapping) - of the very means3D the frame renders - as its extra colours.
    -> render()'s dict (with "depth", "alpha" and "extra" = the moments map (M1, M2, 0)) plus "distortion" [1,H,W], distortion_map of
    the two.  "render" and "radii" are render()'s, bit for bit.  A model's 3D filter, pipe.antialiasing and a LatentGaussianModel
    compose as they do with render().  pipe.absgrad raises ValueError (the frame carries depth and alpha, which the abs blend backward
    does not).  A training loop takes distortion_loss(pkg["extra"], pkg["alpha"]) instead of the map's mean, which never stores the map;
    with_map=False leaves "distortion" out of the dict and its launch out of the frame."""
    from diff_gaussian_rasterization.distortion import depth_moments, distortion_map
    if getattr(pipe, "absgrad", False):
        raise ValueError("render_with_distortion: the frame is rendered with depth_alpha=True, which pipe.absgrad is not supported with "
                         "(the abs blend backward does not carry the depth and alpha gradients): turn pipe.absgrad off for this frame")

    def moments(scales, rotations):
        return depth_moments(pc.get_xyz, viewpoint_camera.world_view_transform, near, far, mapping)

    pkg = _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, None, True, None, None, extra_colors=moments)
    if with_map:
        pkg["distortion"] = distortion_map(pkg["extra"], pkg["alpha"])
    return pkg


def _zero_points(like: torch.Tensor) -> torch.Tensor:
    """One block of zeros shaped like `like` per device (re-made when the model's size or dtype changes)."""
    key = (like.device.type, like.device.index)
    z = _ZERO_POINTS.get(key)
    if z is None or z.shape != like.shape or z.dtype != like.dtype:
        z = _ZERO_POINTS[key] = torch.zeros_like(like, requires_grad=False)
    return z


def render(viewpoint_camera, pc, pipe, bg_color: torch.Tensor, scaling_modifier=1.0, override_color=None, depth_alpha=False,
           contributions=None, pixel_error=None, extra_colors=None, median_depth=False):
    """Render the scene.  Background tensor (bg_color) must be on the GPU.
    depth_alpha=True (extension): the dict also holds "depth" and "alpha" [1,H,W], differentiable (diff_gaussian_rasterization).
    contributions (extension): a ContributionStats the frame's blend statistics are added into; rendered under torch.no_grad(),
    through the getters whatever pipe.fused_activations says (module docstring).
    pixel_error (extension; with an ErrorStats as contributions): the error map of this view, passed to the rasterizer.
    extra_colors (extension; with depth_alpha=True): [P,3] float32 blended in the same frame; the dict also holds "extra" [3,H,W].
    median_depth=True (extension; with depth_alpha=True; not with extra_colors, contributions or pipe.absgrad): the dict also holds
    "median_depth" [1,H,W], differentiable in the median splat's depth."""
    if median_depth:
        from diff_gaussian_rasterization import check_median_depth
        check_median_depth(depth_alpha, getattr(pipe, "absgrad", False), contributions, extra_colors=extra_colors)
        return _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, depth_alpha, None, pixel_error,
                       median_depth=True)
    if extra_colors is not None:
        return _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, depth_alpha, contributions, pixel_error,
                       extra_colors=extra_colors)
    if contributions is not None:
        with torch.no_grad():
            return _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, depth_alpha, contributions, pixel_error)
    return _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, depth_alpha, None, pixel_error)


def _render(viewpoint_camera, pc, pipe, bg_color, scaling_modifier, override_color, depth_alpha, contributions, pixel_error=None,
            extra_colors=None, median_depth=False):
    # extra_colors: a tensor, or (render_with_normals) a function of the (scales, rotations) the frame is rendered from
    xyz = pc.get_xyz
    # (the reference builds this as zeros_like(...) + 0 and retain_grad()s the non-leaf result; a leaf with requires_grad keeps
    # its .grad by itself.  Its VALUES are never read, by the rasterizer or by the training loop, only its .grad: every frame
    # gets a fresh leaf over one shared block of zeros per device instead of a 12 P-byte fill of its own)
    screenspace_points = _zero_points(xyz).detach().requires_grad_(True)

    raster_settings = GaussianRasterizationSettings(
        image_height=int(viewpoint_camera.image_height), image_width=int(viewpoint_camera.image_width),
        tanfovx=math.tan(viewpoint_camera.FoVx * 0.5), tanfovy=math.tan(viewpoint_camera.FoVy * 0.5),
        bg=bg_color, scale_modifier=scaling_modifier, viewmatrix=viewpoint_camera.world_view_transform,
        projmatrix=viewpoint_camera.full_proj_transform, sh_degree=pc.active_sh_degree,
        campos=viewpoint_camera.camera_center, prefiltered=False, debug=pipe.debug)
    rasterizer = GaussianRasterizer(raster_settings=raster_settings, depth_alpha=depth_alpha,
                                    antialiasing=getattr(pipe, "antialiasing", False), absgrad=getattr(pipe, "absgrad", False),
                                    contributions=contributions, pixel_error=pixel_error, median_depth=median_depth)

    def result(out):
        d = {"render": out[0], "viewspace_points": screenspace_points, "visibility_filter": out[1] > 0, "radii": out[1]}
        if depth_alpha:
            d["depth"], d["alpha"] = out[2], out[3]
        if extra_colors is not None:
            d["extra"] = out[4]
        if median_depth:
            d["median_depth"] = out[4]
        return d

    def extra_kw(scales, rotations):
        """The rasterizer call's extra_colors keyword; nothing without one: the call as it was."""
        if extra_colors is None:
            return {}
        return {"extra_colors": extra_colors(scales, rotations) if callable(extra_colors) else extra_colors}

    # the fused path hands the RAW parameters to the kernels and so bypasses the getters — and with them the reference's
    # freeze flags (scene/gaussian_model.py:104-125 detach() the getter's result): a model with any of them set takes the
    # plain path, where a frozen parameter receives no gradient
    frozen = any(getattr(pc, f, False) for f in ("freeze_means", "freeze_scales", "freeze_rotations", "freeze_opacities"))
    packed = bool(getattr(pc, "packed_features", False))          # scene.GaussianModel: get_features is ONE interleaved leaf [P,M,3]
    fused = getattr(pipe, "fused_activations", None)
    if fused is None:            # not set: this package's own model renders from its raw leaves, any other store through its getters
        fused = packed
    if contributions is not None:      # one path for every statistics frame: the statistics do not depend on a performance switch
        fused = False
    # the 3D smoothing filter (scene.GaussianModel.compute_3D_filter): a per-Gaussian op in front of the rasterizer, independent of
    # the camera being rendered.  None: no launch, the frame is what it was.  A stale filter raises here (checked_filter_3D)
    if hasattr(pc, "checked_filter_3D"):
        filter_3D = pc.checked_filter_3D()
    else:                        # another store with the attribute: the same rule
        filter_3D = getattr(pc, "filter_3D", None)
        if filter_3D is not None and filter_3D.shape[0] != xyz.shape[0]:
            raise ValueError(f"filter_3D has {filter_3D.shape[0]} rows for {xyz.shape[0]} Gaussians: call compute_3D_filter(cameras)")
    if (fused and override_color is None and not pipe.compute_cov3D_python and not pipe.convert_SHs_python and not frozen
            and (packed or hasattr(pc, "_features_rest"))):
        opacity, scaling = pc._opacity, pc._scaling
        if filter_3D is not None:
            from diff_gaussian_rasterization.filter3d import apply_filter_3d
            opacity, scaling = apply_filter_3d(opacity, scaling, filter_3D, raw=True)
        if packed:               # exp / normalize / sigmoid inside the kernels, the SH table as it is: no getter runs at all
            return result(rasterizer.forward_raw(pc._xyz, screenspace_points, pc._features, None,
                                                 opacity, scaling, pc._rotation, **extra_kw(scaling, pc._rotation)))
        return result(rasterizer.forward_raw(pc._xyz, screenspace_points, pc._features_dc, pc._features_rest,
                                             opacity, scaling, pc._rotation, **extra_kw(scaling, pc._rotation)))

    filtered = filter_3D is not None
    scales = rotations = cov3D_precomp = None
    if pipe.compute_cov3D_python:
        cov3D_precomp = pc.get_covariance(scaling_modifier)              # (the model's own: filtered scales when it has a filter)
    else:
        scales, rotations = (pc.get_scaling_with_3D_filter if filtered else pc.get_scaling), pc.get_rotation

    shs = colors_precomp = None
    if override_color is None:
        if pipe.convert_SHs_python:
            feats = pc.get_features
            shs_view = feats.transpose(1, 2).view(-1, 3, (int(pc.max_sh_degree) + 1) ** 2)
            dir_pp = xyz - viewpoint_camera.camera_center.repeat(feats.shape[0], 1)
            dir_pp = dir_pp / dir_pp.norm(dim=1, keepdim=True)
            colors_precomp = torch.clamp_min(eval_sh(int(pc.active_sh_degree), shs_view, dir_pp) + 0.5, 0.0)
        else:
            shs = pc.get_features
    else:
        colors_precomp = override_color

    return result(rasterizer(means3D=xyz, means2D=screenspace_points, shs=shs, colors_precomp=colors_precomp,
                             opacities=pc.get_opacity_with_3D_filter if filtered else pc.get_opacity, scales=scales, rotations=rotations,
                             cov3D_precomp=cov3D_precomp, **extra_kw(scales, rotations)))
