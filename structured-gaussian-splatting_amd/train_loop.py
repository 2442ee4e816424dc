"""The reference's training iteration (train.py:63-146) around the drop-in rasterizer, for synthetic scenes:
LR schedule, SH-degree ramp, render -> L1/D-SSIM -> backward, densification bookkeeping, densify/prune,
opacity reset, Adam step.  SURVEY 8f row f1.  opt.densify_strategy = "mcmc" replaces the densification part:
regulariser gradients before the step; relocation and growth after it, inside the refinement window; position noise every iteration.
opt.bilateral_grid puts the per-image bilateral grid between render() and the loss; off, the loop is as before.
opt.filter_3d keeps the model's 3D smoothing filter current: computed from `cameras` before the first render, after
every edit that changes or moves the Gaussians, and every 100 iterations after densification; off, the loop is as before.
opt.significance_prune_iterations lists iterations at which the model is pruned by significance: behind the
optimizer step, the blend statistics of all `cameras` are collected and the least significant fraction removed; empty (the default),
the loop is as before.
opt.densify_error_views > 0 replaces the refinement's criterion: at a refinement iteration that many cameras are
drawn, the model's error-weighted blend statistics are taken over them (GaussianModel.error_stats; with opt.bilateral_grid the image is
corrected by the camera's grid first), and the ceil(opt.densify_error_growth * P) Gaussians responsible for the most image error
(opt.densify_error_score: "max" over the views, or "sum") are cloned or split in place of those over the gradient threshold; the
prune is unchanged.  0 (the default): the loop is as before.  The defaults of the two numbers are not tuned on captured scenes.
opt.lambda_normal > 0 adds the normal-consistency loss from iteration opt.normal_from_iter on: one
gaussian_renderer.render_normals frame of the same camera beside the colour frame, opt.lambda_normal * normal_consistency_loss(...)
added to the loss in front of backward(); on_iteration still receives the image loss alone.  It composes with every strategy above (the
normals frame is rendered without pipe.absgrad).  0 (the default): the loop is as before.  Neither number is tuned on captured scenes.
opt.normal_in_frame (with lambda_normal > 0) takes the colour image and the three maps from ONE gaussian_renderer.render_with_normals
frame per iteration from normal_from_iter on instead of two frames; the densification statistics then see the normal
term's means2D gradient too.  Not with opt.densify_absgrad (the frame carries depth and alpha).  False (the default): the loop is as before.
opt.depth_ratio (2DGS's, in [0, 1]; with lambda_normal > 0) is handed to render_normals: above 0 the normal term's depth normals are
taken from the mix (1 - r) mean + r median depth (2DGS uses 1 for bounded scenes), and the loss is formed on that
depth.  Not with normal_in_frame (the one frame carries extra colours).  0 (the default): the loop is as before.  Untuned.
opt.lambda_dist > 0 adds the depth-distortion loss from iteration opt.dist_from_iter on: the colour frame itself
comes from gaussian_renderer.render_with_distortion (one frame, no second render), and opt.lambda_dist * distortion_loss(pkg["extra"],
pkg["alpha"]) joins the loss in front of backward(); on_iteration still receives the image loss alone.  The densification statistics
then see the distortion term's means2D gradient too, as 2DGS's do.  It composes with the two-frame normal term and every strategy
above.  Not with normal_in_frame (the frame's one extra triple is taken by the normals, and a fourth extra channel is not built), not
with opt.densify_absgrad (the frame carries depth and alpha), not with a ShardedRenderer.  0 (the default): the loop is as before.
Neither number is tuned on captured scenes."""
import math
import random

import torch

from fused_adam import FusedAdam, SparseFusedAdam
from gaussian_renderer import render
from loss_utils import training_loss


def train(gaussians, cameras, targets, opt, pipe, background, iterations, first_iter=1, scene_extent=5.0,
          white_background=False, on_iteration=None, bilagrid=None):
    """cameras / targets: lists of equal length (Camera-like objects and [3,H,W] ground-truth images).
    opt.bilateral_grid: every camera owns a bilateral grid (`bilagrid`, or a new BilateralGrid of opt.bilateral_grid_shape on the
    model's device, kept as gaussians.bilagrid); the rendered image goes through its grid before the loss, the grids' total variation
    joins the loss with weight opt.bilateral_grid_tv, and the grids step with an Adam of their own.  render() and evaluation are
    untouched: correcting test views is the caller's business."""
    stack = []
    use_bilagrid = bool(getattr(opt, "bilateral_grid", False))
    if use_bilagrid:
        from diff_gaussian_rasterization.bilagrid import BilateralGrid, bilateral_grid_lr, total_variation_loss
        if bilagrid is None:
            bilagrid = BilateralGrid(len(cameras), *opt.bilateral_grid_shape).to(gaussians.get_xyz.device)
        if bilagrid.grids.shape[0] != len(cameras):
            raise ValueError(f"train: {bilagrid.grids.shape[0]} bilateral grids for {len(cameras)} cameras")
        gaussians.bilagrid = bilagrid
        bilagrid_optimizer = FusedAdam([bilagrid.grids], lr=opt.bilateral_grid_lr, eps=1e-15, native=bilagrid.grids.is_cuda)
    mcmc = getattr(opt, "densify_strategy", "default") == "mcmc"
    filter_3d = bool(getattr(opt, "filter_3d", False))
    prune_at = tuple(int(i) for i in getattr(opt, "significance_prune_iterations", ()))
    if prune_at and mcmc:
        raise ValueError("significance_prune_iterations with densify_strategy = \"mcmc\": the MCMC strategy keeps its tables at a fixed "
                         "size (relocation and growth to a cap), pruning by significance shrinks them")
    error_views = int(getattr(opt, "densify_error_views", 0))
    if error_views > 0:
        if mcmc:
            raise ValueError("densify_error_views with densify_strategy = \"mcmc\": the MCMC strategy has its own relocation and growth rule")
        if getattr(opt, "densify_absgrad", False):
            raise ValueError("densify_error_views with densify_absgrad: the error score replaces the gradient criterion that absgrad feeds")
        if opt.densify_error_score not in gaussians.DENSIFY_ERROR_SCORES:
            raise ValueError(f"densify_error_score = {opt.densify_error_score!r}: one of "
                             f"{', '.join(repr(n) for n in gaussians.DENSIFY_ERROR_SCORES)}")
    lambda_normal = float(getattr(opt, "lambda_normal", 0.0))
    if lambda_normal < 0:
        raise ValueError(f"lambda_normal = {lambda_normal}: a weight of at least 0 expected")
    if lambda_normal > 0:
        from diff_gaussian_rasterization.normals import normal_consistency_loss
        from gaussian_renderer import render_normals
    normal_in_frame = lambda_normal > 0 and bool(getattr(opt, "normal_in_frame", False))
    depth_ratio = float(getattr(opt, "depth_ratio", 0.0)) if lambda_normal > 0 else 0.0
    if not 0.0 <= depth_ratio <= 1.0:
        raise ValueError(f"depth_ratio = {depth_ratio}: a value in [0, 1] expected")
    if normal_in_frame and depth_ratio > 0:
        raise ValueError("normal_in_frame with depth_ratio > 0: the one frame carries the normals as extra colours, and the median depth "
                         "is not rendered together with extra colours (use the two-frame path: normal_in_frame = False)")
    if normal_in_frame:
        from gaussian_renderer import render_with_normals
        if getattr(opt, "densify_absgrad", False):
            raise ValueError("normal_in_frame with densify_absgrad: the one frame carries the depth and alpha maps, which the abs blend "
                             "backward does not (use the two-frame path: normal_in_frame = False)")
    lambda_dist = float(getattr(opt, "lambda_dist", 0.0))
    if lambda_dist < 0:
        raise ValueError(f"lambda_dist = {lambda_dist}: a weight of at least 0 expected")
    if lambda_dist > 0:
        from diff_gaussian_rasterization.distortion import distortion_loss
        from gaussian_renderer import render_with_distortion
        if normal_in_frame:
            raise ValueError("lambda_dist with normal_in_frame: the colour frame carries one extra triple, which the normals take, and a "
                             "blend with a fourth extra channel is not built (use the two-frame normal term: normal_in_frame = False)")
        if getattr(opt, "densify_absgrad", False):
            raise ValueError("lambda_dist with densify_absgrad: the distortion term's frame carries the depth and alpha maps, which the "
                             "abs blend backward does not")
    if filter_3d:
        gaussians.compute_3D_filter(cameras)
    for it in range(first_iter, iterations + 1):
        xyz_lr = gaussians.update_learning_rate(it)
        if it % 1000 == 0:
            gaussians.oneupSHdegree()
        if not stack:
            stack = list(range(len(cameras)))
        idx = stack.pop(random.randint(0, len(stack) - 1))
        bg = torch.rand(3, device=background.device) if opt.random_background else background
        if getattr(opt, "densify_absgrad", False):             # the abs blend backward costs a little: only while its statistics are read
            pipe.absgrad = it < opt.densify_until_iter
        in_frame = normal_in_frame and it >= opt.normal_from_iter
        with_dist = lambda_dist > 0 and it >= opt.dist_from_iter
        if with_dist:
            pkg = render_with_distortion(cameras[idx], gaussians, pipe, bg, with_map=False)
        else:
            pkg = render_with_normals(cameras[idx], gaussians, pipe, bg) if in_frame else render(cameras[idx], gaussians, pipe, bg)
        image, vsp, vis, radii = pkg["render"], pkg["viewspace_points"], pkg["visibility_filter"], pkg["radii"]
        if use_bilagrid:
            image = bilagrid(image, idx)
        loss = training_loss(image, targets[idx], opt.lambda_dssim)
        if use_bilagrid:
            loss = loss + opt.bilateral_grid_tv * total_variation_loss(bilagrid.grids)
        image_loss = loss                                          # what on_iteration receives
        if with_dist:
            loss = loss + lambda_dist * distortion_loss(pkg["extra"], pkg["alpha"])
        if in_frame:
            cam = cameras[idx]
            normal_loss = normal_consistency_loss(pkg["normal"], pkg["depth"], pkg["alpha"], math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
            (loss + lambda_normal * normal_loss).backward()
        elif lambda_normal > 0 and it >= opt.normal_from_iter:
            cam, absgrad = cameras[idx], getattr(pipe, "absgrad", False)
            if absgrad:                                            # the normals frame carries depth and alpha: rendered without it
                pipe.absgrad = False
            maps = render_normals(cam, gaussians, pipe, depth_ratio=depth_ratio) if depth_ratio > 0 else render_normals(cam, gaussians, pipe)
            if absgrad:
                pipe.absgrad = absgrad
            normal_loss = normal_consistency_loss(maps["normal"], maps["surf_depth" if depth_ratio > 0 else "depth"], maps["alpha"], math.tan(cam.FoVx * 0.5), math.tan(cam.FoVy * 0.5))
            (loss + lambda_normal * normal_loss).backward()
        else:
            loss.backward()
        with torch.no_grad():
            if mcmc:
                gaussians.mcmc_add_regularizer_grads(opt.mcmc_opacity_reg, opt.mcmc_scale_reg)
            elif it < opt.densify_until_iter:
                gaussians.update_densification_stats(vsp, radii)       # train.py:127-130, one native pass
                if it > opt.densify_from_iter and it % opt.densification_interval == 0:
                    size_threshold = 20 if it > opt.opacity_reset_interval else None
                    if error_views > 0:
                        views = random.sample(range(len(cameras)), min(error_views, len(cameras)))
                        stats = gaussians.error_stats(cameras, targets, pipe, bg, views=views, correct=bilagrid if use_bilagrid else None)
                        scores = stats.error_max if opt.densify_error_score == "max" else stats.error_sum
                        gaussians.densify_and_prune_by_score(scores, math.ceil(opt.densify_error_growth * gaussians.get_xyz.shape[0]),
                                                             0.005, scene_extent, size_threshold)
                    else:
                        gaussians.densify_and_prune(opt.densify_grad_threshold, 0.005, scene_extent, size_threshold)
                    if filter_3d:
                        gaussians.compute_3D_filter(cameras)
                if it % opt.opacity_reset_interval == 0 or (white_background and it == opt.densify_from_iter):
                    gaussians.reset_opacity()
            if it < iterations:
                if isinstance(gaussians.optimizer, SparseFusedAdam):
                    gaussians.optimizer.step(visibility=radii)           # optimizer_type = "sparse_adam": the frame's radii are the mask
                else:
                    gaussians.optimizer.step()
                gaussians.optimizer.zero_grad(set_to_none=True)
                if use_bilagrid:
                    bilagrid_optimizer.param_groups[0]["lr"] = bilateral_grid_lr(opt.bilateral_grid_lr, it - 1, iterations)
                    bilagrid_optimizer.step()
                    bilagrid_optimizer.zero_grad(set_to_none=True)
                if mcmc and opt.densify_from_iter < it < opt.densify_until_iter and it % opt.densification_interval == 0:
                    gaussians.mcmc_relocate(opt.mcmc_min_opacity)
                    gaussians.mcmc_grow(opt.mcmc_cap_max, opt.mcmc_min_opacity)
                    if filter_3d:
                        gaussians.compute_3D_filter(cameras)
            if it in prune_at:
                k = prune_at.index(it)
                stats = gaussians.contribution_stats(cameras, pipe)
                gaussians.prune_by_significance(gaussians.significance(stats, opt.significance_prune_score),
                                                fraction=opt.significance_prune_fraction * opt.significance_prune_decay ** k)
                if filter_3d:
                    gaussians.compute_3D_filter(cameras)
            if mcmc:
                gaussians.mcmc_inject_noise(opt.mcmc_noise_lr * xyz_lr)
            # Mip-Splatting's schedule once densification is over: every 100 iterations, not in the last 100
            if filter_3d and it % 100 == 0 and opt.densify_until_iter < it < iterations - 100:
                gaussians.compute_3D_filter(cameras)
        if on_iteration is not None:
            on_iteration(it, image_loss, gaussians)
    return gaussians
