"""Drop-in for the reference's `diff_gaussian_rasterization` package, MI355X-native.

Public surface = what the reference imports and calls (gaussian_renderer/__init__.py:14,36-51,85-93):

    GaussianRasterizationSettings(image_height, image_width, tanfovx, tanfovy, bg, scale_modifier,
                                  viewmatrix, projmatrix, sh_degree, campos, prefiltered, debug)
    GaussianRasterizer(raster_settings).forward(means3D, means2D, opacities, shs=None, colors_precomp=None,
                                                scales=None, rotations=None, cov3D_precomp=None)
        -> (color[3,H,W] float32, radii[P] int32)
    GaussianRasterizer.markVisible(positions) -> bool[P]

Extension: GaussianRasterizer(raster_settings, depth_alpha=True) returns (color[3,H,W], radii[P], depth[1,H,W], alpha[1,H,W]) from
the same blend: depth = sum_i w_i z_i (w_i = alpha_i T_i over the splats the colour composites, z_i the view-space depth; no
background term, not normalised: the mean depth is depth / alpha) and alpha = 1 - T_final.  Both are differentiable; a loss on
them reaches means3D (through z too) and means2D - so the densification statistics, which read means2D.grad, see it as well.

Extension: camera gradients.  When grad mode is on and raster_settings.viewmatrix, .projmatrix or .campos requires grad, backward()
also returns dL/dviewmatrix, dL/dprojmatrix and dL/dcampos (camera_grads_wanted), each shaped like the tensor passed and in the
row-vector convention it is consumed in; they are separate gradients, chained by the caller's own torch graph to its pose
parametrisation (scene.cameras.camera_with_pose_delta is one).  Two more launches, sums in a fixed order; off: the plain call.

Extension: GaussianRasterizer(raster_settings, antialiasing=True) is upstream's anti-aliasing switch (the 2D filter of Mip-Splatting):
every opacity is scaled by sqrt(det cov2D / det(cov2D + 0.3 I)) by one differentiable per-Gaussian op in front of the rasterizer
(antialias.compensate_opacity), which then runs exactly as without it; the depth and alpha maps use the compensated opacity too.
Refused with a ValueError: cov3D_precomp, and a viewmatrix / projmatrix / campos that requires grad (rho's camera gradient is not
computed).  Off (the default): no extra launch, the same bits.

Extension: GaussianRasterizer(raster_settings, absgrad=True) is gsplat's `absgrad` (AbsGS / Gaussian Opacity Fields): backward() also
assigns `means2D.absgrad` [P,3] on the very tensor passed as means2D - per Gaussian, the sum over pixels of the ABSOLUTE value of that
pixel's dL/dmean2D, in the layout and scaling of means2D.grad (column 2 exactly 0) - from one more instantiation of the blend backward
and one small extraction launch.  It is assigned, not accumulated, by every backward (a second one under retain_graph included),
whether or not means2D requires grad.  Refused with a ValueError: depth_alpha=True and tile_rows / ShardedRenderer.  Off (the
default): no attribute, no extra launch, the same bits.

Extension: GaussianRasterizer(raster_settings, contributions=stats) with a contrib.ContributionStats also adds the frame's per-Gaussian
blend statistics into `stats` - the pixels that composited each Gaussian, the sum and the maximum of its blend weights w = alpha T -
from one more instantiation of the blend forward (module contrib).  forward / forward_raw return what they return
without it, bit for bit; with antialiasing the compensated opacity is what gets blended.  A statistics frame has no backward.  Refused
with a ValueError: a `stats` of another P or device, depth_alpha=True, absgrad=True, tile_rows / ShardedRenderer, and grad mode on
with an input that requires grad (render under torch.no_grad()).  Off (the default): no extra launch, the same bits.

Extension: GaussianRasterizer(raster_settings, contributions=stats, pixel_error=E) with a contrib.ErrorStats and a float32 error map E
([H,W] or [1,H,W], read clamped to [0, 1]) also scores every Gaussian by the image error it is responsible for in the frame,
E_g = sum over the pixels of w E: a fourth total of the same blend kernel, folded behind the frame's last chunk into stats.error_sum_q32
and stats.error_max (module contrib).  The frame is the plain frame and the three statistics are the statistics
frame's, bit for bit.  Refused with a ValueError: pixel_error without contributions, contributions that is not an ErrorStats, a map of
another shape, dtype or device, and everything a statistics frame refuses.  pixel_error=None: a plain statistics frame.

Extension: GaussianRasterizer(raster_settings, depth_alpha=True)(..., extra_colors=t) with t [P,3] float32 on the frame's device
returns (color, radii, depth, alpha, extra): extra [3,H,W] = sum_i w_i t_i, three more channels blended inside the colour frame with the
colour's own weights and no background term - bit for bit the colour of the same geometry rendered with colors_precomp = t over a
zero background - from one more instantiation of the aux blend kernels.  Differentiable in t and in everything
the weights depend on; color, radii, depth and alpha are the bits of the call without it.  forward and forward_raw (and
FUSE_GETTERS) alike, with debug, antialiasing and a model's 3D filter.  Refused with a ValueError: extra_colors without
depth_alpha=True, another shape, dtype or device, absgrad, contributions, tile_rows / ShardedRenderer, and a viewmatrix / projmatrix /
campos that requires grad.  extra_colors=None (the default): the calls made without it, the same launches, the same bits.

Extension: GaussianRasterizer(raster_settings, depth_alpha=True, median_depth=True) returns (color, radii, depth, alpha, median):
median [1,H,W] is, per pixel, the view depth z_m of the LAST composited splat whose front transmittance T_m (the blend's own float32
T, the value that multiplies alpha_m into w_m) is above one half - the depth at which the accumulated opacity crosses one half, 2DGS's
rule - selected inside the same blend by one more instantiation of the aux kernels.  A pixel with a composited splat
always has one (where the opacity never reaches one half: the farthest composited splat); a pixel nothing composited gets +0.0; not
normalised, no background term: mask by alpha.  The selection is piecewise constant: dL/dmedian of a pixel goes to the depth of that
pixel's median splat, and through it to means3D (and to a viewmatrix that requires grad), and to nothing else.  color, radii, depth,
alpha and their gradients are the bits of the call without the flag.  forward, forward_raw and FUSE_GETTERS alike, with debug,
antialiasing, a model's 3D filter and camera tensors that require grad.  Refused with a ValueError: median_depth without
depth_alpha=True, absgrad, contributions, tile_rows / ShardedRenderer and extra_colors (the ext x median kernels are not built).
Off (the default): the calls made without it, the same launches, the same bits.

Autograd contract (train.py:106, scene/gaussian_model.py:415-417): gradients for
(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, None) in that order;
`means2D.grad[:, :2]` is dL/d(NDC position) with the W/2, H/2 pixel scale folded in, `[:, 2] = 0`.

Everything below the autograd.Function is the C ABI of libgsrast.so (include/gsrast.h): hand-written
gfx950 HIP kernels.  There is no CPU path — missing library => RuntimeError at first use.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import torch
from torch import nn

from . import _native as N


class GaussianRasterizationSettings(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool


def _f32c(t: Optional[torch.Tensor], device=None) -> Optional[torch.Tensor]:
    """Contiguous fp32 view/copy on `device`, or None for missing / empty tensors (the reference passes
    empty tensors for absent optionals; callers may hand in non-contiguous or detached views:
    scene/latent_gaussian_model.py:193-199, scene/gaussian_model.py:104-125)."""
    if t is None or t.numel() == 0:
        return None
    if t.dtype != torch.float32:
        t = t.float()
    if device is not None and t.device != device:
        raise ValueError(f"tensor on {t.device}, rasterizer inputs live on {device}")
    return t.contiguous()


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Opaque byte workspace from torch's caching allocator.  Sizes are rounded up to 1/8-octave steps (<= 12.5 %
    slack) so that frames whose P or R differ a little — another camera, a densification step — hit the same cached
    block instead of a fresh hipMalloc (measured: 35 ms stalls after every densify without it)."""
    n = max(int(nbytes), 1)
    step = 1 << max(n.bit_length() - 4, 12)
    return torch.empty(-(-n // step) * step, dtype=torch.uint8, device=device)


def _binning_bytes(n: int, tiles: int) -> int:
    """gsr_binning_size(desc, n) without the call (csrc/gsr_binning.hip carve_binning; tests/test_abi.py holds the two together):
    six u32 arrays and one byte array of max(n, 1) entries, one 4 KB checkpoint per `seg` instances (+ 2) and the blend backward's
    unit lists (per shard n / seg + 1 full and 16 x 8 (tiles / 8 + 1) partial units of 8 bytes), each block padded to 256 bytes."""
    n, seg, up = max(int(n), 1), N.bwd_segment_entries(), lambda b: (b + 255) // 256 * 256
    return 6 * up(4 * n) + up(n) + up((n // seg + 2) * 4096) + up(8 * (n // seg + 1 + 16 * N.MAX_CHUNKS * (int(tiles) // 8 + 1)) * 8)


_binning_guess = {}        # (P, W, H, slab, device) -> instances the binning workspace of that frame shape last had to hold


class _Frame:
    """Native handles of one forward pass, kept alive by autograd's ctx for the backward."""
    __slots__ = ("desc", "cam", "keep", "plan", "geom_ws", "binning_ws", "image_ws", "radii", "color", "gauss", "M", "device", "raw", "pre",
                 "depth", "alpha", "aux_ws", "aux", "extra_table", "extra_map", "median", "median_enc")

    @property
    def R(self):
        """num_rendered of the reference (upper bound of the instances this frame binned)."""
        return int(self.plan.num_rendered)


def _camera(rs: GaussianRasterizationSettings, device):
    bg, vm, pm, cp = (_f32c(rs.bg, device), _f32c(rs.viewmatrix, device), _f32c(rs.projmatrix, device),
                      _f32c(rs.campos, device))
    if bg is None or vm is None or pm is None or cp is None:
        raise ValueError("bg, viewmatrix, projmatrix and campos must be non-empty device tensors")
    return N.Camera(N._ptr(bg), N._ptr(vm), N._ptr(pm), N._ptr(cp)), (bg, vm, pm, cp)


# torch.autograd.Function.forward runs with grad mode OFF, so "will a backward follow?" must be asked by the public entry
# points BEFORE they call .apply(): they leave the caller's grad mode here (thread-local: the library is re-entrant).
import threading as _threading

_tls = _threading.local()


def _apply(fn, *args, absgrad_to=None):
    """absgrad_to: the caller's means2D tensor when the backward is to assign its .absgrad (GaussianRasterizer(absgrad=True))."""
    _tls.caller_grad = torch.is_grad_enabled()
    _tls.absgrad_to = absgrad_to
    try:
        return fn.apply(*args)
    finally:
        _tls.caller_grad = None
        _tls.absgrad_to = None


def caller_grad_enabled() -> bool:
    g = getattr(_tls, "caller_grad", None)
    return torch.is_grad_enabled() if g is None else g


def camera_grads_wanted(rs: GaussianRasterizationSettings, grad_enabled: Optional[bool] = None, tile_rows=None) -> bool:
    """Does this call return gradients for the camera?  Exactly when grad mode is on (grad_enabled; None: the caller's own) and one
    of rs.viewmatrix / rs.projmatrix / rs.campos requires grad - what autograd users expect of such a tensor; a caller who does
    not want them detaches.  Whole images only: with tile_rows (a sharded slab) a wanted camera gradient raises ValueError."""
    if grad_enabled is None:
        grad_enabled = caller_grad_enabled()
    on = bool(grad_enabled) and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos))
    if on and tile_rows is not None:
        raise ValueError("camera gradients are computed for whole images only: no tile_rows (sharded slabs) with a viewmatrix, "
                         "projmatrix or campos that requires grad (detach them)")
    return on


def _camera_args(rs: GaussianRasterizationSettings):
    """The three extra inputs of the autograd functions: (viewmatrix, projmatrix, campos) when camera gradients are wanted, else ()."""
    return (rs.viewmatrix, rs.projmatrix, rs.campos) if camera_grads_wanted(rs, torch.is_grad_enabled()) else ()


def _aux_outputs(fr: "_Frame", capacity: int):
    """gsr_aux_outputs of an aux frame, with a depth-checkpoint workspace for a binning workspace of `capacity` instances."""
    size = N.aux_workspace_size if fr.extra_table is None else N.extra_workspace_size          # (an extra frame: four planes)
    fr.aux_ws = _workspace(size(fr.desc, capacity), fr.device)
    fr.aux = N.AuxOutputs(N._ptr(fr.depth), N._ptr(fr.alpha), N._ptr(fr.aux_ws))
    return fr.aux


def rasterize_forward(means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp,
                      rs: GaussianRasterizationSettings, tile_rows=None, out_color=None, sh_rest=None, raw=False,
                      prepare_needs=None, aux=False, contrib=None, pixel_error=None, pixel_error_checked=False, extra=None, median=False):
    """Stage 1 + stage 2 of the native forward.  Returns (color, radii, frame).
    aux=True: the same blend also renders frame.depth and frame.alpha ([1,H,W] each; whole images only).
    extra (with aux=True; [P,3] float32 on the inputs' device, whole images, no contrib): the same blend also renders frame.extra_map
    [3,H,W] from it (check_extra_colors' rules).
    median (with aux=True; whole images, no contrib, no extra): the same blend also selects frame.median [1,H,W] and frame.median_enc
    (int32 [H,W], the backward's; check_median_depth's rules).
    contrib (a contrib.ContributionStats of this P and device; whole images, no aux): the blend also adds the frame's per-Gaussian
    statistics into it.  Such a frame runs the two stages as two calls: a stage 2 that stops for want of room in a later chunk has
    already added its earlier chunks, so a frame that can stop that way (several chunks planned, a workspace for fewer than all
    num_rendered instances) first copies the three accumulators, and the re-run starts from the copies.
    pixel_error (with a contrib.ErrorStats as `contrib`; float32 [H,W] or [1,H,W] on the inputs' device): the blend also adds the
    frame's error-weighted totals into contrib.error_frame_q32 (copied and put back with the three), and the fold into error_sum_q32
    and error_max follows the last chunk on the same stream.  pixel_error_checked: the map is what contrib.check_pixel_error
    returned for this frame and `contrib` (GaussianRasterizer checks before anything runs, once).  A frame that raises leaves
    contrib.error_frame_q32 as it found it: zero.
    raw=True: the tensors are the parameter store's RAW values (sh = _features_dc, sh_rest = _features_rest,
    opacities = logits, scales = log-scales, rotations = unnormalised) and the activations run in the kernels.
    prepare_needs: which gradients a backward will want (as rasterize_backward_geom's `needs`), when one will follow: the
    backward's output tensors are then allocated up front, while the host waits for the plan anyway."""
    if extra is not None:
        check_extra_colors(extra, means3D, aux, tile_rows=tile_rows, contributions=contrib, rs=rs)
    if median:
        check_median_depth(aux, tile_rows=tile_rows, contributions=contrib, extra_colors=extra)
    if aux and tile_rows is not None:
        raise ValueError("depth / alpha maps are rendered for whole images only: no tile_rows (sharded slabs) with aux=True")
    if contrib is not None and (aux or tile_rows is not None):
        raise ValueError(_CONTRIB_PLAIN_ONLY)
    if tile_rows is not None:
        camera_grads_wanted(rs, tile_rows=tile_rows)          # raises when a slab is asked for camera gradients
    device = means3D.device
    if contrib is not None:
        from .contrib import check_inputs
        check_inputs(contrib, (means3D,), "rasterize_forward")
    if pixel_error is not None and not pixel_error_checked:
        from .contrib import check_pixel_error
        pixel_error = check_pixel_error(contrib, pixel_error, int(rs.image_height), int(rs.image_width), device, "rasterize_forward")
    if device.type != "cuda":
        raise RuntimeError("diff_gaussian_rasterization (MI355X build) needs tensors on a HIP device; "
                           "there is no CPU path")
    P = int(means3D.shape[0])
    H, W = int(rs.image_height), int(rs.image_width)
    means3D = _f32c(means3D, device)
    sh, colors_precomp = _f32c(sh, device), _f32c(colors_precomp, device)
    opacities = _f32c(opacities, device)
    scales, rotations, cov3D_precomp = _f32c(scales, device), _f32c(rotations, device), _f32c(cov3D_precomp, device)
    sh_rest = _f32c(sh_rest, device)
    M = int(sh.shape[1]) if sh is not None else 0
    raw = int(raw)                   # 0: activated inputs; 1: raw, SH as features_dc + features_rest; 2: raw, SH as one [P,M,3] table
    if raw:
        if sh is None or scales is None or rotations is None or colors_precomp is not None or cov3D_precomp is not None:
            raise ValueError("raw mode takes SH coefficients, log-scales and raw rotations (no precomputed colours / covariances)")
        if raw == 1:
            if M != 1:
                raise ValueError("raw mode takes features_dc [P,1,3], features_rest [P,M-1,3], log-scales and raw rotations")
            M = 1 + (int(sh_rest.shape[1]) if sh_rest is not None else 0)
        elif raw != 2 or sh_rest is not None:
            raise ValueError("raw=2 takes the interleaved SH table [P,M,3] as `sh` and no sh_rest")
    fr = _Frame()
    fr.device, fr.M = device, M
    fr.desc = N.make_desc(P, int(rs.sh_degree), M, W, H, rs.tanfovx, rs.tanfovy, rs.scale_modifier, rs.prefiltered,
                          rs.debug, tile_rows)
    fr.cam, cam_keep = _camera(rs, device)
    fr.gauss = N.Gaussians(N._ptr(means3D), N._ptr(sh), N._ptr(colors_precomp), N._ptr(opacities), N._ptr(scales),
                           N._ptr(rotations), N._ptr(cov3D_precomp), N._ptr(sh_rest), raw)
    fr.keep = (cam_keep, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest)
    fr.raw = raw
    fr.pre = None
    fr.depth = fr.alpha = fr.aux_ws = fr.aux = fr.extra_table = fr.extra_map = fr.median = fr.median_enc = None
    if median:             # every pixel is written by the first chunk's blend
        fr.median = torch.empty(1, H, W, dtype=torch.float32, device=device)
        fr.median_enc = torch.empty(H, W, dtype=torch.int32, device=device)
    med = (fr.median, fr.median_enc) if median else None
    if extra is not None:  # the kernels gather 16-byte rows (e0, e1, e2, unused)
        fr.extra_table = torch.nn.functional.pad(extra.detach().contiguous(), (0, 1))
        fr.extra_map = torch.empty(3, H, W, dtype=torch.float32, device=device)
    if aux:                # every pixel is written by the first chunk's blend
        fr.depth = torch.empty(1, H, W, dtype=torch.float32, device=device)
        fr.alpha = torch.empty(1, H, W, dtype=torch.float32, device=device)
    geom_bytes, image_bytes = N.workspace_sizes(fr.desc)
    fr.geom_ws = _workspace(geom_bytes, device)
    fr.image_ws = _workspace(image_bytes, device)
    fr.radii = torch.empty(P, dtype=torch.int32, device=device)            # every entry is written by the preprocess kernel
    with torch.cuda.device(device):
        # Everything that can be allocated before the plan readback is: the stream is idle while the host waits for R,
        # so the first kernels of the second stage should follow the readback as closely as possible.  The binning
        # workspace is guessed from the last frame of the same shape and re-allocated only when R outgrew it.
        if out_color is not None:
            color = out_color
        else:       # a full-frame render writes every pixel; a slab leaves the other rows untouched, so those start at 0
            color = (torch.empty if tile_rows is None else torch.zeros)(3, H, W, dtype=torch.float32, device=device)
        guess_key = (P, W, H, None if tile_rows is None else tuple(int(v) for v in tile_rows), device.index)
        guess = _binning_guess.get(guess_key, 0)
        tiles = ((W + 15) // 16) * ((H + 15) // 16)
        binning = _workspace(_binning_bytes(guess, tiles), device) if guess > 0 else None
        early = None
        if prepare_needs is not None and P > 0 and any(prepare_needs) and caller_grad_enabled():
            needs = tuple(bool(x) for x in prepare_needs)
            early = (needs,) + _alloc_grads(fr, needs, torch.empty) + (torch.empty(P, N.SCREEN_GRAD_STRIDE, dtype=torch.float32, device=device),)
        # With a workspace guessed from the last frame of this shape both stages run in ONE native call (gsr_forward): the
        # stream is idle from the plan readback until stage 2's first launch, and a trip through the interpreter in between
        # doubles that gap.  The call also enqueues the backward's zero fill itself, right after stage 2's last readback.
        done = False
        if binning is not None and contrib is None:
            plan, done = N.forward_both(fr.desc, fr.cam, fr.gauss, fr.geom_ws, fr.image_ws, fr.radii, binning, guess, color, device,
                                        early_fill=early[2] if early is not None else None,
                                        aux=_aux_outputs(fr, guess) if aux else None,
                                        extra=None if extra is None else (fr.extra_table, fr.extra_map), median=med)
        else:
            plan = N.forward_preprocess(fr.desc, fr.cam, fr.gauss, fr.geom_ws, fr.radii, device, image_ws=fr.image_ws)
        fr.plan = plan
        if early is not None:          # handed to the backward; prepare_backward() zero-fills them on sparse frames
            needs, tensors, grads, screen = early
            fr.pre = {"needs": needs, "tensors": tensors, "grads": grads, "screen": screen}
        # The binning workspace (24 B per instance) is sized for what the FIRST depth chunk can emit, not for the upper bound R
        # of every chunk (11.8 GB at 5e6 Gaussians / 4K): frames whose tiles saturate never get past that chunk.  A frame that
        # does need more stops with GSR_ERR_WORKSPACE before it writes anything it has no room for, and is re-run once with a
        # workspace for R; frames of that shape then start with R.  (Plain arithmetic here, no library calls: the stream is
        # idle between the plan readback and the first launch of stage 2.)
        R = int(plan.num_rendered)
        if done:
            capacity = int(plan.binning_capacity) if plan.binning_capacity > 0 else guess
            fr.binning_ws = binning
        else:
            capacity = max(N.first_chunk_capacity(plan), min(guess, R))
            if binning is not None and capacity <= guess and contrib is None:
                capacity = R                                   # the guessed workspace covered the first chunk, a later one did not fit
        # a statistics frame that may stop in a later chunk: what the accumulators held before it
        accumulators = () if contrib is None else (contrib.count, contrib.weight_sum_q32, contrib.weight_max)
        if pixel_error is not None:
            accumulators += (contrib.error_frame_q32,)
        saved = [t.clone() for t in accumulators] if contrib is not None and capacity < R else None
        while not done:
            need = _binning_bytes(capacity, tiles)
            if binning is None or binning.numel() < need:
                binning = _workspace(need, device)
            plan.binning_capacity = capacity
            fr.binning_ws = binning
            try:
                N.forward_render(fr.desc, fr.cam, fr.gauss, fr.geom_ws, binning, fr.image_ws, plan, color, device,
                                 aux=_aux_outputs(fr, capacity) if aux else None,
                                 extra=None if extra is None else (fr.extra_table, fr.extra_map), median=med,
                                 contrib=contrib.native() if contrib is not None else None,
                                 err=contrib.native_error(pixel_error) if pixel_error is not None else None)
                if pixel_error is not None:
                    contrib.fold()
                if contrib is not None:
                    contrib.frames += 1
                break
            except N.GsrError as e:
                if e.status != N.ERR_WORKSPACE or capacity >= R:
                    if pixel_error is not None:                # no fold follows: the chunks that ran must not reach the next frame's
                        contrib.error_frame_q32.zero_()
                    raise
                capacity, binning = R, None
                if saved is not None:                          # (behind the chunks that ran, on the same stream)
                    for t, t0 in zip(accumulators, saved):
                        t.copy_(t0)
        _binning_guess[guess_key] = capacity
        if len(_binning_guess) > 64:
            _binning_guess.pop(next(iter(_binning_guess)))
    fr.color = color               # the blend backward walks the lists front to back and needs the final pixel
    return color, fr.radii, fr


def rasterize_backward_screen(fr: "_Frame", grad_color: torch.Tensor, only_for_own_geom: bool = False, grad_depth=None,
                              grad_alpha=None, absgrad: bool = False, grad_extra=None, extra_out=None, grad_median=None) -> torch.Tensor:
    """K7 + deterministic per-Gaussian reduction -> screen-space gradients [P, 12].
    grad_depth / grad_alpha ([1,H,W] or [H,W], an aux frame only; None = zero): when either is given the aux backward runs and slot 9
    holds dL/dz; otherwise the colour-only kernels (the plain frame's bits).
    grad_extra ([3,H,W], an extra frame only; None = zero) / extra_out ([P,3], required for an extra frame): an extra frame always
    runs the ext backward - slot 9 as the aux backward leaves it - which also writes the extra table's gradient into extra_out.
    grad_median ([1,H,W] or [H,W], a median frame only; None = zero): when given the median backward runs - the aux backward whose
    slot 9 also gains the median's share of dL/dz; without it a median frame takes the aux frame's calls.
    absgrad: the abs instantiation of the colour-only kernels - slots 10, 11 also hold the per-pixel absolute sums of d/dmean2D
    (rasterize_screen_absgrad extracts them); whole images, no aux gradients.
    only_for_own_geom: the tensor goes straight into this frame's geometry backward and nowhere else (the autograd path): rows it
    never reads may stay undefined.  The dense geometry backward reads the rows of VISIBLE Gaussians; when every planned chunk ran,
    all of them sit in the binned prefix, whose rows the reduction writes (zeros included): no 48 P-byte memset."""
    P = fr.desc.P
    grad_color = _f32c(grad_color, fr.device)
    grad_depth, grad_alpha = _f32c(grad_depth, fr.device), _f32c(grad_alpha, fr.device)
    with_aux = fr.aux is not None and (grad_depth is not None or grad_alpha is not None)
    with_ext = fr.extra_table is not None
    grad_extra = _f32c(grad_extra, fr.device) if with_ext else None
    if with_ext and extra_out is None:
        raise ValueError("rasterize_backward_screen: an extra frame's backward needs extra_out [P,3]")
    with_aux = with_aux or (with_ext and grad_extra is not None)
    grad_median = _f32c(grad_median, fr.device) if fr.median_enc is not None else None
    with_aux = with_aux or grad_median is not None
    if absgrad and (fr.aux is not None or fr.desc.tile_row_end > 0 or fr.desc.tile_row_begin != 0):
        raise ValueError("absgrad: the abs blend backward is built for whole colour-only frames: no depth / alpha maps, no tile_rows")
    screen = fr.pre.pop("screen", None) if fr.pre is not None else None        # allocated (and, on sparse frames, zero-filled) by the forward
    if screen is None:
        screen = torch.empty(max(P, 1), N.SCREEN_GRAD_STRIDE, dtype=torch.float32, device=fr.device)
        covered = fr.plan.num_rendered > 0 and fr.plan.chunks_run == fr.plan.num_chunks
        fr.plan.screen_prezeroed = 2 if (only_for_own_geom and covered) else 0            # (1: set only by prepare_backward(), for the very tensor it filled)
    if grad_color is None and not with_aux:
        if with_ext:
            extra_out.zero_()
        return screen.zero_()[:P]
    with torch.cuda.device(fr.device):
        # one 48-B gradient row per EMITTED instance: backward-only scratch, returned to the allocator on exit
        rows = _workspace(N.backward_rows_size(fr.desc, fr.plan), fr.device)
        if with_ext:
            ext_rows = _workspace(N.extra_rows_size(fr.desc, fr.plan), fr.device)
            N.backward_render_extra(fr.desc, fr.cam, fr.geom_ws, fr.binning_ws, fr.image_ws, rows, fr.plan, fr.color, fr.aux, fr.extra_table,
                                    fr.extra_map, grad_color, grad_depth, grad_alpha, grad_extra, screen, ext_rows, extra_out, fr.device)
        elif grad_median is not None:
            N.backward_render_median(fr.desc, fr.cam, fr.geom_ws, fr.binning_ws, fr.image_ws, rows, fr.plan, fr.color, fr.aux, grad_color,
                                     grad_depth, grad_alpha, fr.median_enc, grad_median, screen, fr.device)
        elif with_aux:
            N.backward_render_aux(fr.desc, fr.cam, fr.geom_ws, fr.binning_ws, fr.image_ws, rows, fr.plan, fr.color, fr.aux, grad_color,
                                  grad_depth, grad_alpha, screen, fr.device)
        else:
            N.backward_render(fr.desc, fr.cam, fr.geom_ws, fr.binning_ws, fr.image_ws, rows, fr.plan, fr.color, grad_color, screen,
                              fr.device, absgrad=absgrad)
        fr.plan.screen_prezeroed = 0
    return screen[:P]


def _alloc_grads(fr: "_Frame", needs, alloc):
    """Gradient tensors of one frame (None where not wanted / not applicable) and their gsr_grads struct."""
    P, M, dev = fr.desc.P, fr.M, fr.device
    (_, means3D, sh, colors_precomp, opacities, scales, rotations, cov3D_precomp, sh_rest) = fr.keep

    def mk(flag, present, *shape):
        return alloc(*shape, dtype=torch.float32, device=dev) if (flag and present) else None
    t = (mk(needs[0], True, P, 3), mk(needs[1], True, P, 3), mk(needs[2], sh is not None, P, 1 if fr.raw == 1 else M, 3),
         mk(needs[3], colors_precomp is not None, P, 3), mk(needs[4], True, P, 1), mk(needs[5], scales is not None, P, 3),
         mk(needs[6], rotations is not None, P, 4), mk(needs[7], cov3D_precomp is not None, P, 6),
         mk(fr.raw == 1 and len(needs) > 8 and needs[8], sh_rest is not None, P, M - 1, 3))
    grads = N.Grads(N._ptr(t[0]), N._ptr(t[1]), N._ptr(t[2]), N._ptr(t[3]), N._ptr(t[4]), N._ptr(t[5]), N._ptr(t[6]),
                    N._ptr(t[7]), N._ptr(t[8]), 0)
    return t, grads


def prepare_backward(fr: "_Frame", needs, screen_prefix_only: bool = False) -> None:
    """Called right after the forward when a backward will follow: the stream is idle while the host walks back
    through the caller's code to the loss, so the backward's zero fills (screen-space gradients + the parameter
    gradients of the sparse geometry backward, ~280 MB at 1e6 Gaussians) are enqueued NOW, in one launch, into the
    tensors the forward allocated up front (rasterize_forward(prepare_needs=...)) or into fresh ones.
    (Measured and dropped: the same fill on a second stream beside the stage-2 kernels or beside k_render_bwd — the
    fill takes 65-86 us instead of 53 and the kernels it runs beside slow down by as much: no step time is gained.)"""
    P, plan = fr.desc.P, fr.plan
    # ctx.needs_input_grad stays True for leaf parameters under torch.no_grad() (eval / test-view renders): no backward can follow
    if P == 0 or plan.num_rendered <= 0 or plan.chunks_run <= 0 or not any(needs) or not caller_grad_enabled():
        return
    if N.effective_binned_ranks(plan) * 4 >= P:
        return                                  # the dense geometry backward writes every row itself
    needs = tuple(bool(x) for x in needs)
    if fr.pre is None or fr.pre["needs"] != needs:
        tensors, grads = _alloc_grads(fr, needs, torch.empty)
        fr.pre = {"needs": needs, "tensors": tensors, "grads": grads,
                  "screen": torch.empty(P, N.SCREEN_GRAD_STRIDE, dtype=torch.float32, device=fr.device)}
    if fr.pre["grads"].prezeroed:              # gsr_forward has already enqueued the fill (parameter gradients only)
        if screen_prefix_only:
            plan.screen_prezeroed = 2
        return
    with torch.cuda.device(fr.device):
        # screen_prefix_only: the screen-space gradients go straight into this frame's sparse geometry backward, which reads
        # the rows of the binned prefix only (the autograd path): that tensor needs no clearing at all
        N.backward_prepare(fr.desc, fr.gauss, plan, None if screen_prefix_only else fr.pre["screen"], fr.pre["grads"], fr.device)
        if screen_prefix_only:
            plan.screen_prezeroed = 2


def rasterize_backward_geom(fr: "_Frame", screen: torch.Tensor, needs, g0: int = 0, g1: Optional[int] = None,
                            binned_ranks: Optional[int] = None, rows: Optional[torch.Tensor] = None, depth_chain: bool = False):
    """K8 + K9 on Gaussians [g0, g1).  `needs` = (means3D, means2D, sh, colors, opacities, scales, rotations,
    cov3D[, sh_rest]) booleans.  Returns the 8 gradient tensors (None where not needed / not applicable); for a
    raw-mode frame 9: sh is then d/d_features_dc [P,1,3] and the ninth d/d_features_rest [P,M-1,3].
    rows (int32 device tensor, whole range only): the Gaussians that can have a non-zero screen gradient, when that is not
    the frame's own binned prefix (a sharded render: the union over the ranks).
    depth_chain: `screen` came from the aux backward (slot 9 = dL/dz): its chain to means3D is added."""
    P, dev = fr.desc.P, fr.device
    g1 = P if g1 is None else g1
    partial = (g0, g1) != (0, P)
    pre, fr.pre = fr.pre, None
    if pre is not None and not partial and tuple(bool(x) for x in needs) == pre["needs"]:
        tensors, grads = pre["tensors"], pre["grads"]                  # allocated and zero-filled right after the forward; used once
    else:
        tensors, grads = _alloc_grads(fr, needs, torch.zeros if partial else torch.empty)
    g_means3D, g_means2D, g_sh, g_col, g_op, g_sc, g_rot, g_cov, g_rest = tensors
    if P > 0 and g1 > g0:
        with torch.cuda.device(dev):
            if rows is not None and not partial:
                N.backward_geom_rows(fr.desc, fr.cam, fr.gauss, fr.radii, fr.geom_ws, screen, rows, grads, dev)
                binned_ranks = -2
            own = None
            if rows is None and binned_ranks is None:        # gradients of this very frame: its own binned depth prefix
                own = fr.plan
                binned_ranks = N.binned_prefix(own)
            if binned_ranks != -2:
                N.backward_geom(fr.desc, fr.cam, fr.gauss, fr.radii, fr.geom_ws, screen, g0, g1, grads, dev, binned_ranks,
                                own_plan=None if partial else own, depth_chain=depth_chain)
    if fr.raw:
        return g_means3D, g_means2D, g_sh, g_col, g_op, g_sc, g_rot, g_cov, g_rest
    return g_means3D, g_means2D, g_sh, g_col, g_op, g_sc, g_rot, g_cov


def rasterize_backward_camera(fr: "_Frame", screen: torch.Tensor, needs=(True, True, True), depth_chain: bool = False):
    """Camera gradients of this very frame, behind rasterize_backward_geom(fr, screen, ...) of the whole range: (dL/dviewmatrix [4,4],
    dL/dprojmatrix [4,4], dL/dcampos [3]), None where `needs` says not wanted.  Two launches (per-block partial sums over the rows the
    geometry backward visited, then their sum in block order): the same frame gives the same bits.
    depth_chain: `screen` came from the aux backward: the depth map's chain through z is added to dL/dviewmatrix."""
    dev, plan = fr.device, fr.plan
    out = torch.empty(35, dtype=torch.float32, device=dev)
    parts = (out[:16], out[16:32], out[32:35])
    grads = N.CameraGrads(*(N._ptr(t) if n else None for t, n in zip(parts, needs)))
    with torch.cuda.device(dev):
        ws = _workspace(N.camera_grad_workspace_size(fr.desc), dev)
        N.backward_camera(fr.desc, fr.cam, fr.gauss, fr.radii, fr.geom_ws, screen, ws, grads, dev, N.binned_prefix(plan), own_plan=plan,
                          depth_chain=depth_chain)
    return tuple((t.view(4, 4) if t.numel() == 16 else t) if n else None for t, n in zip(parts, needs))


def rasterize_screen_absgrad(fr: "_Frame", screen: torch.Tensor) -> torch.Tensor:
    """The absolute sums [P,3] = (slot 10, slot 11, 0) of this very frame's rasterize_backward_screen(..., absgrad=True), over the
    rows rasterize_backward_geom(fr, screen, ...) of the whole range visits; zeros elsewhere.  One launch (a fill first on sparse frames)."""
    P, dev = fr.desc.P, fr.device
    out = torch.empty(P, 3, dtype=torch.float32, device=dev)
    if P > 0:
        with torch.cuda.device(dev):
            N.screen_absgrad(fr.desc, fr.radii, fr.geom_ws, screen, out, dev, N.binned_prefix(fr.plan), own_plan=fr.plan)
    return out


def _assign_absgrad(ctx, fr, screen):
    """backward() of an absgrad call: means2D.absgrad = the frame's absolute sums, on the tensor the caller passed (assigned, not added)."""
    target = ctx.absgrad_to
    if target is not None:
        target.absgrad = rasterize_screen_absgrad(fr, screen).view(ctx.shapes[0])


def _camera_meta(ctx, cam, first):
    """forward(): remember whether the three camera inputs were passed, which of them want a gradient, their shapes and dtypes."""
    ctx.cam_needs = tuple(ctx.needs_input_grad[first:first + 3]) if cam[0] is not None else None
    ctx.cam_meta = tuple((t.shape, t.dtype) for t in cam) if cam[0] is not None else None


def _camera_backward(ctx, fr, screen, depth_chain):
    """backward(): the camera inputs' gradients, each in its input's shape and dtype (a transposed / non-contiguous input: element
    for element); () when the inputs were not passed."""
    if ctx.cam_needs is None:
        return ()
    if not any(ctx.cam_needs):
        return (None, None, None)
    grads = rasterize_backward_camera(fr, screen, ctx.cam_needs, depth_chain)
    return tuple(None if g is None else g.view(shape).to(dtype) for g, (shape, dtype) in zip(grads, ctx.cam_meta))


def _dump(path, payload):
    try:
        torch.save(payload, path)
    except Exception:      # the dump is a debugging aid; never mask the original error
        pass


_FRAME_TENSORS = ("geom_ws", "binning_ws", "image_ws", "radii", "color")       # color: the forward's OUTPUT, saved like the upstream
# extension saves its buffers — a caller that modifies the rendered image in place before backward() gets autograd's usual error


def _stash_frame(ctx, frame):
    """Hand the frame's device buffers (workspaces, radii, the contiguous input copies) to autograd's saved-tensor slots:
    like the upstream extension's saved buffers they are released right after backward() — or kept, and a second
    backward() allowed, under retain_graph=True; a second backward() without it raises autograd's usual error."""
    keep = [t for t in frame.keep[1:] if t is not None]
    aux = (frame.depth, frame.aux_ws) if frame.aux is not None else ()          # an aux frame: its depth map and checkpoints, last
    ext = (frame.extra_table, frame.extra_map) if frame.extra_table is not None else ()      # an extra frame: its table and map, in front
    med = (frame.median_enc,) if frame.median_enc is not None else ()           # a median frame: which entry each pixel's median is
    ctx.save_for_backward(*(getattr(frame, n) for n in _FRAME_TENSORS), *frame.keep[0], *keep, *ext, *med, *aux)
    ctx.frame_keep_mask = tuple(t is not None for t in frame.keep[1:])
    ctx.frame_aux = bool(aux)
    ctx.frame_ext = bool(ext)
    ctx.frame_med = bool(med)
    for n in _FRAME_TENSORS:
        setattr(frame, n, None)
    frame.keep = None
    frame.depth = frame.alpha = frame.aux_ws = frame.extra_table = frame.extra_map = frame.median = frame.median_enc = None
    ctx.frame = frame


def _unstash_frame(ctx):
    fr = ctx.frame
    saved = ctx.saved_tensors                      # raises if the graph's buffers were already freed
    for n, t in zip(_FRAME_TENSORS, saved[:5]):
        setattr(fr, n, t)
    it = iter(saved[9:])
    fr.keep = (tuple(saved[5:9]),) + tuple(next(it) if m else None for m in ctx.frame_keep_mask)
    if ctx.frame_ext:
        fr.extra_table, fr.extra_map = next(it), next(it)
    if ctx.frame_med:
        fr.median_enc = next(it)
    if ctx.frame_aux:
        fr.depth, fr.aux_ws = saved[-2], saved[-1]
        fr.aux = N.AuxOutputs(N._ptr(fr.depth), None, N._ptr(fr.aux_ws))      # (the backward does not read alpha)
    return fr


def _restash_frame(fr):
    for n in _FRAME_TENSORS:
        setattr(fr, n, None)
    fr.keep = None
    fr.depth = fr.aux_ws = fr.extra_table = fr.extra_map = fr.median_enc = None
    fr.plan.screen_prezeroed = 0


def _finish_forward(ctx, frame, color, radii, aux, means2D, opacities):
    """The tail of both Functions' forward(): the frame into autograd's slots, what backward() needs on ctx, the return tuple."""
    maps = (frame.depth, frame.alpha) + ((frame.extra_map,) if frame.extra_map is not None else ())
    maps += (frame.median,) if frame.median is not None else ()
    _stash_frame(ctx, frame)
    ctx.absgrad_to = getattr(_tls, "absgrad_to", None)
    ctx.shapes = (means2D.shape, opacities.shape)
    ctx.mark_non_differentiable(radii)
    ctx.set_materialize_grads(False)         # radii's "gradient" would arrive as a zero-filled int32 [P] tensor: one launch per step
    return (color, radii) + (maps if aux else ())


def _backward_core(ctx, fr, needs, grad_out_color, grad_depth, grad_alpha, grad_fifth=None):
    """The core of both Functions' backward(): (rasterize_backward_geom's gradients for `needs`, means2D's and the opacities' in
    their inputs' shapes; the camera gradients - for an extra frame (no camera gradients) the tail of the inputs' gradients instead:
    three Nones and the extra colours').  grad_fifth: the gradient of the call's fifth output - the extra map's, or a median frame's
    median map's.  The frame goes back to its stashed state."""
    grad_median = grad_fifth if fr.median_enc is not None else None
    grad_extra = grad_fifth if fr.extra_table is not None else None
    # no depth / alpha gradient: the colour-only kernels, bit for bit the plain frame's gradients
    with_aux = grad_depth is not None or grad_alpha is not None or grad_median is not None
    g_extra = None
    if fr.extra_table is not None:            # an extra frame: the ext backward, which leaves slot 9 as the aux backward does
        with_aux = True
        g_extra = torch.empty(fr.desc.P, 3, dtype=torch.float32, device=fr.device)
    screen = rasterize_backward_screen(fr, grad_out_color, only_for_own_geom=True, grad_depth=grad_depth, grad_alpha=grad_alpha,
                                       absgrad=ctx.absgrad_to is not None, grad_extra=grad_extra, extra_out=g_extra, grad_median=grad_median)
    g = list(rasterize_backward_geom(fr, screen, needs, depth_chain=with_aux))
    g_cam = _camera_backward(ctx, fr, screen, with_aux)
    if g_extra is not None:
        g_cam = (None, None, None, g_extra if ctx.extra_needs else None)
    _assign_absgrad(ctx, fr, screen)
    for i, shape in ((1, ctx.shapes[0]), (4, ctx.shapes[1])):         # means2D, opacities
        if g[i] is not None:
            g[i] = g[i].view(shape)
    _restash_frame(fr)
    return g, g_cam


class _RasterizeGaussians(torch.autograd.Function):
    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                raster_settings, aux=False, viewmatrix=None, projmatrix=None, campos=None, extra_colors=None):
        # viewmatrix / projmatrix / campos: raster_settings' own tensors, passed as inputs only when camera gradients are wanted
        # (camera_grads_wanted): the values are read from raster_settings either way
        # extra_colors: passed only by a call with extra colours (behind three Nones: such a call has no camera gradients)
        rs = raster_settings
        _camera_meta(ctx, (viewmatrix, projmatrix, campos), 10)
        ctx.extra_needs = extra_colors is not None and ctx.needs_input_grad[13]
        args = (means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp)
        if rs.debug:
            cpu_args = tuple(a.detach().cpu().clone() for a in args)      # README.md:147-150 semantics
            try:
                color, radii, frame = rasterize_forward(*args, rs, aux=bool(aux), extra=extra_colors, median=aux == _AUX_MEDIAN)
                torch.cuda.synchronize(means3D.device)
            except Exception:
                _dump("snapshot_fw.dump", (cpu_args, tuple(rs)))
                print("\nAn error occured in forward. Please forward snapshot_fw.dump for debugging.")
                raise
        else:
            color, radii, frame = rasterize_forward(*args, rs, prepare_needs=tuple(ctx.needs_input_grad[:8]), aux=bool(aux), extra=extra_colors,
                                                    median=aux == _AUX_MEDIAN)
            prepare_backward(frame, tuple(ctx.needs_input_grad[:8]), screen_prefix_only=True)
        ctx.raster_settings = rs
        return _finish_forward(ctx, frame, color, radii, aux, means2D, opacities)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_depth=None, grad_alpha=None, grad_fifth=None):
        fr, rs = _unstash_frame(ctx), ctx.raster_settings
        # input order: means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp
        needs = tuple(ctx.needs_input_grad[:8])
        if rs.debug:
            kept = fr.keep[1:]                 # (the frame lets go of them once its gradients are enqueued)
            try:
                g, g_cam = _backward_core(ctx, fr, needs, grad_out_color, grad_depth, grad_alpha, grad_fifth)
                torch.cuda.synchronize(fr.device)
            except Exception:
                _dump("snapshot_bw.dump", (tuple(None if k is None else k.detach().cpu() for k in kept),
                                           None if grad_out_color is None else grad_out_color.detach().cpu(), tuple(rs)))
                print("\nAn error occured in backward. Writing snapshot_bw.dump for debugging.\n")
                raise
        else:
            g, g_cam = _backward_core(ctx, fr, needs, grad_out_color, grad_depth, grad_alpha, grad_fifth)
        return (*g, None, None) + g_cam


class _RasterizeGaussiansRaw(torch.autograd.Function):
    """SURVEY 8a row a14 fused: same rasterizer, fed with the parameter store's RAW tensors.  The activations of
    scene/gaussian_model.py:47-60 (exp, sigmoid, normalize) and the torch.cat of get_features (:120-123) run inside
    the preprocess kernel, their chain rule inside the geometry backward: gradients arrive on the raw parameters."""

    @staticmethod
    def forward(ctx, xyz, means2D, features_dc, features_rest, opacity_logits, log_scales, raw_rotations, raster_settings, aux=False,
                viewmatrix=None, projmatrix=None, campos=None, extra_colors=None):
        rs = raster_settings
        _camera_meta(ctx, (viewmatrix, projmatrix, campos), 9)         # (as _RasterizeGaussians.forward)
        ctx.extra_needs = extra_colors is not None and ctx.needs_input_grad[12]
        n = ctx.needs_input_grad       # xyz, means2D, f_dc, f_rest, opacity, scales, rotations
        needs = (n[0], n[1], n[2], False, n[4], n[5], n[6], False, n[3])
        # features_rest None: features_dc is the whole interleaved table [P,M,3] (scene.GaussianModel's packed leaf)
        color, radii, frame = rasterize_forward(xyz, features_dc, None, opacity_logits, log_scales, raw_rotations, None, rs,
                                                sh_rest=features_rest, raw=2 if features_rest is None else 1,
                                                prepare_needs=None if rs.debug else needs, aux=bool(aux), extra=extra_colors,
                                                median=aux == _AUX_MEDIAN)
        if rs.debug:
            torch.cuda.synchronize(xyz.device)
        prepare_backward(frame, needs, screen_prefix_only=True)
        return _finish_forward(ctx, frame, color, radii, aux, means2D, opacity_logits)

    @staticmethod
    def backward(ctx, grad_out_color, _grad_radii, grad_depth=None, grad_alpha=None, grad_fifth=None):
        n = ctx.needs_input_grad       # xyz, means2D, f_dc, f_rest, opacity, scales, rotations
        needs = (n[0], n[1], n[2], False, n[4], n[5], n[6], False, n[3])
        g, g_cam = _backward_core(ctx, _unstash_frame(ctx), needs, grad_out_color, grad_depth, grad_alpha, grad_fifth)
        g_xyz, g_means2D, g_dc, _, g_op, g_sc, g_rot, _, g_rest = g
        return (g_xyz, g_means2D, g_dc, g_rest, g_op, g_sc, g_rot, None, None) + g_cam


_AUX_MEDIAN = 2            # the autograd functions' `aux` argument of a median frame (False / True: none / the depth and alpha maps)


def check_median_depth(depth_alpha, absgrad=False, contributions=None, tile_rows=None, extra_colors=None):
    """The rules of `median_depth` (module docstring), checked before anything runs: a ValueError with the reason."""
    who = "median_depth"
    if absgrad:
        raise ValueError(f"{who}: not with absgrad=True (the abs blend backward carries no depth gradients)")
    if contributions is not None:
        raise ValueError(f"{who}: not with contributions (a statistics frame is the plain colour forward)")
    if not depth_alpha:
        raise ValueError(f"{who}: the median rides on the depth / alpha blend kernels: construct the rasterizer with depth_alpha=True")
    if tile_rows is not None:
        raise ValueError(f"{who}: whole images only: no tile_rows (sharded slabs / ShardedRenderer)")
    if extra_colors is not None:
        raise ValueError(f"{who}: not with extra_colors (the ext x median blend kernels are not built): render the median in a frame "
                         "of its own")


def check_extra_colors(extra_colors, means3D, depth_alpha, absgrad=False, contributions=None, tile_rows=None, rs=None):
    """The rules of `extra_colors` (module docstring), checked before anything runs: a ValueError with the reason."""
    who = "extra_colors"
    if absgrad:
        raise ValueError(f"{who}: not with absgrad=True (the abs blend backward carries neither the depth / alpha nor the extra gradients)")
    if contributions is not None:
        raise ValueError(f"{who}: not with contributions (a statistics frame is the plain colour forward)")
    if not depth_alpha:
        raise ValueError(f"{who}: the extra channels ride on the depth / alpha blend kernels: construct the rasterizer with depth_alpha=True")
    if tile_rows is not None:
        raise ValueError(f"{who}: whole images only: no tile_rows (sharded slabs / ShardedRenderer)")
    if not isinstance(extra_colors, torch.Tensor):
        raise ValueError(f"{who}: a float32 tensor [P,3] is expected, got {type(extra_colors).__name__}")
    P = int(means3D.shape[0])
    if tuple(extra_colors.shape) != (P, 3):
        raise ValueError(f"{who}: shape {tuple(extra_colors.shape)}, expected ({P}, 3): three values per Gaussian")
    if extra_colors.dtype != torch.float32:
        raise ValueError(f"{who}: dtype {extra_colors.dtype}, expected torch.float32")
    if extra_colors.device != means3D.device:
        raise ValueError(f"{who}: on {extra_colors.device}, the frame's inputs live on {means3D.device}")
    if rs is not None and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
        raise ValueError(f"{who}: camera gradients are not computed for the extra channels: detach viewmatrix, projmatrix and campos")


def _extra_args(extra_colors):
    """The tail of an autograd call with extra colours: no camera inputs (refused), then the tensor.  None: nothing, the call as it was."""
    return () if extra_colors is None else (None, None, None, extra_colors)


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp,
                        raster_settings, depth_alpha=False, absgrad=False, extra_colors=None, median_depth=False):
    if median_depth:
        check_median_depth(depth_alpha, absgrad, extra_colors=extra_colors)
    if absgrad and depth_alpha:
        raise ValueError(_ABSGRAD_NO_AUX)
    if extra_colors is not None:
        check_extra_colors(extra_colors, means3D, depth_alpha, absgrad, rs=raster_settings)
        return _apply(_RasterizeGaussians, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                      cov3Ds_precomp, raster_settings, True, *_extra_args(extra_colors))
    return _apply(_RasterizeGaussians, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                  cov3Ds_precomp, raster_settings, _AUX_MEDIAN if median_depth else bool(depth_alpha), *_camera_args(raster_settings),
                  absgrad_to=means2D if absgrad else None)


_CONTRIB_PLAIN_ONLY = ("contributions: the statistics kernel is the plain colour forward's - no depth_alpha=True, no absgrad=True and no "
                       "tile_rows (sharded slabs); render those in separate calls")


_ABSGRAD_NO_AUX = ("absgrad=True with depth_alpha=True: the blend backward that carries both the depth / alpha gradients and the "
                   "absolute sums is not built; render the two in separate calls")


# ---- opt-in: fuse the reference's getters without touching the caller -------------------------------------------
# With FUSE_GETTERS on (module attribute, or GSR_FUSE_GETTERS=1 in the environment) GaussianRasterizer.forward looks at
# the autograd history of its arguments.  If they are exactly what the reference's GaussianModel getters produce from
# leaf parameters — opacities = sigmoid(leaf), scales = exp(leaf), rotations = F.normalize(leaf),
# shs = cat((leaf_dc, leaf_rest), 1), means3D a leaf (scene/gaussian_model.py:101-125) — the frame is rendered
# from those leaves with the activations inside the kernels (forward_raw).  Pixels are the same; the gradients reach
# the same leaves with the same values to fp32 rounding, but the ~15 torch kernels of the getters' backward (and the
# 2 x 192 MB copies of cat's) never run.  Anything that does not match falls back to the plain path.  Not default:
# hooks / retain_grad() on the intermediate activated tensors would not fire.
import os as _os

FUSE_GETTERS = _os.environ.get("GSR_FUSE_GETTERS", "0") not in ("", "0")


def _leaf_of(fn, index=0):
    """The leaf tensor behind input `index` of autograd node `fn`, or None."""
    nxt = fn.next_functions
    if index >= len(nxt) or nxt[index][0] is None or type(nxt[index][0]).__name__ != "AccumulateGrad":
        return None
    return nxt[index][0].variable


def _unary_getter(t, node_name):
    fn = t.grad_fn
    if fn is None or type(fn).__name__ != node_name or len(fn.next_functions) != 1:
        return None
    leaf = _leaf_of(fn)
    return leaf if leaf is not None and leaf.shape == t.shape and leaf.dtype == torch.float32 else None


def _normalize_getter(t):
    """leaf such that t = torch.nn.functional.normalize(leaf) (p = 2, dim = 1, eps = 1e-12), or None."""
    fn = t.grad_fn
    if fn is None or type(fn).__name__ != "DivBackward0" or len(fn.next_functions) != 2:
        return None
    leaf = _leaf_of(fn, 0)
    node = fn.next_functions[1][0]
    for name in ("ExpandBackward0", "ClampMinBackward0", "LinalgVectorNormBackward0"):
        if node is None or type(node).__name__ != name:
            return None
        if name == "ClampMinBackward0" and abs(float(node._saved_min) - 1e-12) > 1e-18:
            return None
        if name == "LinalgVectorNormBackward0":
            if float(node._saved_ord) != 2.0 or tuple(node._saved_dim) != (1,) or not node._saved_keepdim:
                return None
            if _leaf_of(node) is not leaf:
                return None
            break
        node = node.next_functions[0][0] if len(node.next_functions) == 1 else None
    return leaf if leaf is not None and leaf.shape == t.shape and leaf.dtype == torch.float32 else None


def _match_getters(means3D, opacities, shs, scales, rotations):
    """(xyz, f_dc, f_rest, opacity, scaling, rotation) leaves when the arguments are the reference getters' outputs."""
    try:
        if not (means3D.is_leaf and means3D.dtype == torch.float32 and means3D.is_cuda):
            return None
        op, sc, rot = _unary_getter(opacities, "SigmoidBackward0"), _unary_getter(scales, "ExpBackward0"), _normalize_getter(rotations)
        fn = shs.grad_fn
        if op is None or sc is None or rot is None or fn is None or type(fn).__name__ != "CatBackward0":
            return None
        if int(fn._saved_dim) != 1 or len(fn.next_functions) != 2:
            return None
        dc, rest = _leaf_of(fn, 0), _leaf_of(fn, 1)
        P = means3D.shape[0]
        if dc is None or rest is None or tuple(dc.shape) != (P, 1, 3) or rest.dim() != 3 or rest.shape[0] != P or rest.shape[2] != 3:
            return None
        if dc.dtype != torch.float32 or rest.dtype != torch.float32 or rest.shape[1] + 1 != shs.shape[1] or rest.shape[1] == 0:
            return None
        return means3D, dc, rest, op, sc, rot
    except (AttributeError, RuntimeError, TypeError):
        return None


class GaussianRasterizer(nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings, depth_alpha: bool = False, antialiasing: bool = False,
                 absgrad: bool = False, contributions=None, pixel_error=None, median_depth: bool = False):
        """median_depth=True (extension; with depth_alpha=True): forward / forward_raw also return the median depth map [1,H,W] as a fifth
        output (module docstring); not with absgrad, contributions, tile_rows or extra_colors.
        contributions (a contrib.ContributionStats, extension): every frame is also added into it (module docstring); the frame has
        no backward; not with depth_alpha or absgrad.
        pixel_error (float32 [H,W] or [1,H,W], extension; with a contrib.ErrorStats as contributions): every frame also adds its
        error-weighted totals and folds them into the running sum and maximum (module docstring).
        absgrad=True (gsplat's flag): backward() also assigns means2D.absgrad [P,3] (module docstring); not with depth_alpha.
        depth_alpha=True (extension): forward / forward_raw also return the depth and alpha maps [1,H,W] (module docstring).
        antialiasing=True (upstream's flag): the opacities are compensated for the 0.3 px^2 dilation first (module docstring)."""
        super().__init__()
        self.raster_settings = raster_settings
        self.depth_alpha = bool(depth_alpha)
        self.antialiasing = bool(antialiasing)
        self.absgrad = bool(absgrad)
        self.median_depth = bool(median_depth)
        if self.median_depth:
            check_median_depth(self.depth_alpha, self.absgrad, contributions)
        if self.absgrad and self.depth_alpha:
            raise ValueError(_ABSGRAD_NO_AUX)
        self.contributions = contributions
        if contributions is not None:
            from .contrib import ContributionStats
            if not isinstance(contributions, ContributionStats):
                raise ValueError(f"contributions must be a ContributionStats, got {type(contributions).__name__}")
            if self.depth_alpha or self.absgrad:
                raise ValueError(_CONTRIB_PLAIN_ONLY)
        self.pixel_error = pixel_error
        if pixel_error is not None:
            from .contrib import check_error_stats
            check_error_stats(contributions, "GaussianRasterizer")

    def _checked_error_map(self, rs, device, what):
        """The frame's error map, checked against the frame (None without one): once per frame, before anything runs."""
        if self.pixel_error is None:
            return None
        from .contrib import check_pixel_error
        return check_pixel_error(self.contributions, self.pixel_error, int(rs.image_height), int(rs.image_width), device, what)

    def _contrib_frame(self, error_map, *args, **kw):
        """A statistics frame (its inputs and its error map checked by the caller): the native forward itself - no autograd node,
        nothing can follow it - and the plain call's (color, radii)."""
        with torch.no_grad():
            color, radii, _ = rasterize_forward(*args, contrib=self.contributions, pixel_error=error_map, pixel_error_checked=True, **kw)
            if self.raster_settings.debug:
                torch.cuda.synchronize(radii.device)
        return color, radii

    def _aux_arg(self):
        """The autograd functions' `aux` argument of this rasterizer's frames."""
        return _AUX_MEDIAN if self.median_depth else self.depth_alpha

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum test per point (the reference's `_C.mark_visible`; unused in-tree, kept for API parity)."""
        rs = self.raster_settings
        with torch.no_grad():
            pos = _f32c(positions, positions.device)
            present = torch.zeros(positions.shape[0], dtype=torch.uint8, device=positions.device)
            if pos is not None:
                vm, pm = _f32c(rs.viewmatrix, positions.device), _f32c(rs.projmatrix, positions.device)
                with torch.cuda.device(positions.device):
                    N.mark_visible(pos, vm, pm, present)
        return present.bool()

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None, rotations=None,
                cov3D_precomp=None, extra_colors=None):
        """extra_colors (extension; [P,3] float32, with depth_alpha=True): three more channels blended in this frame; the call then
        returns (color, radii, depth, alpha, extra [3,H,W]) (module docstring)."""
        rs = self.raster_settings
        if self.median_depth:                    # (before anything runs: a refused call has launched nothing)
            check_median_depth(self.depth_alpha, self.absgrad, self.contributions, extra_colors=extra_colors)
        if extra_colors is not None:             # (before anything runs: a refused call has launched nothing)
            check_extra_colors(extra_colors, means3D, self.depth_alpha, self.absgrad, self.contributions, rs=rs)
        if self.contributions is not None:       # (before anything runs: a refused call has launched nothing)
            from .contrib import check_inputs
            check_inputs(self.contributions, (means3D, means2D, opacities, shs, colors_precomp, scales, rotations, cov3D_precomp,
                                              rs.viewmatrix, rs.projmatrix, rs.campos), "GaussianRasterizer.forward")
            error_map = self._checked_error_map(rs, means3D.device, "GaussianRasterizer.forward")
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception("Please provide excatly one of either SHs or precomputed colors!")
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception("Please provide exactly one of either scale/rotation pair or precomputed 3D covariance!")
        if self.antialiasing:
            if cov3D_precomp is not None:
                raise ValueError("antialiasing needs scales and rotations: the opacity compensation's gradient goes to them, not to a "
                                 "precomputed 3D covariance")
            from .antialias import compensate_opacity
            opacities = compensate_opacity(opacities, means3D, scales, rotations, rs)
        empty = torch.empty(0, dtype=torch.float32, device=means3D.device)
        shs = empty if shs is None else shs
        colors_precomp = empty if colors_precomp is None else colors_precomp
        scales = empty if scales is None else scales
        rotations = empty if rotations is None else rotations
        cov3D_precomp = empty if cov3D_precomp is None else cov3D_precomp
        rs = rs._replace(sh_degree=int(rs.sh_degree), image_height=int(rs.image_height),
                         image_width=int(rs.image_width))
        if self.contributions is not None:
            return self._contrib_frame(error_map, means3D, shs, colors_precomp, opacities, scales, rotations,
                                       cov3D_precomp, rs)
        if FUSE_GETTERS and torch.is_grad_enabled() and not rs.debug and shs.numel() and scales.numel() and rotations.numel():
            leaves = _match_getters(means3D, opacities, shs, scales, rotations)
            if leaves is not None:
                xyz, dc, rest, op, sc, rot = leaves
                if extra_colors is not None:
                    return _apply(_RasterizeGaussiansRaw, xyz, means2D, dc, rest, op, sc, rot, rs, True, *_extra_args(extra_colors))
                return _apply(_RasterizeGaussiansRaw, xyz, means2D, dc, rest, op, sc, rot, rs, self._aux_arg(), *_camera_args(rs),
                              absgrad_to=means2D if self.absgrad else None)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales, rotations,
                                   cov3D_precomp, rs, self.depth_alpha, self.absgrad, extra_colors, self.median_depth)

    def forward_raw(self, xyz, means2D, features_dc, features_rest, opacity_logits, log_scales, raw_rotations, extra_colors=None):
        """Extension (not in the reference API): render straight from the reference GaussianModel's raw parameters
        (`_xyz, _features_dc, _features_rest, _opacity, _scaling, _rotation`), activations fused into the kernels.
        Same pixels and radii as forward(get_xyz, ..., get_opacity, get_features, get_scaling, get_rotation) and the
        same gradients on the raw parameters as autograd through those getters, to fp32 rounding."""
        rs = self.raster_settings
        rs = rs._replace(sh_degree=int(rs.sh_degree), image_height=int(rs.image_height), image_width=int(rs.image_width))
        if self.median_depth:
            check_median_depth(self.depth_alpha, self.absgrad, self.contributions, extra_colors=extra_colors)
        if extra_colors is not None:             # (as forward: the same rules, the same fifth output)
            check_extra_colors(extra_colors, xyz, self.depth_alpha, self.absgrad, self.contributions, rs=rs)
        if self.contributions is not None:
            from .contrib import check_inputs
            check_inputs(self.contributions, (xyz, means2D, features_dc, features_rest, opacity_logits, log_scales, raw_rotations,
                                              rs.viewmatrix, rs.projmatrix, rs.campos), "GaussianRasterizer.forward_raw")
            error_map = self._checked_error_map(rs, xyz.device, "GaussianRasterizer.forward_raw")
        if self.antialiasing:
            from .antialias import compensate_opacity
            opacity_logits = compensate_opacity(opacity_logits, xyz, log_scales, raw_rotations, rs, raw=True)
        packed = features_rest is None and features_dc.dim() == 3 and features_dc.shape[1] > 1      # one [P,M,3] table
        if not packed and (features_rest is None or features_rest.numel() == 0):
            features_rest = torch.empty(0, dtype=torch.float32, device=xyz.device)
        if self.contributions is not None:
            return self._contrib_frame(error_map, xyz, features_dc, None, opacity_logits, log_scales, raw_rotations,
                                       None, rs, sh_rest=features_rest, raw=2 if features_rest is None else 1)
        if extra_colors is not None:
            return _apply(_RasterizeGaussiansRaw, xyz, means2D, features_dc, features_rest, opacity_logits, log_scales, raw_rotations, rs,
                          True, *_extra_args(extra_colors))
        return _apply(_RasterizeGaussiansRaw, xyz, means2D, features_dc, features_rest, opacity_logits, log_scales, raw_rotations, rs,
                      self._aux_arg(), *_camera_args(rs), absgrad_to=means2D if self.absgrad else None)
