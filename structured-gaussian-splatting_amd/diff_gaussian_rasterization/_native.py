"""ctypes binding of libgsrast.so (C ABI: include/gsrast.h).

There is NO fallback: if the HIP library is missing or a call fails, this module raises.  The product
path never imports the CPU oracle (oracle/ is test infrastructure).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
from typing import Optional

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LIB_PATH = os.environ.get("GSR_LIB_PATH") or os.path.join(_PKG_ROOT, "lib", "libgsrast.so")      # override: kernel-variant experiments
_CSRC = os.path.join(_PKG_ROOT, "csrc")
SCREEN_GRAD_STRIDE = 12

_f32p = C.c_void_p

MIRRORS = {}          # typedef of include/gsrast.h -> its ctypes mirror (tests/test_abi.py checks every layout against gcc's)


class _Mirror(C.Structure):
    """Base of the mirrors: `class X(_Mirror, c="gsr_x")` records the header typedef(s) X mirrors, as X.c_names and in MIRRORS."""
    def __init_subclass__(cls, c=(), **kw):
        super().__init_subclass__(**kw)
        cls.c_names = (c,) if isinstance(c, str) else tuple(c)
        MIRRORS.update((n, cls) for n in cls.c_names)


class FrameDesc(_Mirror, c="gsr_frame_desc"):
    _fields_ = [("P", C.c_int32), ("sh_degree", C.c_int32), ("sh_coeffs", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("tanfovx", C.c_float), ("tanfovy", C.c_float), ("scale_modifier", C.c_float),
                ("prefiltered", C.c_int32), ("debug", C.c_int32), ("tile_row_begin", C.c_int32),
                ("tile_row_end", C.c_int32)]


class Camera(_Mirror, c="gsr_camera"):
    _fields_ = [("bg", _f32p), ("viewmatrix", _f32p), ("projmatrix", _f32p), ("campos", _f32p)]


class Gaussians(_Mirror, c="gsr_gaussians"):
    _fields_ = [("means3D", _f32p), ("shs", _f32p), ("colors_precomp", _f32p), ("opacities", _f32p),
                ("scales", _f32p), ("rotations", _f32p), ("cov3D_precomp", _f32p),
                ("shs_rest", _f32p), ("raw", C.c_int32)]      # raw-parameter mode (a14): see include/gsrast.h


class Grads(_Mirror, c="gsr_grads"):
    _fields_ = [("means3D", _f32p), ("means2D", _f32p), ("shs", _f32p), ("colors_precomp", _f32p),
                ("opacities", _f32p), ("scales", _f32p), ("rotations", _f32p), ("cov3D_precomp", _f32p),
                ("shs_rest", _f32p), ("prezeroed", C.c_int32)]


class AuxOutputs(_Mirror, c="gsr_aux_outputs"):
    """gsr_aux_outputs: the depth and alpha maps [H,W] and their checkpoint workspace (gsr_aux_workspace_size)."""
    _fields_ = [("depth", _f32p), ("alpha", _f32p), ("ckpt_ws", C.c_void_p)]


class ContribStats(_Mirror, c="gsr_contrib_stats"):
    """gsr_contrib_stats: the per-Gaussian accumulators of the blend statistics, [P] each (count and weight_sum_q32 64-bit, weight_max_bits
    the bits of a float)."""
    _fields_ = [("count", C.c_void_p), ("weight_sum_q32", C.c_void_p), ("weight_max_bits", C.c_void_p)]


class ContribError(_Mirror, c="gsr_contrib_error"):
    """gsr_contrib_error: the per-pixel error map [H*W] (read only) and the frame's per-Gaussian error totals [P] (64-bit, units of 2^-32)."""
    _fields_ = [("pixel_error", _f32p), ("error_frame_q32", C.c_void_p)]


class CameraGrads(_Mirror, c="gsr_camera_grads"):
    """gsr_camera_grads: dL/dviewmatrix [16], dL/dprojmatrix [16], dL/dcampos [3]; any may be NULL."""
    _fields_ = [("viewmatrix", _f32p), ("projmatrix", _f32p), ("campos", _f32p)]


class StructuredDesc(_Mirror, c="gsr_structured_desc"):
    """gsr_structured_desc: B structures of K children with sh_coeffs SH coefficients per channel each."""
    _fields_ = [("B", C.c_int32), ("K", C.c_int32), ("sh_coeffs", C.c_int32)]


class Structures(_Mirror, c="gsr_structures"):
    """gsr_structures: means [B,3], opacities [B], scales [B,3], rotations [B,4]."""
    _fields_ = [("means", _f32p), ("opacities", _f32p), ("scales", _f32p), ("rotations", _f32p)]


class Children(_Mirror, c=("gsr_children", "gsr_children_grads")):
    """gsr_children (the composed tensors) and gsr_children_grads (their incoming gradients, NULL = zero): one layout."""
    _fields_ = [("xyz", _f32p), ("opacity", _f32p), ("scaling", _f32p), ("rotation", _f32p), ("features", _f32p)]


ChildrenGrads = Children


class StructuredGrads(_Mirror, c="gsr_structured_grads"):
    """gsr_structured_grads: dL/ddecoded [B, K D] and the structure gradients; NULL = not wanted."""
    _fields_ = [("decoded", _f32p), ("means", _f32p), ("opacities", _f32p), ("scales", _f32p), ("rotations", _f32p)]


class DecoderDesc(_Mirror, c="gsr_decoder_desc"):
    """gsr_decoder_desc: B structures, an input row of in_size = positional dims + latent_size floats, out_size outputs."""
    _fields_ = [("B", C.c_int32), ("in_size", C.c_int32), ("latent_size", C.c_int32), ("hidden_size", C.c_int32),
                ("out_size", C.c_int32)]


class DecoderParams(_Mirror, c="gsr_decoder_params"):
    """gsr_decoder_params: nn.Linear layouts, w [out, in]."""
    _fields_ = [("w0", _f32p), ("b0", _f32p), ("w1", _f32p), ("b1", _f32p), ("w2", _f32p), ("b2", _f32p)]


class DecoderGrads(_Mirror, c="gsr_decoder_grads"):
    """gsr_decoder_grads: NULL = not wanted."""
    _fields_ = [("latents", _f32p), ("w0", _f32p), ("b0", _f32p), ("w1", _f32p), ("b1", _f32p), ("w2", _f32p), ("b2", _f32p)]


# constants of the header, mirrored by hand (tests/test_abi.py compares them with its #defines and enum)
MAX_CHUNKS = 8
LAST_SHIFT = 26
ERR_WORKSPACE = -4
ADAM_MAX_TENSORS = 8
ADAM_STEP_UNCORRECTED = 2 ** 63 - 1        # GSR_ADAM_STEP_UNCORRECTED: a `step` that applies no bias correction
MCMC_MAX_TENSORS = 8
MCMC_ROLES = {"copy": 0, "opacity": 1, "scaling": 2}
PROFILE_NAME_LEN = 32


class FramePlan(_Mirror, c="gsr_frame_plan"):
    _fields_ = [("num_rendered", C.c_int64), ("num_visible", C.c_int32), ("num_chunks", C.c_int32),
                ("chunk_rank_begin", C.c_int32 * (MAX_CHUNKS + 1)), ("chunk_instances_max", C.c_int64 * MAX_CHUNKS),
                ("chunks_run", C.c_int32), ("sort_result", C.c_int32), ("instances_emitted", C.c_int64),
                ("binning_initialised", C.c_int32), ("screen_prezeroed", C.c_int32), ("binning_capacity", C.c_int64),
                ("chunk_key_end", C.c_uint32 * MAX_CHUNKS), ("chunks_sorted", C.c_int32), ("chunks_filtered", C.c_int32),
                ("tile_order_ready", C.c_int32), ("key_max", C.c_uint32)]


class DebugViews(_Mirror, c="gsr_debug_views"):
    _fields_ = [("splat_records", C.c_void_p), ("tiles_touched", C.c_void_p), ("depth_order", C.c_void_p),
                ("point_offsets", C.c_void_p), ("clamped", C.c_void_p), ("sorted_gaussian", C.c_void_p),
                ("ranges", C.c_void_p), ("final_T", C.c_void_p), ("n_contrib", C.c_void_p), ("tile_walk", C.c_void_p),
                ("bwd_units", C.c_void_p), ("bwd_unit_count", C.c_void_p), ("bwd_unit_cap_full", C.c_uint32), ("bwd_unit_cap_part", C.c_uint32)]


class AdamTensor(_Mirror, c="gsr_adam_tensor"):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("lr", C.c_float), ("lr_tail", C.c_float), ("step", C.c_int64), ("row_len", C.c_int32), ("split", C.c_int32)]


class McmcTensor(_Mirror, c="gsr_mcmc_tensor"):
    """gsr_mcmc_tensor: a [P, width] tensor, its Adam moments (both or neither None) and its role."""
    _fields_ = [("param", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("width", C.c_int32), ("role", C.c_int32)]


# ---- The C ABI's signatures, once: every function include/gsrast.h declares -> (restype, argtypes in header order).  load() applies
# them, so a wrong arity or a mirror of the wrong struct is a TypeError / ArgumentError; tests/test_abi.py holds the table to the
# header's prototypes.  A struct parameter is POINTER(its mirror) and takes the instance bare (or None); a host out-parameter is
# POINTER(scalar) and takes the scalar object bare; _dev is everything else behind a pointer (device memory, the stream, the host
# arrays of gsr_profile_read) and takes a plain int address, a ctypes object or None.
_int, _i32, _i64, _u32, _f32, _size, _dev, _P = C.c_int, C.c_int32, C.c_int64, C.c_uint32, C.c_float, C.c_size_t, C.c_void_p, C.POINTER
_desc, _cam, _gs, _plan, _grads, _aux = _P(FrameDesc), _P(Camera), _P(Gaussians), _P(FramePlan), _P(Grads), _P(AuxOutputs)
_stats, _err = _P(ContribStats), _P(ContribError)
_forward = (_desc, _cam, _gs, _dev, _dev, _dev, _plan, _dev, _i64, _dev, _grads)          # gsr_forward's arguments in front of the stream
_forward_render = (_desc, _cam, _gs, _dev, _dev, _dev, _plan, _dev)                       # gsr_forward_render's
_backward_render = (_desc, _cam, _dev, _dev, _dev, _dev, _plan, _dev)                     # gsr_backward_render's, up to out_color
_backward_geom = (_desc, _cam, _gs, _dev, _dev, _dev, _i32, _i32, _i32, _plan, _grads, _dev)
SIGNATURES = {
    "gsr_version": (_int, ()),
    "gsr_last_error": (C.c_char_p, ()),
    "gsr_workspace_sizes": (_int, (_desc, _P(_size), _P(_size))),
    "gsr_binning_size": (_int, (_desc, _i64, _P(_size))),
    "gsr_binning_first_chunk_capacity": (_int, (_plan, _P(_i64))),
    "gsr_forward_preprocess": (_int, (_desc, _cam, _gs, _dev, _dev, _dev, _plan, _dev)),
    "gsr_forward_render": (_int, _forward_render + (_dev,)),
    "gsr_forward": (_int, _forward + (_dev,)),
    "gsr_backward_rows_size": (_int, (_desc, _plan, _P(_size))),
    "gsr_backward_prepare": (_int, (_desc, _gs, _plan, _dev, _grads, _dev)),
    "gsr_backward_render": (_int, _backward_render + (_dev, _dev, _dev)),
    "gsr_bwd_segment_entries": (_int, ()),
    "gsr_backward_geom": (_int, _backward_geom),
    "gsr_backward_geom_rows": (_int, (_desc, _cam, _gs, _dev, _dev, _dev, _dev, _i32, _grads, _dev)),
    "gsr_aux_workspace_size": (_int, (_desc, _i64, _P(_size))),
    "gsr_forward_render_aux": (_int, _forward_render + (_aux, _dev)),
    "gsr_forward_aux": (_int, _forward + (_aux, _dev)),
    "gsr_backward_render_aux": (_int, _backward_render + (_aux, _dev, _dev, _dev, _dev, _dev)),
    "gsr_backward_geom_aux": (_int, _backward_geom),
    "gsr_forward_render_contrib": (_int, _forward_render + (_stats, _dev)),
    "gsr_forward_contrib": (_int, _forward + (_stats, _dev)),
    "gsr_forward_render_contrib_error": (_int, _forward_render + (_stats, _err, _dev)),
    "gsr_forward_contrib_error": (_int, _forward + (_stats, _err, _dev)),
    "gsr_contrib_error_fold": (_int, (_i64, _dev, _dev, _dev, _dev)),
    "gsr_camera_grad_workspace_size": (_int, (_desc, _P(_size))),
    "gsr_backward_camera": (_int, (_desc, _cam, _gs, _dev, _dev, _dev, _i32, _plan, _i32, _dev, _P(CameraGrads), _dev)),
    "gsr_backward_render_abs": (_int, _backward_render + (_dev, _dev, _dev)),
    "gsr_screen_absgrad": (_int, (_desc, _dev, _dev, _dev, _i32, _plan, _dev, _dev)),
    "gsr_frame_arrays": (_int, (_desc, _dev, _P(_dev), _P(_dev))),
    "gsr_exchange_rows_gather": (_int, (_desc, _dev, _u32, _dev, _i32, _dev, _dev, _dev)),
    "gsr_exchange_rows_scatter": (_int, (_desc, _i32, _dev, _dev, _dev, _dev)),
    "gsr_mark_visible": (_int, (_i32, _dev, _dev, _dev, _dev, _dev)),
    "gsr_debug_get_views": (_int, (_desc, _dev, _dev, _dev, _plan, _P(DebugViews))),
    "gsr_loss_workspace_size": (_int, (_i32, _i32, _i32, _P(_size))),
    "gsr_loss_l1_ssim_forward": (_int, (_i32, _i32, _i32, _f32, _dev, _dev, _dev, _dev, _dev)),
    "gsr_loss_l1_ssim_backward": (_int, (_i32, _i32, _i32, _f32, _dev, _dev, _dev, _dev, _dev, _dev)),
    "gsr_loss_l1_backward": (_int, (_i64, _dev, _dev, _dev, _dev, _dev)),
    "gsr_loss_l1_ssim_forward_rows": (_int, (_i32, _i32, _i32, _dev, _dev, _dev, _dev, _i32, _i32, _dev)),
    "gsr_loss_l1_ssim_backward_rows": (_int, (_i32, _i32, _i32, _f32, _dev, _dev, _dev, _dev, _dev, _i32, _i32, _dev)),
    "gsr_dist2_workspace_size": (_int, (_i32, _P(_size))),
    "gsr_dist2_knn3": (_int, (_i32, _dev, _dev, _dev, _dev)),
    "gsr_adam_step": (_int, (_i64, _dev, _dev, _dev, _dev, _f32, _f32, _f32, _f32, _i64, _dev)),
    "gsr_adam_step_split": (_int, (_i64, _i32, _i32, _dev, _dev, _dev, _dev, _f32, _f32, _f32, _f32, _f32, _i64, _dev)),
    "gsr_adam_step_multi": (_int, (_i32, _P(AdamTensor), _f32, _f32, _f32, _dev)),
    "gsr_adam_step_sparse_multi": (_int, (_i32, _P(AdamTensor), _i64, _dev, _i32, _f32, _f32, _f32, _dev)),
    "gsr_activations_forward": (_int, (_i64,) + (_dev,) * 7),
    "gsr_activations_backward": (_int, (_i64,) + (_dev,) * 10),
    "gsr_structured_compose_forward": (_int, (_P(StructuredDesc), _dev, _P(Structures), _P(Children), _dev)),
    "gsr_structured_compose_backward": (_int, (_P(StructuredDesc), _dev, _P(Structures), _P(ChildrenGrads), _P(StructuredGrads), _dev)),
    "gsr_opacity_compensation_forward": (_int, (_desc, _cam, _gs, _dev, _dev)),
    "gsr_opacity_compensation_backward": (_int, (_desc, _cam, _gs, _dev, _grads, _dev)),
    "gsr_decoder_workspace_size": (_int, (_P(DecoderDesc), _P(_size))),
    "gsr_decoder_forward": (_int, (_P(DecoderDesc), _dev, _dev, _P(DecoderParams), _dev, _dev)),
    "gsr_decoder_backward": (_int, (_P(DecoderDesc), _dev, _dev, _P(DecoderParams), _dev, _P(DecoderGrads), _dev, _size, _dev)),
    "gsr_mcmc_relocation_workspace_size": (_int, (_i64, _P(_size))),
    "gsr_mcmc_relocation": (_int, (_i64, _i64, _dev, _dev, _dev, _f32, _dev, _dev, _dev, _dev)),
    "gsr_mcmc_relocate_rows": (_int, (_i32, _P(McmcTensor), _i64, _i64, _dev, _dev, _dev, _dev, _dev)),
    "gsr_mcmc_inject_noise": (_int, (_i64, _dev, _dev, _dev, _dev, _dev, _f32, _dev)),
    "gsr_mcmc_reg_grads": (_int, (_i64, _dev, _dev, _f32, _f32, _dev, _dev, _dev)),
    "gsr_bilagrid_workspace_size": (_int, (_i32, _i32, _i32, _i32, _i32, _P(_size), _P(_size))),
    "gsr_bilagrid_forward": (_int, (_i32,) * 7 + (_dev,) * 4),
    "gsr_bilagrid_backward": (_int, (_i32,) * 7 + (_dev,) * 6 + (_size, _dev)),
    "gsr_bilagrid_tv_forward": (_int, (_i32, _i32, _i32, _i32, _dev, _dev, _dev, _dev)),
    "gsr_bilagrid_tv_backward": (_int, (_i32, _i32, _i32, _i32, _dev, _dev, _dev, _dev)),
    "gsr_vq_workspace_size": (_int, (_i64, _i32, _i32, _P(_size))),
    "gsr_vq_assign": (_int, (_i64, _i32, _i32, _dev, _dev, _dev, _dev, _dev, _size, _dev)),
    "gsr_vq_update": (_int, (_i64, _i32, _i32, _dev, _dev, _dev, _dev, _dev, _dev, _size, _dev)),
    "gsr_filter3d_workspace_size": (_int, (_i64, _P(_size))),
    "gsr_filter3d_compute": (_int, (_i64, _i32, _dev, _f32, _dev, _dev, _dev, _size, _P(_i32), _dev)),
    "gsr_filter3d_apply_forward": (_int, (_i64, _i32, _dev, _dev, _dev, _dev, _dev, _dev)),
    "gsr_filter3d_apply_backward": (_int, (_i64, _i32) + (_dev,) * 8),
    "gsr_densify_stats": (_int, (_i32, _dev, _dev, _dev, _dev, _dev, _dev)),
    "gsr_debug_sort_temp_bytes": (_int, (_P(_size),)),
    "gsr_debug_sort_pairs": (_int, (_dev, _dev, _dev, _dev, _i64, _i32, _i32, _dev, _P(_i32), _dev)),
    "gsr_debug_sort_pairs_ex": (_int, (_dev,) * 6 + (_i64, _i64, _i64, _i32, _i32, _dev, _P(_i32), _dev)),
    "gsr_profile_enable": (_int, (_int,)),
    "gsr_profile_read": (_int, (_int, _dev, _dev, _dev)),
}
EXPORTS = tuple(SIGNATURES)

# The normal-map entry points, declared in include/gsrast_normals.h (which gsrast.h includes): the same rules, a table per header, so
# that each table is held to the prototypes of its own file (tests/test_abi.py, tests/test_normals_ref.py).
_image = (_i32, _i32, _f32, _f32, _f32)                                                    # H, W, tanfovx, tanfovy, alpha_min
NORMALS_SIGNATURES = {
    "gsr_gaussian_normals_forward": (_int, (_i64,) + (_dev,) * 7),
    "gsr_gaussian_normals_backward": (_int, (_i64,) + (_dev,) * 8),
    "gsr_depth_normal_forward": (_int, _image + (_dev,) * 4),
    "gsr_depth_normal_backward": (_int, _image + (_dev,) * 6),
    "gsr_normal_consistency_workspace_size": (_int, (_i32, _i32, _P(_size))),
    "gsr_normal_consistency_forward": (_int, _image + (_dev,) * 4 + (_size, _dev, _dev)),
    "gsr_normal_consistency_backward": (_int, _image + (_dev,) * 8),
}
# The extra-channel entry points, declared in include/gsrast_extra.h (which gsrast.h includes): a table of their own, held to that
# header's prototypes by tests/test_extra_abi.py.  They take no struct of their own (the aux frame's gsr_aux_outputs and plain pointers).
EXTRA_SIGNATURES = {
    "gsr_extra_workspace_size": (_int, (_desc, _i64, _P(_size))),
    "gsr_extra_rows_size": (_int, (_desc, _plan, _P(_size))),
    "gsr_forward_render_extra": (_int, _forward_render + (_aux, _dev, _dev, _dev)),
    "gsr_forward_extra": (_int, _forward + (_aux, _dev, _dev, _dev)),
    "gsr_backward_render_extra": (_int, _backward_render + (_aux,) + (_dev,) * 10),
}
# The median-depth entry points, declared in include/gsrast_median.h (which gsrast.h includes): a table of their own, held to that
# header's prototypes by tests/test_median_abi.py.  The aux frame's gsr_aux_outputs and plain pointers.
MEDIAN_SIGNATURES = {
    "gsr_forward_render_median": (_int, _forward_render + (_aux, _dev, _dev, _dev)),
    "gsr_forward_median": (_int, _forward + (_aux, _dev, _dev, _dev)),
    "gsr_backward_render_median": (_int, _backward_render + (_aux,) + (_dev,) * 7),
}
# TSDF fusion and mesh extraction, declared in include/gsrast_tsdf.h (which gsrast.h includes): held to that header's prototypes by
# tests/test_tsdf_ref.py.  No struct of their own; the two totals of gsr_tsdf_mesh_count are host out-parameters.
_dims = (_i32, _i32, _i32)                                                                 # nx, ny, nz
TSDF_SIGNATURES = {
    "gsr_tsdf_integrate": (_int, _dims + (_f32,) * 5 + (_i32, _i32) + (_f32,) * 4 + (_dev,) * 8),
    "gsr_tsdf_mesh_workspace_size": (_int, _dims + (_P(_size),)),
    "gsr_tsdf_mesh_count": (_int, _dims + (_f32, _dev, _dev, _dev, _size, _P(_i64), _P(_i64), _dev)),
    "gsr_tsdf_mesh_emit": (_int, _dims + (_f32,) * 5 + (_dev,) * 4 + (_size, _i64, _i64) + (_dev,) * 4),
}
# Mesh cleaning, declared in include/gsrast_mesh.h (which gsrast.h includes): held to that header's prototypes by
# tests/test_mesh_clean_ref.py.  No struct of their own; the two totals of gsr_mesh_clean_count are host out-parameters.
MESH_SIGNATURES = {
    "gsr_mesh_clean_workspace_size": (_int, (_i32, _i32, _P(_size))),
    "gsr_mesh_components": (_int, (_i32, _i32, _dev, _dev, _dev, _dev, _size, _dev)),
    "gsr_mesh_clean_count": (_int, (_i32, _i32) + (_dev,) * 5 + (_size, _P(_i64), _P(_i64), _dev)),
    "gsr_mesh_clean_emit": (_int, (_i32, _i32, _dev, _dev, _size, _i64, _i64) + (_dev,) * 4),
}
# The depth-distortion loss, declared in include/gsrast_distortion.h (which gsrast.h includes): held to that header's prototypes by
# tests/test_distortion_ref.py.  No struct of their own.
_moments = (_i64, _dev, _dev, _i32, _f32, _f32)                                            # P, means3D, viewmatrix, mapping, near, far
DISTORTION_MAPPINGS = {"ndc": 0, "linear": 1}                                              # GSR_DISTORTION_NDC, GSR_DISTORTION_LINEAR
DISTORTION_SIGNATURES = {
    "gsr_depth_moments_forward": (_int, _moments + (_dev, _dev)),
    "gsr_depth_moments_backward": (_int, _moments + (_dev, _dev, _dev)),
    "gsr_distortion_map_forward": (_int, (_i32, _i32) + (_dev,) * 4),
    "gsr_distortion_map_backward": (_int, (_i32, _i32) + (_dev,) * 6),
    "gsr_distortion_loss_workspace_size": (_int, (_i32, _i32, _P(_size))),
    "gsr_distortion_loss_forward": (_int, (_i32, _i32, _dev, _dev, _dev, _size, _dev, _dev)),
    "gsr_distortion_loss_backward": (_int, (_i32, _i32) + (_dev,) * 6),
}
# The sparse TSDF volume, declared in include/gsrast_tsdf_sparse.h (which gsrast.h includes): held to that header's prototypes by
# tests/test_tsdf_sparse_ref.py.  No struct of their own; the counts of the two count calls are host out-parameters.
_bricks = (_dev,) * 4                                                                      # brick_table, brick_coords, brick_order, brick_rank
TSDF_SPARSE_SIGNATURES = {
    "gsr_tsdf_sparse_allocate": (_int, _dims + (_f32,) * 6 + (_i32, _i32) + (_f32,) * 4 + (_dev,) * 5),
    "gsr_tsdf_sparse_commit_workspace_size": (_int, _dims + (_P(_size),)),
    "gsr_tsdf_sparse_commit_count": (_int, _dims + (_dev, _dev, _dev, _size, _P(_i64), _dev)),
    "gsr_tsdf_sparse_commit_assign": (_int, _dims + (_i64, _i64, _dev, _dev, _dev, _size, _dev, _dev, _dev, _dev)),
    "gsr_tsdf_sparse_integrate": (_int, _dims + (_f32,) * 5 + (_i32, _i32) + (_f32,) * 4 + (_i64,) + (_dev,) * 9),
    "gsr_tsdf_sparse_mesh_workspace_size": (_int, (_i64, _P(_size))),
    "gsr_tsdf_sparse_mesh_count": (_int, _dims + (_i64, _f32, _dev, _dev) + _bricks + (_dev, _size, _P(_i64), _P(_i64), _dev)),
    "gsr_tsdf_sparse_mesh_emit": (_int, _dims + (_f32,) * 4 + (_i64, _f32, _dev, _dev, _dev) + _bricks + (_dev, _size, _i64, _i64) + (_dev,) * 5),
}
_ALL_SIGNATURES = {**SIGNATURES, **NORMALS_SIGNATURES, **EXTRA_SIGNATURES, **MEDIAN_SIGNATURES, **TSDF_SIGNATURES, **MESH_SIGNATURES,
                   **DISTORTION_SIGNATURES, **TSDF_SPARSE_SIGNATURES}

_lib = None


def lib_path() -> str:
    return _LIB_PATH


def build(force: bool = False) -> str:
    """Compile libgsrast.so for gfx950 with hipcc (csrc/Makefile).  Cross-compiles without a GPU."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", _CSRC, "-j4"], stdout=subprocess.DEVNULL)
    return _LIB_PATH


def load():
    """The CDLL with SIGNATURES applied: its functions return the status (or value) as it is."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(
                f"libgsrast.so not found at {_LIB_PATH}: the HIP extension is required (no CPU fallback exists). "
                f"Build it with `make -C {_CSRC}` or `python -c 'import __graft_entry__ as g; g.build()'`.")
        lib = C.CDLL(_LIB_PATH)
        for name, (restype, argtypes) in _ALL_SIGNATURES.items():
            if not hasattr(lib, name):
                raise RuntimeError(f"libgsrast.so does not export {name}")
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


class GsrError(RuntimeError):
    status = 0


def _errcheck(rc, fn, args=None):
    """ctypes' errcheck of the checked functions: a non-zero status raises GsrError under the function's own name."""
    if rc != 0:
        e = GsrError(f"{fn.__name__} failed (status {rc}): {load().gsr_last_error().decode('utf-8', 'replace')}")
        e.status = rc
        raise e
    return rc


class _Checked:
    """_gsr.gsr_x(...): the typed gsr_x of load() that raises GsrError on a non-zero status (only for the functions that return one:
    gsr_version, gsr_last_error, gsr_bwd_segment_entries and gsr_profile_read return a value and are called through load())."""

    def __getattr__(self, name):                  # once per name: the function then sits in the instance's __dict__
        if name not in _ALL_SIGNATURES:
            raise AttributeError(name)
        fn = load()[name]                         # a function object of its own: load()'s keep returning the status
        fn.restype, fn.argtypes = _ALL_SIGNATURES[name]
        fn.errcheck = _errcheck
        self.__dict__[name] = fn
        return fn


_gsr = _Checked()


def _size(fn, *args) -> int:
    """A size query: fn(*args, size_t *bytes) -> bytes."""
    b = C.c_size_t()
    fn(*args, b)
    return b.value


def _size2(fn, *args):
    """A size query with two results: fn(*args, size_t *a, size_t *b) -> (a, b).  (Apart from _size: a general one costs 0.5 us a call.)"""
    a, b = C.c_size_t(), C.c_size_t()
    fn(*args, a, b)
    return a.value, b.value


def _ptr(t: Optional[torch.Tensor]):
    if t is None or t.numel() == 0:
        return None
    return t.data_ptr()


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def make_desc(P, sh_degree, sh_coeffs, width, height, tanfovx, tanfovy, scale_modifier, prefiltered, debug,
              tile_rows=None) -> FrameDesc:
    ty0, ty1 = (0, 0) if tile_rows is None else (int(tile_rows[0]), int(tile_rows[1]))
    return FrameDesc(int(P), int(sh_degree), int(sh_coeffs), int(width), int(height), float(tanfovx), float(tanfovy),
                     float(scale_modifier), int(bool(prefiltered)), int(bool(debug)), ty0, ty1)


def workspace_sizes(desc: FrameDesc):
    return _size2(_gsr.gsr_workspace_sizes, desc)


def binning_size(desc: FrameDesc, R: int) -> int:
    return _size(_gsr.gsr_binning_size, desc, R)


def binning_first_chunk_capacity(plan: FramePlan) -> int:
    n = C.c_int64(0)
    _gsr.gsr_binning_first_chunk_capacity(plan, n)
    return n.value


def forward_preprocess(desc, cam: Camera, g: Gaussians, geom_ws, radii, device, image_ws=None) -> FramePlan:
    plan = FramePlan()
    _gsr.gsr_forward_preprocess(desc, cam, g, _ptr(geom_ws), _ptr(image_ws), _ptr(radii), plan, _stream(device))
    return plan


def _variant(who: str, aux, contrib, err, extra=None, median=None):
    """(i, more) of a frame's variant: i picks among a wrapper's (plain, _aux, _contrib, _contrib_error, _extra, _median) entry points,
    `more` are the arguments that one takes in front of the stream.  extra: (table [P,4], map [3,H,W]) of an extra frame, which is an
    aux frame.  median: (median [H,W] float32, median_enc [H,W] int32) of a median frame, which is an aux frame without extra."""
    if median is not None:
        if aux is None or contrib is not None or err is not None or extra is not None:
            raise ValueError(f"{who}: the median depth rides on the aux frame (aux required, no extra / contrib / err)")
        return 5, (aux, _ptr(median[0]), _ptr(median[1]))
    if extra is not None:
        if aux is None or contrib is not None or err is not None:
            raise ValueError(f"{who}: extra channels ride on the aux frame (aux required, no contrib / err)")
        return 4, (aux, _ptr(extra[0]), _ptr(extra[1]))
    if aux is not None and contrib is not None:
        raise ValueError(f"{who}: aux and contrib together (that kernel is not built)")
    if err is not None and contrib is None:
        raise ValueError(f"{who}: err without contrib")
    if contrib is not None:
        return (2, (contrib,)) if err is None else (3, (contrib, err))
    return (0, ()) if aux is None else (1, (aux,))


def forward_both(desc, cam: Camera, g: Gaussians, geom_ws, image_ws, radii, binning_ws, binning_capacity, out_color, device,
                 early_fill: Optional[Grads] = None, aux: Optional[AuxOutputs] = None, contrib: Optional[ContribStats] = None,
                 err: Optional[ContribError] = None, extra=None, median=None):
    """gsr_forward (gsr_forward_median with `aux` and `median`; gsr_forward_extra with `aux` and `extra`; gsr_forward_aux with `aux`, gsr_forward_contrib with `contrib`; not both; gsr_forward_contrib_error with `contrib`
    and `err`): both stages in one call.  Returns
    (plan, done): done = False when the binning workspace was too small for the first chunk (nothing of stage 2 ran: allocate and
    call forward_render) - or, when the plan has more than one chunk, for a later one: a statistics frame has then already added
    its earlier chunks (include/gsrast.h), so its caller sizes the workspace for num_rendered."""
    plan = FramePlan()
    lib = load()                      # the plain functions: GSR_ERR_WORKSPACE is an answer here, not an error
    i, more = _variant("forward_both", aux, contrib, err, extra, median)
    fn = (lib.gsr_forward, lib.gsr_forward_aux, lib.gsr_forward_contrib, lib.gsr_forward_contrib_error, lib.gsr_forward_extra,
          lib.gsr_forward_median)[i]
    rc = fn(desc, cam, g, _ptr(geom_ws), _ptr(image_ws), _ptr(radii), plan, _ptr(binning_ws), int(binning_capacity), _ptr(out_color),
            early_fill, *more, _stream(device))
    if rc == ERR_WORKSPACE:           # the guessed workspace did not do (for the first chunk, or for a later one)
        return plan, False
    _errcheck(rc, fn)
    return plan, True


def forward_render(desc, cam: Camera, g: Gaussians, geom_ws, binning_ws, image_ws, plan: FramePlan, out_color, device,
                   aux: Optional[AuxOutputs] = None, contrib: Optional[ContribStats] = None, err: Optional[ContribError] = None,
                   extra=None, median=None):
    i, more = _variant("forward_render", aux, contrib, err, extra, median)
    fn = (_gsr.gsr_forward_render, _gsr.gsr_forward_render_aux, _gsr.gsr_forward_render_contrib, _gsr.gsr_forward_render_contrib_error,
          _gsr.gsr_forward_render_extra, _gsr.gsr_forward_render_median)[i]
    fn(desc, cam, g, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), plan, _ptr(out_color), *more, _stream(device))


def contrib_error_fold(error_frame_q32, error_sum_q32, error_max, device):
    """gsr_contrib_error_fold on the device's current stream: the frame's error totals into the running sum and maximum, then cleared."""
    _gsr.gsr_contrib_error_fold(int(error_frame_q32.shape[0]), _ptr(error_frame_q32), _ptr(error_sum_q32), _ptr(error_max), _stream(device))


def aux_workspace_size(desc: FrameDesc, binning_capacity: int) -> int:
    """gsr_aux_workspace_size: bytes of the depth checkpoints of an aux frame whose binning workspace holds that many instances."""
    return _size(_gsr.gsr_aux_workspace_size, desc, int(binning_capacity))


def extra_workspace_size(desc: FrameDesc, binning_capacity: int) -> int:
    """gsr_extra_workspace_size: bytes of the four-plane aux checkpoints of an extra frame (its gsr_aux_outputs.ckpt_ws)."""
    return _size(_gsr.gsr_extra_workspace_size, desc, int(binning_capacity))


def extra_rows_size(desc: FrameDesc, plan: FramePlan) -> int:
    """gsr_extra_rows_size: bytes of the extra backward's second row plane."""
    return _size(_gsr.gsr_extra_rows_size, desc, plan)


def backward_render_extra(desc, cam: Camera, geom_ws, binning_ws, image_ws, rows_ws, plan: FramePlan, out_color, aux: AuxOutputs, extra,
                          extra_map, dL_dcolor, dL_ddepth, dL_dalpha, dL_dextra_map, screen_grads, extra_rows_ws, dL_dextra, device):
    """gsr_backward_render_extra: any of the four upstream gradients may be None (zero); screen_grads as backward_render_aux leaves
    it, dL_dextra [P,3] receives the extra table's gradient."""
    _gsr.gsr_backward_render_extra(desc, cam, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), _ptr(rows_ws), plan, _ptr(out_color), aux,
                                   _ptr(extra), _ptr(extra_map), _ptr(dL_dcolor), _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(dL_dextra_map),
                                   _ptr(screen_grads), _ptr(extra_rows_ws), _ptr(dL_dextra), _stream(device))


def backward_render_median(desc, cam: Camera, geom_ws, binning_ws, image_ws, rows_ws, plan: FramePlan, out_color, aux: AuxOutputs,
                           dL_dcolor, dL_ddepth, dL_dalpha, median_enc, dL_dmedian, screen_grads, device):
    """gsr_backward_render_median: any of the four upstream gradients may be None (zero); screen_grads slot 9 receives dL/dz, the
    median map's share at each pixel's median splat included."""
    _gsr.gsr_backward_render_median(desc, cam, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), _ptr(rows_ws), plan, _ptr(out_color), aux,
                                    _ptr(dL_dcolor), _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(median_enc), _ptr(dL_dmedian),
                                    _ptr(screen_grads), _stream(device))


def backward_rows_size(desc: FrameDesc, plan: FramePlan) -> int:
    return _size(_gsr.gsr_backward_rows_size, desc, plan)


def backward_prepare(desc, g: Gaussians, plan: FramePlan, screen_grads, grads: Grads, device):
    _gsr.gsr_backward_prepare(desc, g, plan, _ptr(screen_grads), grads, _stream(device))


def backward_render(desc, cam: Camera, geom_ws, binning_ws, image_ws, rows_ws, plan: FramePlan, out_color, dL_dcolor, screen_grads,
                    device, absgrad: bool = False):
    """absgrad: gsr_backward_render_abs - screen_grads slots 10, 11 also receive the per-pixel absolute sums of d/dmean2D."""
    fn = _gsr.gsr_backward_render_abs if absgrad else _gsr.gsr_backward_render
    fn(desc, cam, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), _ptr(rows_ws), plan, _ptr(out_color), _ptr(dL_dcolor), _ptr(screen_grads),
       _stream(device))


def screen_absgrad(desc, radii, geom_ws, screen_grads, out, device, binned_ranks: int = -1, own_plan: Optional[FramePlan] = None):
    """gsr_screen_absgrad, behind backward_geom of the same arguments: out [P,3] = (slot 10, slot 11, 0) of the rows it visits."""
    _gsr.gsr_screen_absgrad(desc, _ptr(radii), _ptr(geom_ws), _ptr(screen_grads), binned_ranks, own_plan, _ptr(out), _stream(device))


def backward_render_aux(desc, cam: Camera, geom_ws, binning_ws, image_ws, rows_ws, plan: FramePlan, out_color, aux: AuxOutputs,
                        dL_dcolor, dL_ddepth, dL_dalpha, screen_grads, device):
    """gsr_backward_render_aux: any of the three upstream gradients may be None (zero); screen_grads slot 9 receives dL/dz."""
    _gsr.gsr_backward_render_aux(desc, cam, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), _ptr(rows_ws), plan, _ptr(out_color), aux,
                                 _ptr(dL_dcolor), _ptr(dL_ddepth), _ptr(dL_dalpha), _ptr(screen_grads), _stream(device))


_SEG = [0]


def bwd_segment_entries() -> int:
    """List entries per work unit of the blend backward (a build constant of the library)."""
    if not _SEG[0]:
        _SEG[0] = int(load().gsr_bwd_segment_entries())
    return _SEG[0]


def backward_geom(desc, cam: Camera, g: Gaussians, radii, geom_ws, screen_grads, g0, g1, grads: Grads, device,
                  binned_ranks: int = -1, own_plan: Optional[FramePlan] = None, depth_chain: bool = False):
    """own_plan: the frame's plan when screen_grads are this very frame's (gsr_backward_render of the same plan), else None.
    depth_chain: screen_grads slot 9 holds dL/dz (gsr_backward_render_aux): gsr_backward_geom_aux adds its chain to means3D."""
    fn = _gsr.gsr_backward_geom_aux if depth_chain else _gsr.gsr_backward_geom
    fn(desc, cam, g, _ptr(radii), _ptr(geom_ws), _ptr(screen_grads), g0, g1, binned_ranks, own_plan, grads, _stream(device))


def camera_grad_workspace_size(desc: FrameDesc) -> int:
    """gsr_camera_grad_workspace_size: bytes of the per-block partial sums of gsr_backward_camera."""
    return _size(_gsr.gsr_camera_grad_workspace_size, desc)


def backward_camera(desc, cam: Camera, g: Gaussians, radii, geom_ws, screen_grads, workspace, out: CameraGrads, device,
                    binned_ranks: int = -1, own_plan: Optional[FramePlan] = None, depth_chain: bool = False):
    """gsr_backward_camera, behind backward_geom of the same arguments (binned_ranks / own_plan / depth_chain as there)."""
    _gsr.gsr_backward_camera(desc, cam, g, _ptr(radii), _ptr(geom_ws), _ptr(screen_grads), binned_ranks, own_plan, int(bool(depth_chain)),
                             _ptr(workspace), out, _stream(device))


def binned_prefix(plan: FramePlan) -> int:
    """The depth ranks of the chunks that ran: the binned_ranks of a frame's own backward (csrc/gsr_dispatch.h geom_rows)."""
    return int(plan.chunk_rank_begin[plan.chunks_run]) if plan.num_rendered > 0 and plan.chunks_run > 0 else 0


def first_chunk_capacity(plan: FramePlan) -> int:
    """csrc/gsr_dispatch.h first_chunk_capacity (= gsr_binning_first_chunk_capacity), as plain arithmetic: rasterize_forward sizes the
    binning workspace between the plan readback and the first launch of stage 2, where the stream idles through every library call."""
    R, first = int(plan.num_rendered), int(plan.chunk_instances_max[0])
    return min(first + first // 4 + (1 << 20), R) if plan.num_chunks > 1 else R


def effective_binned_ranks(plan: FramePlan) -> int:
    """csrc/gsr_dispatch.h effective_binned_ranks: the ranks of the chunks that ran, a live-filtered chunk counted as nothing."""
    if plan.num_rendered <= 0 or plan.chunks_run <= 0:
        return 0
    return sum(int(plan.chunk_rank_begin[c + 1]) - int(plan.chunk_rank_begin[c]) for c in range(int(plan.chunks_run))
               if not (int(plan.chunks_filtered) >> c) & 1)


def backward_geom_rows(desc, cam: Camera, g: Gaussians, radii, geom_ws, screen_grads, rows, grads: Grads, device):
    """Sparse geometry backward over the Gaussians listed in `rows` (int32 device tensor)."""
    _gsr.gsr_backward_geom_rows(desc, cam, g, _ptr(radii), _ptr(geom_ws), _ptr(screen_grads), _ptr(rows), rows.numel(), grads, _stream(device))


_frame_offsets = {}


def frame_arrays(desc, geom_ws):
    """(depth_keys, depth_order): int32 views [P] into the geometry workspace (keys: bits of the view depth, -1 = invisible)."""
    P = desc.P
    offs = _frame_offsets.get(P)
    if offs is None:
        k, o = C.c_void_p(), C.c_void_p()
        _gsr.gsr_frame_arrays(desc, _ptr(geom_ws), k, o)
        base = geom_ws.data_ptr()
        offs = _frame_offsets[P] = (int(k.value) - base, int(o.value) - base)
    return tuple(geom_ws[o:o + 4 * P].view(torch.int32) for o in offs)


def exchange_rows_gather(desc, geom_ws, key_max: int, screen, n_rows: int):
    """(rows int32 [n_rows], packed float32 [n_rows, 12]): the Gaussians with depth key <= key_max in index order and their
    screen-gradient rows, packed for one all-reduce."""
    # n_rows comes from ANOTHER rank's count: entries this rank's keys do not fill must be inert (-1 is skipped by the scatter and by
    # the sparse geometry backward; their packed rows are zero), not whatever the allocator left there
    rows = torch.full((n_rows,), -1, dtype=torch.int32, device=screen.device)
    packed = torch.zeros(n_rows, SCREEN_GRAD_STRIDE, dtype=torch.float32, device=screen.device)
    _gsr.gsr_exchange_rows_gather(desc, _ptr(geom_ws), int(key_max) & 0xFFFFFFFF, _ptr(screen), n_rows, _ptr(rows), _ptr(packed),
                                  _stream(screen.device))
    return rows, packed


def exchange_rows_scatter(desc, rows, packed, screen):
    _gsr.gsr_exchange_rows_scatter(desc, rows.numel(), _ptr(rows), _ptr(packed), _ptr(screen), _stream(screen.device))


def mark_visible(means3D, viewmatrix, projmatrix, present):
    _gsr.gsr_mark_visible(means3D.shape[0], _ptr(means3D), _ptr(viewmatrix), _ptr(projmatrix), _ptr(present), _stream(means3D.device))


def debug_views(desc, geom_ws, binning_ws, image_ws, plan: FramePlan) -> dict:
    """Intermediate arrays as torch views INTO the workspaces (tests / profiling)."""
    v = DebugViews()
    _gsr.gsr_debug_get_views(desc, _ptr(geom_ws), _ptr(binning_ws), _ptr(image_ws), plan, v)
    P, N, R = desc.P, desc.width * desc.height, int(plan.binning_capacity or plan.num_rendered)
    Tn = ((desc.width + 15) // 16) * ((desc.height + 15) // 16)

    def view(ws, addr, nbytes, dtype, shape):
        if not addr or ws is None or nbytes == 0:
            return None
        off = addr - ws.data_ptr()
        return ws[off:off + nbytes].view(dtype).view(shape)
    return dict(
        splat_records=view(geom_ws, v.splat_records, P * 48, torch.float32, (P, 12)),
        tiles_touched=(lambda t: None if t is None else t[:, 0])(view(geom_ws, v.tiles_touched, P * 8, torch.int32, (P, 2))),
        optical_mass=(lambda t: None if t is None else t[:, 1])(view(geom_ws, v.tiles_touched, P * 8, torch.int32, (P, 2))),
        depth_order=view(geom_ws, v.depth_order, P * 4, torch.int32, (P,)),
        point_offsets=view(geom_ws, v.point_offsets, P * 4, torch.int32, (P,)),
        clamped=view(geom_ws, v.clamped, P, torch.uint8, (P,)),
        # bits 0..27 Gaussian index, bits 28..31 quadrant mask (copies: the workspace word holds both)
        sorted_gaussian=(lambda t: None if t is None else t & 0x0FFFFFFF)(view(binning_ws, v.sorted_gaussian, R * 4, torch.int32, (R,))),
        sorted_quadrants=(lambda t: None if t is None else (t >> 28) & 0xF)(view(binning_ws, v.sorted_gaussian, R * 4, torch.int32, (R,))),
        ranges=view(image_ws, v.ranges, MAX_CHUNKS * Tn * 8, torch.int32, (MAX_CHUNKS, Tn, 2)),
        final_T=view(image_ws, v.final_T, N * 4, torch.float32, (desc.height, desc.width)),
        n_contrib=view(image_ws, v.n_contrib, N * 4, torch.int32, (desc.height, desc.width)),
        tile_walk=view(image_ws, v.tile_walk, MAX_CHUNKS * Tn * 4, torch.int32, (MAX_CHUNKS, Tn)),
        # (tile | chunk << 24, segment) per work unit of the blend backward: per shard 17 lists [cap_full + 16 cap_part], their lengths
        bwd_units=view(binning_ws, v.bwd_units, 8 * (int(v.bwd_unit_cap_full) + 16 * int(v.bwd_unit_cap_part)) * 8, torch.int32,
                       (8, int(v.bwd_unit_cap_full) + 16 * int(v.bwd_unit_cap_part), 2)),
        bwd_unit_caps=(int(v.bwd_unit_cap_full), int(v.bwd_unit_cap_part)),
        bwd_unit_count=view(image_ws, v.bwd_unit_count, 8 * 17 * 4, torch.int32, (8, 17)))


def profile_enable(on: bool):
    """Per-kernel hipEvent timing inside the library (thread-local; resets the accumulators)."""
    _gsr.gsr_profile_enable(int(on))


def profile_read(n_max: int = 32) -> dict:
    """{kernel name: (total_ms, launches)} since profile_enable(True), up to n_max names; synchronises the recorded events."""
    names = ((C.c_char * PROFILE_NAME_LEN) * n_max)()
    ms = (C.c_float * n_max)()
    cnt = (C.c_int32 * n_max)()
    n = load().gsr_profile_read(n_max, names, ms, cnt)
    return {names[i].value.decode(): (float(ms[i]), int(cnt[i])) for i in range(n)}


def loss_workspace_size(C_, H, W) -> int:
    return _size(_gsr.gsr_loss_workspace_size, C_, H, W)


def loss_forward(image, target, lam, workspace, out3):
    Cn, H, W = image.shape
    _gsr.gsr_loss_l1_ssim_forward(Cn, H, W, lam, _ptr(image), _ptr(target), _ptr(workspace), _ptr(out3), _stream(image.device))


def loss_backward(image, target, lam, upstream, workspace, grad_image):
    Cn, H, W = image.shape
    _gsr.gsr_loss_l1_ssim_backward(Cn, H, W, lam, _ptr(upstream), _ptr(image), _ptr(target), _ptr(workspace), _ptr(grad_image), _stream(image.device))


def loss_l1_backward(image, target, upstream, grad_image):
    _gsr.gsr_loss_l1_backward(image.numel(), _ptr(upstream), _ptr(image), _ptr(target), _ptr(grad_image), _stream(image.device))


def loss_forward_rows(image, target, workspace, out2, row_begin, row_end):
    Cn, H, W = image.shape
    _gsr.gsr_loss_l1_ssim_forward_rows(Cn, H, W, _ptr(image), _ptr(target), _ptr(workspace), _ptr(out2), row_begin, row_end, _stream(image.device))


def loss_backward_rows(image, target, lam, upstream, workspace, grad_image, row_begin, row_end):
    Cn, H, W = image.shape
    _gsr.gsr_loss_l1_ssim_backward_rows(Cn, H, W, lam, _ptr(upstream), _ptr(image), _ptr(target), _ptr(workspace), _ptr(grad_image),
                                        row_begin, row_end, _stream(image.device))


def debug_sort_pairs(keys: torch.Tensor, vals: torch.Tensor, end_bit: int, count_on_device: bool = False):
    """Stable radix sort of (int32-viewed-as-u32 key, value) pairs through the library's own sort (test hook)."""
    n = keys.numel()
    k = [keys.contiguous().clone(), torch.empty_like(keys)]
    v = [vals.contiguous().clone(), torch.empty_like(vals)]
    temp = torch.empty(_size(_gsr.gsr_debug_sort_temp_bytes), dtype=torch.uint8, device=keys.device)
    res = C.c_int32(0)
    with torch.cuda.device(keys.device):
        _gsr.gsr_debug_sort_pairs(_ptr(k[0]) or temp.data_ptr(), _ptr(k[1]) or temp.data_ptr(), _ptr(v[0]) or temp.data_ptr(),
                                  _ptr(v[1]) or temp.data_ptr(), n, end_bit, int(count_on_device), _ptr(temp), res, _stream(keys.device))
    return k[res.value], v[res.value]


def debug_sort_pairs_ex(keys: torch.Tensor, vals: torch.Tensor, end_bit: int, n_max: int, base: int = 0,
                        vals2: Optional[torch.Tensor] = None, even_passes: bool = False):
    """The library's stable radix sort as the per-chunk tile sort calls it (test hook): the n = keys.numel() pairs sit at
    [base, base + n) of buffers of base + n_max words, the count and the base are device words, n_max sizes the launch and
    picks the scatter variant, vals2 (optional) travels with vals.  Returns (keys, vals, vals2 or None, result buffer) of the
    pairs' range."""
    n = keys.numel()
    if n > n_max:
        raise ValueError("n > n_max")
    size = base + max(n_max, 1)

    def pair(t):
        a = torch.full((size,), -1, dtype=torch.int32, device=keys.device)
        a[base:base + n] = t.reshape(-1).to(torch.int32)
        return [a, torch.full_like(a, -1)]
    k, v = pair(keys), pair(vals)
    v2 = pair(vals2) if vals2 is not None else [None, None]
    temp = torch.empty(_size(_gsr.gsr_debug_sort_temp_bytes), dtype=torch.uint8, device=keys.device)
    res = C.c_int32(0)
    with torch.cuda.device(keys.device):
        _gsr.gsr_debug_sort_pairs_ex(_ptr(k[0]), _ptr(k[1]), _ptr(v[0]), _ptr(v[1]), _ptr(v2[0]), _ptr(v2[1]), n, n_max, base, end_bit,
                                     int(even_passes), _ptr(temp), res, _stream(keys.device))
    r = res.value
    out = lambda bufs: None if bufs[r] is None else bufs[r][base:base + n]
    return out(k), out(v), out(v2), r


def dist2_knn3(xyz: torch.Tensor) -> torch.Tensor:
    """Mean squared distance to the 3 nearest other points (gsr_dist2_knn3)."""
    P = int(xyz.shape[0])
    pts = xyz.detach().float().contiguous()
    out = torch.zeros(P, dtype=torch.float32, device=pts.device)
    if P == 0:
        return out
    ws = torch.empty(_size(_gsr.gsr_dist2_workspace_size, P), dtype=torch.uint8, device=pts.device)
    with torch.cuda.device(pts.device):
        _gsr.gsr_dist2_knn3(P, _ptr(pts), _ptr(out), _ptr(ws), _stream(pts.device))
    return out


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step):
    _gsr.gsr_adam_step(param.numel(), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), lr, beta1, beta2, eps, int(step),
                       _stream(param.device))


def adam_step_split(param, grad, exp_avg, exp_avg_sq, split, lr_head, lr_tail, beta1, beta2, eps, step):
    """param [rows, ...] contiguous; the first `split` elements of every row step with lr_head, the rest with lr_tail."""
    rows = param.shape[0]
    row_len = param.numel() // max(rows, 1)
    _gsr.gsr_adam_step_split(rows, row_len, int(split), _ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), lr_head, lr_tail, beta1,
                             beta2, eps, int(step), _stream(param.device))


def _adam_tensors(items):
    """The C ABI's gsr_adam_tensor array of up to ADAM_MAX_TENSORS tuples (param, grad, exp_avg, exp_avg_sq, lr, lr_tail, step, row_len,
    split); row_len = 0: one learning rate for the tensor."""
    arr = (AdamTensor * len(items))()
    for a, (p, g, m, v, lr, lr_tail, step, row_len, split) in zip(arr, items):
        a.param, a.grad, a.exp_avg, a.exp_avg_sq, a.n = _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel()
        a.lr, a.lr_tail, a.step, a.row_len, a.split = float(lr), float(lr_tail), int(step), int(row_len), int(split)
    return len(items), arr


def adam_step_multi(items, beta1, beta2, eps):
    """The whole optimizer step in one launch; items: see _adam_tensors."""
    _gsr.gsr_adam_step_multi(*_adam_tensors(items), beta1, beta2, eps, _stream(items[0][0].device))


def adam_step_sparse_multi(items, visible, beta1, beta2, eps):
    """adam_step_multi over the rows that `visible` [rows] marks (gsr_adam_step_sparse_multi): bool / uint8 (non-zero) or int32
    (> 0, the rasterizer's radii) on the tensors' device; every param is [rows, ...].  A hidden row keeps param and both moments."""
    if visible.dtype not in (torch.bool, torch.uint8, torch.int32) or visible.dim() != 1:
        raise TypeError(f"adam_step_sparse_multi: visible must be a [rows] bool, uint8 or int32 tensor, got {visible.dtype} {tuple(visible.shape)}")
    if visible.device != items[0][0].device:
        raise ValueError(f"adam_step_sparse_multi: visible is on {visible.device}, the tensors on {items[0][0].device}")
    visible = visible.contiguous()
    _gsr.gsr_adam_step_sparse_multi(*_adam_tensors(items), visible.shape[0], _ptr(visible), visible.element_size(), beta1, beta2, eps,
                                    _stream(items[0][0].device))


def activations_forward(scaling_raw, rotation_raw, opacity_raw):
    """(exp, normalize, sigmoid) of the three raw tensors in one launch; any may be None."""
    some = next(t for t in (scaling_raw, rotation_raw, opacity_raw) if t is not None)
    P = some.shape[0]
    outs = [None if t is None else torch.empty_like(t) for t in (scaling_raw, rotation_raw, opacity_raw)]
    with torch.cuda.device(some.device):
        _gsr.gsr_activations_forward(P, _ptr(scaling_raw), _ptr(rotation_raw), _ptr(opacity_raw), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]),
                                     _stream(some.device))
    return tuple(outs)


def activations_backward(scales, rotation_raw, opacities, g_scales, g_rotations, g_opacities):
    """Gradients w.r.t. the raw tensors; a None incoming gradient gives a None result."""
    some = next(t for t in (scales, rotation_raw, opacities) if t is not None)
    P = some.shape[0]
    outs = [None if g is None else torch.empty_like(g) for g in (g_scales, g_rotations, g_opacities)]
    with torch.cuda.device(some.device):
        _gsr.gsr_activations_backward(P, _ptr(scales), _ptr(rotation_raw), _ptr(opacities), _ptr(g_scales), _ptr(g_rotations),
                                      _ptr(g_opacities), _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _stream(some.device))
    return tuple(outs)


def densify_stats(radii, viewspace_grad, max_radii2D, xyz_gradient_accum, denom):
    _gsr.gsr_densify_stats(radii.shape[0], _ptr(radii), _ptr(viewspace_grad), _ptr(max_radii2D), _ptr(xyz_gradient_accum), _ptr(denom),
                           _stream(radii.device))


def structured_compose_forward(decoded, means, opacities, scales, rotations, K: int, sh_coeffs: int):
    """gsr_structured_compose_forward: decoded [B, K (11 + 3 sh_coeffs)] and the four structure tensors (contiguous fp32 on one
    device) -> (xyz [P,3], opacity [P,1], scaling [P,3], rotation [P,4], features [P,sh_coeffs,3]), P = B K."""
    B = int(decoded.shape[0])
    P, kw = B * int(K), dict(dtype=torch.float32, device=decoded.device)
    outs = (torch.empty(P, 3, **kw), torch.empty(P, 1, **kw), torch.empty(P, 3, **kw), torch.empty(P, 4, **kw),
            torch.empty(P, int(sh_coeffs), 3, **kw))
    desc = StructuredDesc(B, int(K), int(sh_coeffs))
    st = Structures(_ptr(means), _ptr(opacities), _ptr(scales), _ptr(rotations))
    ch = Children(*(_ptr(t) for t in outs))
    with torch.cuda.device(decoded.device):
        _gsr.gsr_structured_compose_forward(desc, _ptr(decoded), st, ch, _stream(decoded.device))
    return outs


def structured_compose_backward(decoded, means, opacities, scales, rotations, K: int, sh_coeffs: int, grads_in, want):
    """gsr_structured_compose_backward.  grads_in: the five incoming gradients (contiguous, any None = zero); want: five booleans
    for (decoded, means, opacities, scales, rotations).  Returns the five gradients, None where not wanted."""
    desc = StructuredDesc(int(decoded.shape[0]), int(K), int(sh_coeffs))
    outs = [torch.empty_like(t) if w else None for t, w in zip((decoded, means, opacities, scales, rotations), want)]
    if desc.B == 0 or not any(want):
        return tuple(outs)
    st = Structures(_ptr(means), _ptr(opacities), _ptr(scales), _ptr(rotations))
    gin = ChildrenGrads(*(_ptr(g) for g in grads_in))
    gout = StructuredGrads(*(_ptr(t) for t in outs))
    with torch.cuda.device(decoded.device):
        _gsr.gsr_structured_compose_backward(desc, _ptr(decoded), st, gin, gout, _stream(decoded.device))
    return tuple(outs)


def opacity_compensation_forward(desc: FrameDesc, viewmatrix, means3D, opacities, scales, rotations, raw: bool):
    """gsr_opacity_compensation_forward: contiguous fp32 tensors on one device -> the compensated opacities, shaped like `opacities`
    (raw: logits in, logits out)."""
    out = torch.empty_like(opacities)
    if desc.P == 0:
        return out
    cam = Camera(None, _ptr(viewmatrix), None, None)
    g = Gaussians(_ptr(means3D), None, None, _ptr(opacities), _ptr(scales), _ptr(rotations), None, None, 2 if raw else 0)
    with torch.cuda.device(means3D.device):
        _gsr.gsr_opacity_compensation_forward(desc, cam, g, _ptr(out), _stream(means3D.device))
    return out


def opacity_compensation_backward(desc: FrameDesc, viewmatrix, means3D, opacities, scales, rotations, raw: bool, grad_out, want):
    """gsr_opacity_compensation_backward.  grad_out: dL/d(compensated opacities), contiguous; want: four booleans for (opacities,
    means3D, scales, rotations).  Returns the four gradients in that order, None where not wanted."""
    outs = [torch.empty_like(t) if w else None for t, w in zip((opacities, means3D, scales, rotations), want)]
    if desc.P == 0 or not any(want):
        return tuple(outs)
    cam = Camera(None, _ptr(viewmatrix), None, None)
    g = Gaussians(_ptr(means3D), None, None, _ptr(opacities), _ptr(scales), _ptr(rotations), None, None, 2 if raw else 0)
    grads = Grads(_ptr(outs[1]), None, None, None, _ptr(outs[0]), _ptr(outs[2]), _ptr(outs[3]), None, None, 0)
    with torch.cuda.device(means3D.device):
        _gsr.gsr_opacity_compensation_backward(desc, cam, g, _ptr(grad_out), grads, _stream(means3D.device))
    return tuple(outs)


def decoder_desc(latents, w0, w2) -> DecoderDesc:
    """The desc of one decoder call from its tensors: latents [B, L], w0 [hidden, IN], w2 [OUT, hidden]."""
    return DecoderDesc(int(latents.shape[0]), int(w0.shape[1]), int(latents.shape[1]), int(w0.shape[0]), int(w2.shape[0]))


def decoder_workspace_size(desc: DecoderDesc) -> int:
    return _size(_gsr.gsr_decoder_workspace_size, desc)


def decoder_forward(pos_emb, latents, params):
    """gsr_decoder_forward: pos_emb [B, IN - L] or None, latents [B, L], params = (w0, b0, w1, b1, w2, b2), contiguous fp32 on
    one device -> decoded [B, OUT]."""
    desc = decoder_desc(latents, params[0], params[4])
    decoded = torch.empty(desc.B, desc.out_size, dtype=torch.float32, device=latents.device)
    pr = DecoderParams(*(_ptr(t) for t in params))
    with torch.cuda.device(latents.device):
        _gsr.gsr_decoder_forward(desc, _ptr(pos_emb), _ptr(latents), pr, _ptr(decoded), _stream(latents.device))
    return decoded


def decoder_backward(pos_emb, latents, params, d_decoded, want):
    """gsr_decoder_backward.  d_decoded [B, OUT] contiguous; want: seven booleans for (latents, w0, b0, w1, b1, w2, b2).  Returns the
    seven gradients in that order, None where not wanted.  The workspace is a torch allocation that lives for the call."""
    desc = decoder_desc(latents, params[0], params[4])
    outs = [torch.empty_like(t) if w else None for t, w in zip((latents,) + tuple(params), want)]
    if not any(want):
        return tuple(outs)
    if desc.B == 0:
        return tuple(None if o is None else o.zero_() for o in outs)
    ws, nbytes = None, 0
    if any(want[1:]):
        nbytes = decoder_workspace_size(desc)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=latents.device)
    pr = DecoderParams(*(_ptr(t) for t in params))
    gr = DecoderGrads(*(_ptr(t) for t in outs))
    with torch.cuda.device(latents.device):
        _gsr.gsr_decoder_backward(desc, _ptr(pos_emb), _ptr(latents), pr, _ptr(d_decoded), gr, _ptr(ws), nbytes, _stream(latents.device))
    return tuple(outs)


def mcmc_relocation(opacity_raw, scaling_raw, sampled, min_opacity: float):
    """gsr_mcmc_relocation: opacity_raw [P,1] / [P], scaling_raw [P,3] (contiguous fp32), sampled [n] int64 on their device ->
    (new_opacity_raw [n], new_scaling_raw [n,3]).  The counter workspace is a torch allocation that lives for the call."""
    P, n = int(opacity_raw.shape[0]), int(sampled.shape[0])
    new_o = torch.empty(n, dtype=torch.float32, device=opacity_raw.device)
    new_s = torch.empty(n, 3, dtype=torch.float32, device=opacity_raw.device)
    nbytes = _size(_gsr.gsr_mcmc_relocation_workspace_size, P)
    if P == 0 or n == 0:
        return new_o, new_s
    ws = torch.empty(nbytes, dtype=torch.uint8, device=opacity_raw.device)
    with torch.cuda.device(opacity_raw.device):
        _gsr.gsr_mcmc_relocation(P, n, _ptr(opacity_raw), _ptr(scaling_raw), _ptr(sampled), min_opacity, _ptr(ws), _ptr(new_o), _ptr(new_s),
                                 _stream(opacity_raw.device))
    return new_o, new_s


def mcmc_relocate_rows(items, P: int, sampled, dead, new_opacity_raw, new_scaling_raw):
    """gsr_mcmc_relocate_rows.  items: up to MCMC_MAX_TENSORS tuples (param, exp_avg or None, exp_avg_sq or None, role) with role
    one of MCMC_ROLES; dead: [n] int64 or None."""
    arr = (McmcTensor * len(items))()
    for a, (p, m, v, role) in zip(arr, items):
        a.param, a.exp_avg, a.exp_avg_sq = _ptr(p), _ptr(m), _ptr(v)
        a.width, a.role = p.numel() // max(int(p.shape[0]), 1), MCMC_ROLES[role]
    dev = sampled.device
    with torch.cuda.device(dev):
        _gsr.gsr_mcmc_relocate_rows(len(items), arr, int(P), int(sampled.shape[0]), _ptr(sampled), _ptr(dead), _ptr(new_opacity_raw),
                                    _ptr(new_scaling_raw), _stream(dev))


def mcmc_inject_noise(xyz, scaling_raw, rotation_raw, opacity_raw, noise, c: float):
    """gsr_mcmc_inject_noise: in place on xyz [P,3]; all tensors contiguous fp32 on one device."""
    with torch.cuda.device(xyz.device):
        _gsr.gsr_mcmc_inject_noise(int(xyz.shape[0]), _ptr(xyz), _ptr(scaling_raw), _ptr(rotation_raw), _ptr(opacity_raw), _ptr(noise), c,
                                   _stream(xyz.device))


def mcmc_reg_grads(opacity_raw, scaling_raw, lambda_opacity: float, lambda_scale: float, grad_opacity, grad_scaling):
    """gsr_mcmc_reg_grads: in place on the given gradients (either may be None)."""
    some = grad_opacity if grad_opacity is not None else grad_scaling
    if some is None:
        return
    P = int(some.shape[0])
    with torch.cuda.device(some.device):
        _gsr.gsr_mcmc_reg_grads(P, _ptr(opacity_raw), _ptr(scaling_raw), lambda_opacity, lambda_scale, _ptr(grad_opacity), _ptr(grad_scaling),
                                _stream(some.device))


def _bilagrid_dims(grids):
    N, twelve, L, Gy, Gx = (int(v) for v in grids.shape)
    if twelve != 12:
        raise ValueError(f"bilagrid: grids must be [N, 12, L, Gy, Gx], got {tuple(grids.shape)}")
    return N, L, Gy, Gx


def bilagrid_workspace_sizes(H: int, W: int, L: int, Gy: int, Gx: int):
    """gsr_bilagrid_workspace_size -> (bytes of the backward's per-block partial sums, bytes of the TV workspace)."""
    return _size2(_gsr.gsr_bilagrid_workspace_size, H, W, L, Gy, Gx)


def bilagrid_forward(grids, image, idx: int):
    """gsr_bilagrid_forward: grids [N,12,L,Gy,Gx], image [3,H,W], contiguous fp32 on one device -> the corrected image [3,H,W]."""
    N, L, Gy, Gx = _bilagrid_dims(grids)
    H, W = int(image.shape[1]), int(image.shape[2])
    out = torch.empty_like(image)
    with torch.cuda.device(image.device):
        _gsr.gsr_bilagrid_forward(N, L, Gy, Gx, H, W, int(idx), _ptr(grids), _ptr(image), _ptr(out), _stream(image.device))
    return out


def bilagrid_backward(grids, image, idx: int, grad_out, want_grids: bool, want_image: bool):
    """gsr_bilagrid_backward -> (grad_grids [N,12,L,Gy,Gx] dense, grad_image [3,H,W]), None where not wanted.  The partial-sum
    workspace is a torch allocation that lives for the call."""
    N, L, Gy, Gx = _bilagrid_dims(grids)
    H, W = int(image.shape[1]), int(image.shape[2])
    if H * W == 0:
        return (torch.zeros_like(grids) if want_grids else None, torch.empty_like(image) if want_image else None)
    dgrids = torch.empty_like(grids) if want_grids else None
    dimage = torch.empty_like(image) if want_image else None
    ws, nbytes = None, 0
    if want_grids:
        nbytes = bilagrid_workspace_sizes(H, W, L, Gy, Gx)[0]
        ws = torch.empty(nbytes, dtype=torch.uint8, device=image.device)
    with torch.cuda.device(image.device):
        _gsr.gsr_bilagrid_backward(N, L, Gy, Gx, H, W, int(idx), _ptr(grids), _ptr(image), _ptr(grad_out), _ptr(dgrids), _ptr(dimage), _ptr(ws),
                                   nbytes, _stream(image.device))
    return dgrids, dimage


_tv_ws = {}


def _bilagrid_tv_workspace(device):
    """The TV forward's workspace of a (device, stream): cleared once, every call leaves its ticket at zero."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _tv_ws.get(key)
    if ws is None:
        ws = _tv_ws[key] = torch.zeros(bilagrid_workspace_sizes(1, 1, 1, 1, 1)[1], dtype=torch.uint8, device=device)
    return ws


def bilagrid_tv_forward(grids):
    """gsr_bilagrid_tv_forward -> the total variation, a 0-dim tensor."""
    N, L, Gy, Gx = _bilagrid_dims(grids)
    out = torch.empty(1, dtype=torch.float32, device=grids.device)
    ws = _bilagrid_tv_workspace(grids.device)
    with torch.cuda.device(grids.device):
        _gsr.gsr_bilagrid_tv_forward(N, L, Gy, Gx, _ptr(grids), _ptr(ws), _ptr(out), _stream(grids.device))
    return out.reshape(())


def bilagrid_tv_backward(grids, grad_out):
    """gsr_bilagrid_tv_backward: grad_out a one-element fp32 device tensor -> grad_grids."""
    N, L, Gy, Gx = _bilagrid_dims(grids)
    dgrids = torch.empty_like(grids)
    with torch.cuda.device(grids.device):
        _gsr.gsr_bilagrid_tv_backward(N, L, Gy, Gx, _ptr(grids), _ptr(grad_out), _ptr(dgrids), _stream(grids.device))
    return dgrids


def vq_workspace_size(P: int, K: int, D: int) -> int:
    """gsr_vq_workspace_size: bytes of scratch gsr_vq_assign and gsr_vq_update need (one size serves both)."""
    return _size(_gsr.gsr_vq_workspace_size, int(P), int(K), int(D))


def vq_assign(x, codebook):
    """gsr_vq_assign: x [P,D], codebook [K,D], contiguous fp32 on one device -> (idx int32 [P], dist2 fp32 [P])."""
    P, D = int(x.shape[0]), int(x.shape[1])
    K = int(codebook.shape[0])
    nbytes = vq_workspace_size(P, K, D)
    idx = torch.empty(P, dtype=torch.int32, device=x.device)
    dist2 = torch.empty(P, dtype=torch.float32, device=x.device)
    if P == 0:
        return idx, dist2
    with torch.cuda.device(x.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        _gsr.gsr_vq_assign(P, K, D, _ptr(x), _ptr(codebook), _ptr(idx), _ptr(dist2), _ptr(ws), nbytes, _stream(x.device))
    return idx, dist2


def vq_update(x, idx, codebook):
    """gsr_vq_update: x [P,D] fp32, idx [P] int32, codebook [K,D] fp32, contiguous on one device -> (new_codebook [K,D], counts int32 [K])."""
    P, D = int(x.shape[0]), int(x.shape[1])
    K = int(codebook.shape[0])
    nbytes = vq_workspace_size(P, K, D)
    out = torch.empty_like(codebook)
    counts = torch.empty(K, dtype=torch.int32, device=codebook.device)
    with torch.cuda.device(codebook.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=codebook.device)
        _gsr.gsr_vq_update(P, K, D, _ptr(x), _ptr(idx), _ptr(codebook), _ptr(out), _ptr(counts), _ptr(ws), nbytes, _stream(codebook.device))
    return out, counts


def filter3d_compute(xyz, cameras, focal_max: float):
    """gsr_filter3d_compute: xyz [P,3] and the camera table [C,16] (contiguous fp32 on one device; the table's layout: include/gsrast.h)
    -> (filter [P,1], any_seen).  The workspace is a torch allocation that lives for the call; reading any_seen is the call's one host
    synchronisation."""
    P, Cn = int(xyz.shape[0]), int(cameras.shape[0])
    out = torch.empty(P, 1, dtype=torch.float32, device=xyz.device)
    nbytes = _size(_gsr.gsr_filter3d_workspace_size, P)
    seen = C.c_int32(0)
    with torch.cuda.device(xyz.device):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=xyz.device)
        _gsr.gsr_filter3d_compute(P, Cn, _ptr(cameras), focal_max, _ptr(xyz), _ptr(out), _ptr(ws), nbytes, seen, _stream(xyz.device))
    return out, bool(seen.value)


def filter3d_apply_forward(opacities, scales, filter_3D, raw: bool):
    """gsr_filter3d_apply_forward: opacities [P] / [P,1], scales [P,3], filter_3D [P] / [P,1], contiguous fp32 on one device ->
    (opacities', scales') shaped like the inputs."""
    P = int(scales.shape[0])
    o_out, s_out = torch.empty_like(opacities), torch.empty_like(scales)
    with torch.cuda.device(scales.device):
        _gsr.gsr_filter3d_apply_forward(P, int(bool(raw)), _ptr(opacities), _ptr(scales), _ptr(filter_3D), _ptr(o_out), _ptr(s_out),
                                        _stream(scales.device))
    return o_out, s_out


def filter3d_apply_backward(opacities, scales, filter_3D, raw: bool, grad_opacities_out, grad_scales_out, want):
    """gsr_filter3d_apply_backward.  The incoming gradients are contiguous or None (zero); want: two booleans for (opacities, scales).
    Returns the two gradients, None where not wanted."""
    P = int(scales.shape[0])
    outs = [torch.empty_like(t) if w else None for t, w in zip((opacities, scales), want)]
    if P == 0 or not any(want):
        return tuple(outs)
    with torch.cuda.device(scales.device):
        _gsr.gsr_filter3d_apply_backward(P, int(bool(raw)), _ptr(opacities), _ptr(scales), _ptr(filter_3D), _ptr(grad_opacities_out),
                                         _ptr(grad_scales_out), _ptr(outs[0]), _ptr(outs[1]), _stream(scales.device))
    return tuple(outs)


def gaussian_normals_forward(scales, rotations, means3D, viewmatrix, campos):
    """gsr_gaussian_normals_forward: scales [P,3], rotations [P,4], means3D [P,3], viewmatrix [4,4], campos [3], contiguous fp32 on one
    device -> the view-space normals [P,3]."""
    P = int(scales.shape[0])
    out = torch.empty(P, 3, dtype=torch.float32, device=scales.device)
    with torch.cuda.device(scales.device):
        _gsr.gsr_gaussian_normals_forward(P, _ptr(scales), _ptr(rotations), _ptr(means3D), _ptr(viewmatrix), _ptr(campos), _ptr(out),
                                          _stream(scales.device))
    return out


def gaussian_normals_backward(scales, rotations, means3D, viewmatrix, campos, grad_out):
    """gsr_gaussian_normals_backward: grad_out [P,3] contiguous -> dL/drotations [P,4]."""
    P = int(scales.shape[0])
    out = torch.empty(P, 4, dtype=torch.float32, device=scales.device)
    with torch.cuda.device(scales.device):
        _gsr.gsr_gaussian_normals_backward(P, _ptr(scales), _ptr(rotations), _ptr(means3D), _ptr(viewmatrix), _ptr(campos), _ptr(grad_out),
                                           _ptr(out), _stream(scales.device))
    return out


def depth_normal_forward(depth, alpha, tanfovx, tanfovy, alpha_min):
    """gsr_depth_normal_forward: depth, alpha [H,W] contiguous fp32 on one device -> the normal map [3,H,W]."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    out = torch.empty(3, H, W, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        _gsr.gsr_depth_normal_forward(H, W, tanfovx, tanfovy, alpha_min, _ptr(depth), _ptr(alpha), _ptr(out), _stream(depth.device))
    return out


def depth_normal_backward(depth, alpha, tanfovx, tanfovy, alpha_min, grad_out, want):
    """gsr_depth_normal_backward.  grad_out [3,H,W] contiguous; want: two booleans for (depth, alpha).  Returns the two gradients, shaped
    like the inputs, None where not wanted."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    outs = [torch.empty_like(t) if w else None for t, w in zip((depth, alpha), want)]
    if H * W == 0 or not any(want):
        return tuple(outs)
    with torch.cuda.device(depth.device):
        _gsr.gsr_depth_normal_backward(H, W, tanfovx, tanfovy, alpha_min, _ptr(depth), _ptr(alpha), _ptr(grad_out), _ptr(outs[0]), _ptr(outs[1]),
                                       _stream(depth.device))
    return tuple(outs)


_nrm_ws = {}


def _normal_consistency_workspace(device, H, W):
    """The loss forward's workspace of a (device, stream): cleared when made (or grown), every call leaves its ticket at zero."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    need = _size(_gsr.gsr_normal_consistency_workspace_size, H, W)
    ws = _nrm_ws.get(key)
    if ws is None or ws.numel() < need:
        ws = _nrm_ws[key] = torch.zeros(need, dtype=torch.uint8, device=device)
    return ws


def normal_consistency_forward(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min):
    """gsr_normal_consistency_forward: normal_map [3,H,W], depth, alpha [H,W] contiguous fp32 on one device -> the loss, a 0-dim tensor."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    out = torch.empty(1, dtype=torch.float32, device=depth.device)
    with torch.cuda.device(depth.device):
        ws = _normal_consistency_workspace(depth.device, H, W)
        _gsr.gsr_normal_consistency_forward(H, W, tanfovx, tanfovy, alpha_min, _ptr(normal_map), _ptr(depth), _ptr(alpha), _ptr(ws), ws.numel(),
                                            _ptr(out), _stream(depth.device))
    return out.reshape(())


def normal_consistency_backward(normal_map, depth, alpha, tanfovx, tanfovy, alpha_min, grad_loss, want):
    """gsr_normal_consistency_backward.  grad_loss: a one-element fp32 device tensor; want: three booleans for (normal_map, depth, alpha).
    Returns the three gradients, shaped like the inputs, None where not wanted."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    outs = [torch.empty_like(t) if w else None for t, w in zip((normal_map, depth, alpha), want)]
    if not any(want):
        return tuple(outs)
    with torch.cuda.device(depth.device):
        _gsr.gsr_normal_consistency_backward(H, W, tanfovx, tanfovy, alpha_min, _ptr(normal_map), _ptr(depth), _ptr(alpha), _ptr(grad_loss),
                                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _stream(depth.device))
    return tuple(outs)


def depth_moments_forward(means3D, viewmatrix, mapping: int, near: float, far: float):
    """gsr_depth_moments_forward: means3D [P,3], viewmatrix [4,4], contiguous fp32 on one device -> the depth moments [P,3]."""
    P = int(means3D.shape[0])
    out = torch.empty(P, 3, dtype=torch.float32, device=means3D.device)
    with torch.cuda.device(means3D.device):
        _gsr.gsr_depth_moments_forward(P, _ptr(means3D), _ptr(viewmatrix), mapping, near, far, _ptr(out), _stream(means3D.device))
    return out


def depth_moments_backward(means3D, viewmatrix, mapping: int, near: float, far: float, grad_out):
    """gsr_depth_moments_backward: grad_out [P,3] contiguous -> dL/dmeans3D [P,3]."""
    P = int(means3D.shape[0])
    out = torch.empty(P, 3, dtype=torch.float32, device=means3D.device)
    with torch.cuda.device(means3D.device):
        _gsr.gsr_depth_moments_backward(P, _ptr(means3D), _ptr(viewmatrix), mapping, near, far, _ptr(grad_out), _ptr(out),
                                        _stream(means3D.device))
    return out


def distortion_map_forward(moments_map, alpha):
    """gsr_distortion_map_forward: moments_map [3,H,W], alpha [1,H,W] or [H,W], contiguous fp32 on one device -> the map [1,H,W]."""
    H, W = int(moments_map.shape[-2]), int(moments_map.shape[-1])
    out = torch.empty(1, H, W, dtype=torch.float32, device=alpha.device)
    with torch.cuda.device(alpha.device):
        _gsr.gsr_distortion_map_forward(H, W, _ptr(moments_map), _ptr(alpha), _ptr(out), _stream(alpha.device))
    return out


def _distortion_backward(fn, moments_map, alpha, grad, want):
    H, W = int(moments_map.shape[-2]), int(moments_map.shape[-1])
    outs = [torch.empty_like(t) if w else None for t, w in zip((moments_map, alpha), want)]
    if H * W == 0 or not any(want):
        return tuple(outs)
    with torch.cuda.device(alpha.device):
        fn(H, W, _ptr(moments_map), _ptr(alpha), _ptr(grad), _ptr(outs[0]), _ptr(outs[1]), _stream(alpha.device))
    return tuple(outs)


def distortion_map_backward(moments_map, alpha, grad_out, want):
    """gsr_distortion_map_backward.  grad_out [H W] contiguous; want: two booleans for (moments_map, alpha).  Returns the two gradients,
    shaped like the inputs, None where not wanted."""
    return _distortion_backward(_gsr.gsr_distortion_map_backward, moments_map, alpha, grad_out, want)


def distortion_loss_forward(moments_map, alpha):
    """gsr_distortion_loss_forward -> the loss, a 0-dim tensor.  The blocks' sums live in a workspace of the call's own (the caching
    allocator hands it out on the current stream), so calls on two streams share nothing."""
    H, W = int(moments_map.shape[-2]), int(moments_map.shape[-1])
    out = torch.empty(1, dtype=torch.float32, device=alpha.device)
    with torch.cuda.device(alpha.device):
        ws = torch.empty(_size(_gsr.gsr_distortion_loss_workspace_size, H, W), dtype=torch.uint8, device=alpha.device)
        _gsr.gsr_distortion_loss_forward(H, W, _ptr(moments_map), _ptr(alpha), _ptr(ws), ws.numel(), _ptr(out), _stream(alpha.device))
    return out.reshape(())


def distortion_loss_backward(moments_map, alpha, grad_loss, want):
    """gsr_distortion_loss_backward.  grad_loss: a one-element fp32 device tensor; want as for distortion_map_backward."""
    return _distortion_backward(_gsr.gsr_distortion_loss_backward, moments_map, alpha, grad_loss, want)


def tsdf_integrate(dims, origin, voxel_size, sdf_trunc, viewmatrix, depth, alpha, color, tanfovx, tanfovy, alpha_min, depth_max, tsdf, weight,
                   vol_color):
    """gsr_tsdf_integrate on the volume's device and its current stream: depth, alpha [H,W], color [3,H,W], viewmatrix [4,4] and the three
    volume arrays, contiguous fp32 on one device.  One launch, no synchronisation."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    with torch.cuda.device(tsdf.device):
        _gsr.gsr_tsdf_integrate(*dims, *origin, voxel_size, sdf_trunc, H, W, tanfovx, tanfovy, alpha_min, depth_max, _ptr(viewmatrix), _ptr(depth),
                                _ptr(alpha), _ptr(color), _ptr(tsdf), _ptr(weight), _ptr(vol_color), _stream(tsdf.device))


def tsdf_extract_mesh(dims, origin, voxel_size, min_weight, tsdf, weight, vol_color):
    """gsr_tsdf_mesh_count and gsr_tsdf_mesh_emit on the volume's device and its current stream -> (vertices [V,3] float32, faces [F,3]
    int32, colors [V,3] float32).  One host readback: the two totals that size the outputs."""
    dev = tsdf.device
    nbytes = _size(_gsr.gsr_tsdf_mesh_workspace_size, *dims)
    nv, nf = C.c_int64(0), C.c_int64(0)
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _gsr.gsr_tsdf_mesh_count(*dims, min_weight, _ptr(tsdf), _ptr(weight), _ptr(ws), nbytes, nv, nf, _stream(dev))
        vertices = torch.empty(nv.value, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf.value, 3, dtype=torch.int32, device=dev)
        colors = torch.empty(nv.value, 3, dtype=torch.float32, device=dev)
        _gsr.gsr_tsdf_mesh_emit(*dims, *origin, voxel_size, min_weight, _ptr(tsdf), _ptr(weight), _ptr(vol_color), _ptr(ws), nbytes, nv.value,
                                nf.value, _ptr(vertices), _ptr(faces), _ptr(colors), _stream(dev))
    return vertices, faces, colors


def tsdf_sparse_allocate(dims, origin, voxel_size, sdf_trunc, pad, viewmatrix_inverse, depth, alpha, tanfovx, tanfovy, alpha_min, depth_max, marks):
    """gsr_tsdf_sparse_allocate on the marks' device and its current stream.  One launch, no synchronisation."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    with torch.cuda.device(marks.device):
        _gsr.gsr_tsdf_sparse_allocate(*dims, *origin, voxel_size, sdf_trunc, pad, H, W, tanfovx, tanfovy, alpha_min, depth_max,
                                      _ptr(viewmatrix_inverse), _ptr(depth), _ptr(alpha), _ptr(marks), _stream(marks.device))


def tsdf_sparse_commit_count(dims, marks, table):
    """gsr_tsdf_sparse_commit_count on the table's device and its current stream -> (new bricks, workspace, its bytes).  The one host
    readback of a commit; the workspace carries the prefixes to tsdf_sparse_commit_assign."""
    dev = table.device
    nbytes = _size(_gsr.gsr_tsdf_sparse_commit_workspace_size, *dims)
    new = C.c_int64(0)
    with torch.cuda.device(dev):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _gsr.gsr_tsdf_sparse_commit_count(*dims, _ptr(marks), _ptr(table), _ptr(ws), nbytes, new, _stream(dev))
    return new.value, ws, nbytes


def tsdf_sparse_commit_assign(dims, num_bricks, marks, table, ws, nbytes, coords, order, rank):
    """gsr_tsdf_sparse_commit_assign: coords [capacity,3], order and rank [capacity] int32 with room for the new bricks."""
    dev = table.device
    with torch.cuda.device(dev):
        _gsr.gsr_tsdf_sparse_commit_assign(*dims, num_bricks, int(coords.shape[0]), _ptr(marks), _ptr(table), _ptr(ws), nbytes, _ptr(coords),
                                           _ptr(order), _ptr(rank), _stream(dev))


def tsdf_sparse_integrate(dims, origin, voxel_size, sdf_trunc, viewmatrix, depth, alpha, color, tanfovx, tanfovy, alpha_min, depth_max, num_bricks,
                          coords, tsdf, weight, vol_color):
    """gsr_tsdf_sparse_integrate on the pool's device and its current stream.  One launch, no synchronisation."""
    H, W = int(depth.shape[-2]), int(depth.shape[-1])
    with torch.cuda.device(tsdf.device):
        _gsr.gsr_tsdf_sparse_integrate(*dims, *origin, voxel_size, sdf_trunc, H, W, tanfovx, tanfovy, alpha_min, depth_max, num_bricks,
                                       _ptr(viewmatrix), _ptr(depth), _ptr(alpha), _ptr(color), _ptr(coords), _ptr(tsdf), _ptr(weight),
                                       _ptr(vol_color), _stream(tsdf.device))


def tsdf_sparse_extract_mesh(dims, origin, voxel_size, min_weight, num_bricks, tsdf, weight, vol_color, table, coords, order, rank, return_cells):
    """gsr_tsdf_sparse_mesh_count and gsr_tsdf_sparse_mesh_emit on the pool's device and its current stream -> (vertices [V,3] float32,
    faces [F,3] int32, colors [V,3] float32, cells [V,3] int32 or None).  One host readback: the two totals that size the outputs."""
    dev = table.device
    nbytes = _size(_gsr.gsr_tsdf_sparse_mesh_workspace_size, num_bricks)
    nv, nf = C.c_int64(0), C.c_int64(0)
    bricks = (_ptr(table), _ptr(coords), _ptr(order), _ptr(rank))
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        _gsr.gsr_tsdf_sparse_mesh_count(*dims, num_bricks, min_weight, _ptr(tsdf), _ptr(weight), *bricks, _ptr(ws), nbytes, nv, nf, _stream(dev))
        vertices = torch.empty(nv.value, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf.value, 3, dtype=torch.int32, device=dev)
        colors = torch.empty(nv.value, 3, dtype=torch.float32, device=dev)
        cells = torch.empty(nv.value, 3, dtype=torch.int32, device=dev) if return_cells else None
        _gsr.gsr_tsdf_sparse_mesh_emit(*dims, *origin, voxel_size, num_bricks, min_weight, _ptr(tsdf), _ptr(weight), _ptr(vol_color), *bricks,
                                       _ptr(ws), nbytes, nv.value, nf.value, _ptr(vertices), _ptr(faces), _ptr(colors),
                                       _ptr(cells) if return_cells else None, _stream(dev))
    return vertices, faces, colors, cells


def mesh_components(faces, V):
    """gsr_mesh_components on the faces' device and its current stream -> (labels [F] int32, sizes [V] int32, workspace, its bytes).  No
    host synchronisation; the workspace carries the union-find's give-up word to mesh_clean."""
    dev, F = faces.device, int(faces.shape[0])
    nbytes = _size(_gsr.gsr_mesh_clean_workspace_size, V, F)
    with torch.cuda.device(dev):
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        labels = torch.empty(F, dtype=torch.int32, device=dev)
        sizes = torch.empty(V, dtype=torch.int32, device=dev)
        _gsr.gsr_mesh_components(V, F, _ptr(faces), _ptr(labels), _ptr(sizes), _ptr(ws), nbytes, _stream(dev))
    return labels, sizes, ws, nbytes


def mesh_clean(faces, V, labels, sizes, threshold_dev, ws, nbytes):
    """gsr_mesh_clean_count and gsr_mesh_clean_emit behind mesh_components (its labels, sizes and workspace), on the same stream ->
    (vertex_src [V'] int32, face_src [F'] int32, faces_out [F',3] int32).  threshold_dev: a one-element int32 device tensor.  One host
    readback: the two totals that size the outputs (and the give-up word: a set one raises GsrError)."""
    dev, F = faces.device, int(faces.shape[0])
    nv, nf = C.c_int64(0), C.c_int64(0)
    with torch.cuda.device(dev):
        _gsr.gsr_mesh_clean_count(V, F, _ptr(faces), _ptr(labels), _ptr(sizes), _ptr(threshold_dev), _ptr(ws), nbytes, nv, nf, _stream(dev))
        vertex_src = torch.empty(nv.value, dtype=torch.int32, device=dev)
        face_src = torch.empty(nf.value, dtype=torch.int32, device=dev)
        faces_out = torch.empty(nf.value, 3, dtype=torch.int32, device=dev)
        _gsr.gsr_mesh_clean_emit(V, F, _ptr(faces), _ptr(ws), nbytes, nv.value, nf.value, _ptr(vertex_src), _ptr(face_src), _ptr(faces_out),
                                 _stream(dev))
    return vertex_src, face_src, faces_out
