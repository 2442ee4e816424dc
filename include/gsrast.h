/* gsrast.h — C ABI of libgsrast.so, the MI355X (gfx950) differentiable Gaussian rasterizer.
 *
 * This is the drop-in boundary of the hot path.  In the reference the boundary is the pybind11
 * module `diff_gaussian_rasterization._C` of the un-vendored submodule (call site:
 * gaussian_renderer/__init__.py:14,36-51,85-93; contract visible at train.py:106,129 and
 * scene/gaussian_model.py:415-417).  Each entry point below names the `_C` function it replaces.
 *
 * Conventions
 *   - plain C types only; every pointer is a DEVICE pointer unless the name ends in `_host`
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is enqueued on it
 *   - optional inputs/outputs: NULL <=> not provided (the reference passes empty tensors)
 *   - return value: 0 = ok, negative = gsr_status; message via gsr_last_error() (thread-local)
 *   - the library holds no global mutable state; it is re-entrant (forward on the Python main
 *     thread, backward on the autograd worker thread)
 *   - all float tensors are contiguous fp32, layouts as at the reference call site:
 *       means3D[P,3] shs[P,M,3] colors_precomp[P,3] opacities[P] scales[P,3] rotations[P,4]
 *       cov3D_precomp[P,6] viewmatrix[4,4] projmatrix[4,4] (both already transposed, row-vector
 *       convention: scene/cameras.py:54-56) campos[3] bg[3] out_color[3,H,W] radii[P] (int32)
 */
#ifndef GSRAST_H
#define GSRAST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_VERSION 12
#define GSR_SCREEN_GRAD_STRIDE 12   /* floats per Gaussian in `screen_grads`: (dmean2D.x, dmean2D.y,
                                       dconic A, B, C, dopacity, drgb[3], dz (gsr_backward_render_aux;
                                       0 otherwise), 2 pad: the absolute sums of gsr_backward_render_abs,
                                       0 otherwise) */

typedef enum gsr_status {
    GSR_OK = 0,
    GSR_ERR_INVALID_ARGUMENT = -1,
    GSR_ERR_HIP = -2,            /* a HIP runtime call or kernel launch failed */
    GSR_ERR_PREFILTERED = -3,    /* prefiltered=1 but a Gaussian failed the frustum test (A.1) */
    GSR_ERR_WORKSPACE = -4       /* workspace too small for this frame */
} gsr_status;

/* Per-call configuration = the scalar fields of GaussianRasterizationSettings
 * (gaussian_renderer/__init__.py:36-49) plus the tile-row slab of multi-GPU sharding. */
typedef struct gsr_frame_desc {
    int32_t P;               /* number of Gaussians (< 2^28)                                     */
    int32_t sh_degree;       /* active SH degree D, 0..3                                          */
    int32_t sh_coeffs;       /* M = stored coefficients per channel of shs[P,M,3]; 0 with colors */
    int32_t width, height;   /* image_width, image_height                                        */
    float tanfovx, tanfovy, scale_modifier;
    int32_t prefiltered, debug;
    int32_t tile_row_begin;  /* slab [tile_row_begin, tile_row_end) in 16-px tile rows;           */
    int32_t tile_row_end;    /* tile_row_end <= 0 means "to the last row" (whole image: 0, 0)     */
} gsr_frame_desc;

/* Host-side plan of one frame, written by gsr_forward_preprocess and handed to the later stages (the
 * library itself keeps no per-frame state).  The forward is PROGRESSIVE: visible Gaussians are sorted by
 * depth once, split into up to GSR_MAX_CHUNKS depth chunks, and each chunk is binned and blended only
 * into tiles that still have an unsaturated pixel; a tile whose 256 pixels have all hit the
 * transmittance cut-off (A.8) takes no further instances.  Pixels are identical to binning everything. */
#define GSR_MAX_CHUNKS 8
typedef struct gsr_frame_plan {
    int64_t num_rendered;                         /* R: sum over Gaussians of the tiles of their binning
                                                     rectangle (the reference's rectangle clipped to the slab and to
                                                     the alpha >= 1/255 bounding box): upper bound of the instances
                                                     emitted; <= the reference's num_rendered                */
    int32_t num_visible;                          /* V: Gaussians with radius > 0                           */
    int32_t num_chunks;                           /* depth chunks planned (1..GSR_MAX_CHUNKS)               */
    int32_t chunk_rank_begin[GSR_MAX_CHUNKS + 1]; /* chunk c = positions [begin[c], begin[c+1]) of the depth order */
    int64_t chunk_instances_max[GSR_MAX_CHUNKS];  /* instances of chunk c if every tile were open           */
    int32_t chunks_run;                           /* out of gsr_forward_render: chunks actually processed   */
    int32_t sort_result;                          /* out of gsr_forward_render: radix buffer holding lists  */
    int64_t instances_emitted;                    /* out of gsr_forward_render: instances actually binned;
                                                     -1 when the last chunk ran (its count is not read back)  */
    int32_t binning_initialised;                  /* gsr_forward_preprocess was given the image workspace and has
                                                     already reset the tile ranges / open flags in it        */
    int32_t screen_prezeroed;                     /* 1 (set by gsr_backward_prepare): screen_grads is already all zero; 2 (set by
                                                     the caller): only the rows of the binned depth prefix will be read (by the
                                                     sparse gsr_backward_geom of this frame) - no clearing at all            */
    int64_t binning_capacity;                     /* IN to gsr_forward_render (and the backward): instances the binning
                                                     workspace was sized for (gsr_binning_size of that number); 0 = R   */
    uint32_t chunk_key_end[GSR_MAX_CHUNKS];       /* chunk c = visible Gaussians whose depth bits lie in (key_end[c-1], key_end[c]]:
                                                     the chunks are SELECTED by depth; each is sorted when it is binned.
                                                     The last planned chunk's end, and every entry behind it, is 0xFFFFFFFE  */
    int32_t chunks_sorted;                        /* chunks [0, chunks_sorted) of the depth order are already sorted: a re-run of
                                                     gsr_forward_render (after GSR_ERR_WORKSPACE) does not sort them again   */
    int32_t chunks_filtered;                      /* bit c: chunk c was put through the live filter (only the Gaussians that can still
                                                     reach an open tile sit at the front of its range, sorted and binned)        */
    int32_t tile_order_ready;                     /* set by gsr_forward when its zero fill also cleared the blend backward's row-valid
                                                     flags (gsr_backward_render then skips that memset); cleared by
                                                     gsr_forward_render                                                         */
    uint32_t key_max;                             /* no visible Gaussian's depth key exceeds it: the last chunk's sort skips the bits above */
} gsr_frame_plan;

typedef struct gsr_camera {      /* tensor fields of GaussianRasterizationSettings (device) */
    const float *bg, *viewmatrix, *projmatrix, *campos;
} gsr_camera;

typedef struct gsr_gaussians {   /* arguments of GaussianRasterizer.forward (device) */
    const float *means3D, *shs, *colors_precomp, *opacities, *scales, *rotations, *cov3D_precomp;
    /* SURVEY 8a row a14, optional: raw != 0 hands over the optimizer's RAW parameters of the reference's
     * GaussianModel and the activations of scene/gaussian_model.py:47-60,108-127 run inside the per-Gaussian
     * kernels instead of as ~30 torch kernels around them:
     *   opacities = _opacity logits        -> sigmoid        scales    = _scaling log-scales -> exp
     *   rotations = _rotation quaternions  -> normalize      shs       = _features_dc   [P,1,3]
     *   shs_rest  = _features_rest [P, sh_coeffs - 1, 3] (the torch.cat of get_features); NULL iff sh_coeffs == 1
     * raw == 2: the same activations, but the SH coefficients are ONE interleaved table, shs = [P, sh_coeffs, 3] exactly as in the
     * activated case (shs_rest NULL; grads.shs is then [P, sh_coeffs, 3] too): a parameter store that keeps get_features as a
     * single leaf needs no cat and no split.
     * colors_precomp and cov3D_precomp must be NULL.  The backward then returns gradients w.r.t. the raw
     * tensors (chain rule through the activations fused into gsr_backward_geom). */
    const float *shs_rest;
    int32_t raw;
} gsr_gaussians;

typedef struct gsr_grads {       /* outputs of the backward; any may be NULL (not wanted) */
    float *means3D;        /* [P,3]   */
    float *means2D;        /* [P,3]   (x, y) = dL/d(NDC position) incl. W/2, H/2; z = 0            */
    float *shs;            /* [P,M,3] */
    float *colors_precomp; /* [P,3]   */
    float *opacities;      /* [P]     */
    float *scales;         /* [P,3]   */
    float *rotations;      /* [P,4]   */
    float *cov3D_precomp;  /* [P,6]   */
    float *shs_rest;       /* [P,M-1,3] raw == 1 only (then shs is [P,1,3]) */
    int32_t prezeroed;     /* != 0: the caller has already zero-filled every non-NULL tensor above (gsr_backward_prepare);
                              the sparse path of gsr_backward_geom then skips its own fill */
} gsr_grads;

int gsr_version(void);
const char *gsr_last_error(void);

/* Sizes of the two frame-sized opaque workspaces (the reference's geomBuffer / imgBuffer, which
 * `_C.rasterize_gaussians` allocates through its resize callback). */
int gsr_workspace_sizes(const gsr_frame_desc *desc, size_t *geom_bytes, size_t *image_bytes);

/* Size of the per-duplicate workspace (the reference's binningBuffer) for `num_rendered` instances: 24 bytes each.
 * The reference sizes it for R = plan->num_rendered.  Here only what the depth chunks actually emit is touched (2-8 % of R
 * on frames whose tiles saturate), so a caller may size it for gsr_binning_first_chunk_capacity() instances, set
 * plan->binning_capacity to that number, and fall back to R when gsr_forward_render answers GSR_ERR_WORKSPACE (a later
 * chunk did not fit; nothing of it was written: re-run gsr_forward_render with the larger workspace). */
int gsr_binning_size(const gsr_frame_desc *desc, int64_t num_rendered, size_t *binning_bytes);
int gsr_binning_first_chunk_capacity(const gsr_frame_plan *plan_host, int64_t *instances);

/* Stage 1 of `_C.rasterize_gaussians`: per-Gaussian preprocess (cull, project, EWA covariance,
 * SH colour), depth sort of the Gaussians, prefix sum of tiles touched in depth order, chunk plan.
 * Writes radii[P] and *plan_host (one host synchronisation; plan->num_rendered sizes the binning
 * workspace).  image_ws (optional, may be NULL): when given, the per-frame reset of the tile ranges and open
 * flags that stage 2 needs is enqueued here, BEFORE the host waits for the plan, so that it runs in the
 * shadow of the readback. */
int gsr_forward_preprocess(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                           void *geom_ws, void *image_ws, int32_t *radii, gsr_frame_plan *plan_host, void *stream);

/* Stage 2 of `_C.rasterize_gaussians`: per depth chunk — emit (tile, instance) pairs into open tiles,
 * stable radix sort by tile, tile ranges, per-tile front-to-back blend continuing each pixel's state.
 * Stops as soon as no tile is open (one 4-byte readback per chunk).  Updates plan_host->chunks_run /
 * instances_emitted.  Rows of out_color outside the slab are left untouched.  `g` = the same tensors as in stage 1:
 * SH colours (A.6) are evaluated HERE, per chunk, only for the Gaussians of the chunks that get binned. */
int gsr_forward_render(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                       void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color, void *stream);

/* Both stages in ONE call, for callers that bring a binning workspace sized from a guess (the last frame of the same shape):
 * gsr_forward_preprocess, then — without going back to the caller, whose own code between the two calls (an interpreter, a
 * framework's dispatcher) costs tens of microseconds of idle stream right after the plan readback — gsr_forward_render into
 * `binning_ws` if its `binning_capacity` instances cover what gsr_binning_first_chunk_capacity asks for.  If they do not:
 * GSR_ERR_WORKSPACE with the plan filled in and nothing of stage 2 enqueued; allocate and call gsr_forward_render.
 * early_fill (optional): the backward's outputs, as for gsr_backward_prepare (grads->..., any NULL tensor is skipped; the
 * screen-space tensor is not part of it: see gsr_frame_plan.screen_prezeroed = 2).  When the frame ends sparse
 * (chunk_rank_begin[chunks_run] * 4 < P) their zero fill is enqueued here, right after the last readback of stage 2, instead of
 * tens of microseconds later from the caller: early_fill->prezeroed is set and gsr_backward_geom skips its own fill. */
int gsr_forward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                gsr_grads *early_fill, void *stream);

/* Size of the backward-only scratch: one 48-byte gradient row and one "row written" byte per instance the forward EMITTED
 * (plan_host->instances_emitted, a few per cent of num_rendered; the emission bound of the chunks that ran
 * when the forward went through its last chunk), so it is allocated when the backward runs and freed right
 * after it. */
int gsr_backward_rows_size(const gsr_frame_desc *desc, const gsr_frame_plan *plan_host, size_t *rows_bytes);

/* Optional: zero-fill the backward's outputs AHEAD of time, in one launch — typically right after
 * gsr_forward_render returns, when the stream is idle while the host walks back through the caller's code to the
 * loss.  screen_grads [P, GSR_SCREEN_GRAD_STRIDE] (may be NULL) and every non-NULL tensor of `grads` are
 * cleared; plan_host->screen_prezeroed and grads->prezeroed are set so that gsr_backward_render /
 * gsr_backward_geom skip their own fills.  Only worth calling when the sparse geometry backward will run
 * (plan->chunk_rank_begin[plan->chunks_run] * 4 < P). */
int gsr_backward_prepare(const gsr_frame_desc *desc, const gsr_gaussians *g, gsr_frame_plan *plan_host, float *screen_grads,
                         gsr_grads *grads, void *stream);

/* First half of `_C.rasterize_gaussians_backward`: the blend's backward over the slab's tiles into rows_ws and the
 * deterministic per-Gaussian reduction -> screen_grads[P, GSR_SCREEN_GRAD_STRIDE].  out_color = the image the forward
 * of this frame wrote ([3,H,W], unchanged since: the backward walks the lists front to back and needs the final pixel). */
int gsr_backward_render(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                        const void *image_ws, void *rows_ws, const gsr_frame_plan *plan_host, const float *out_color,
                        const float *dL_dcolor, float *screen_grads, void *stream);

/* List entries per work unit of the blend backward (a build constant: binning workspaces hold one 4 KB checkpoint per that
 * many instances). */
int gsr_bwd_segment_entries(void);

/* Second half of `_C.rasterize_gaussians_backward`: per-Gaussian backward (2D covariance, projection,
 * SH, 3D covariance) for Gaussians [g_begin, g_end).  Every non-NULL output row in that range is
 * written (zeros for invisible Gaussians and for SH coefficients above the active degree).
 * binned_ranks: a HINT — the number of leading depth ranks outside which `screen_grads` is known to be all
 * zero (plan->chunk_rank_begin[plan->chunks_run] for gradients that come from THIS frame's
 * gsr_backward_render, or the maximum over ranks after a multi-GPU sum), or -1 for "unknown".  When the whole
 * range is requested and the prefix is short the outputs are memset and only the prefix is visited.
 * own_plan (may be NULL): the frame's plan, when screen_grads come from gsr_backward_render of this very frame (and only then):
 * replaces the hint — a rank that emitted no instance is skipped before anything of it is read, and a chunk that went through the
 * live filter counts as nothing when choosing between "memset + visit" and the dense pass (a training frame whose last chunk is
 * most of the scene binned a few per cent of it). */
int gsr_backward_geom(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                      const int32_t *radii, const void *geom_ws, const float *screen_grads, int32_t g_begin,
                      int32_t g_end, int32_t binned_ranks, const gsr_frame_plan *own_plan, const gsr_grads *out, void *stream);

/* gsr_backward_geom for an explicit list of Gaussians: the sparse geometry backward visits rows[0 .. n_rows) (device,
 * Gaussian indices) instead of the frame's own binned depth prefix; every other row of the outputs must already be zero
 * (gsr_backward_prepare) or is cleared first.  n_rows * 4 >= P runs the dense kernel over all P.  This is what a rank of
 * a tile-row-sharded render calls after the ranks have summed their screen-space gradients: the list is then the union
 * of what the ranks binned (all Gaussians whose depth key is <= the largest chunk end any rank reached). */
int gsr_backward_geom_rows(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                           const void *geom_ws, const float *screen_grads, const int32_t *rows, int32_t n_rows, const gsr_grads *out,
                           void *stream);

/* ---- Depth and alpha maps beside the colour image (the "aux" outputs; additive: every call above keeps its meaning).
 * For one pixel, over the splats the colour composites (same alpha >= 1/255 test, 0.99 clamp and stop rule), w_i = alpha_i T_i:
 *   depth = sum_i w_i z_i   z_i = the Gaussian's view-space z, (means3D . viewmatrix)_z; no background term, not normalised
 *                           (mean depth = depth / alpha)
 *   alpha = 1 - T_final     T_final = |final_T| of gsr_debug_views (frozen in front of the stopping splat)
 * Both are differentiable: gsr_backward_render_aux takes their upstream gradients, gsr_backward_geom_aux adds the depth's chain
 * to means3D.  The means2D gradient then carries the depth and alpha loss terms too (it feeds the densification statistics).
 * ckpt_ws: the depth so far at every checkpoint of the blend backward, gsr_aux_workspace_size bytes for a binning workspace of
 * `binning_capacity` instances (0 = num_rendered): 1 KB per 128 instances plus (GSR_MAX_CHUNKS - 1) KB per 16x16 tile.  It may
 * be NULL when the frame binned nothing (num_rendered == 0).  Whole images only (tile_row_begin = tile_row_end = 0). */
typedef struct gsr_aux_outputs {
    float *depth;          /* [H,W] */
    float *alpha;          /* [H,W] */
    void *ckpt_ws;
} gsr_aux_outputs;
int gsr_aux_workspace_size(const gsr_frame_desc *desc, int64_t binning_capacity, size_t *bytes);
/* gsr_forward_render / gsr_forward that also write aux->depth and aux->alpha (aux NULL: exactly the plain call).  The colour, the
 * radii and the plan are those of the plain call, bit for bit. */
int gsr_forward_render_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                           void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color,
                           const gsr_aux_outputs *aux, void *stream);
int gsr_forward_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                    int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                    gsr_grads *early_fill, const gsr_aux_outputs *aux, void *stream);
/* gsr_backward_render of an aux frame: aux = what its forward was given (depth and ckpt_ws are read, alpha is not);
 * dL_dcolor [3,H,W], dL_ddepth [H,W], dL_dalpha [H,W]: any may be NULL (zero).  screen_grads slot 9 receives dL/dz, the
 * gradient of the Gaussian's view depth.  aux NULL: exactly gsr_backward_render (dL_dcolor required, the other two ignored). */
int gsr_backward_render_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                            const void *image_ws, void *rows_ws, const gsr_frame_plan *plan_host, const float *out_color,
                            const gsr_aux_outputs *aux, const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                            float *screen_grads, void *stream);
/* gsr_backward_geom plus the depth's chain: out->means3D (when not NULL) gains dL/dz (V[0][2], V[1][2], V[2][2]), dL/dz from
 * screen_grads slot 9 (gsr_backward_render_aux), V = viewmatrix as passed. */
int gsr_backward_geom_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                          const int32_t *radii, const void *geom_ws, const float *screen_grads, int32_t g_begin,
                          int32_t g_end, int32_t binned_ranks, const gsr_frame_plan *own_plan, const gsr_grads *out, void *stream);

/* ---- Per-Gaussian blend statistics of a frame (additive: every call above keeps its meaning).  A pixel composites a splat when
 * the blend gives it a weight w = alpha T > 0 (the alpha >= 1/255 test, the 0.99 clamp and the stop rule of the colour image: the
 * event that advances n_contrib).  Per Gaussian g, over every pixel of the frame:
 *   count[g]           += the pixels that composited it
 *   weight_sum_q32[g]  += the sum of its w, in units of 2^-32 (weight_sum = weight_sum_q32 * 2^-32)
 *   weight_max_bits[g]  = max(., the largest single w), as the bits of the binary32 value: w >= 0, so the unsigned bit patterns
 *                         order like the values and the array reads as float [P]
 * The arrays are the caller's, each [P], and are ACCUMULATED INTO, never cleared: zero them once, then call for every camera.  All
 * three are updated with integer atomics (64-bit add, 32-bit max) of per-(tile, Gaussian) totals that are themselves taken in a
 * fixed order, so the same frames give the same bits whatever the tile scheduling, the chunking or the order of the calls.
 * Range: a (tile, Gaussian) total is below 256, so weight_sum_q32 holds 2^32 units of weight per Gaussian before it wraps - a
 * full-screen opaque splat over about 2 000 views at 1920x1080; count holds 2^64 pixels.
 * gsr_forward_render_contrib / gsr_forward_contrib are gsr_forward_render / gsr_forward that also add the frame into *stats
 * (stats NULL: exactly the plain call).  Colour, radii, plan and every workspace are the plain call's, bit for bit: the frame can
 * be followed by its backward.  Whole images only (tile_row_begin = tile_row_end = 0); a slab, or a NULL member with P > 0, is
 * GSR_ERR_INVALID_ARGUMENT before any device work.  A call that stops with GSR_ERR_WORKSPACE in a later depth chunk has already
 * added the earlier chunks: give the frame a binning workspace for num_rendered instances, or keep a copy of the arrays and put it
 * back before the re-run. */
typedef struct gsr_contrib_stats {
    uint64_t *count;             /* [P] */
    uint64_t *weight_sum_q32;    /* [P] */
    uint32_t *weight_max_bits;   /* [P] */
} gsr_contrib_stats;
int gsr_forward_render_contrib(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                               void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color,
                               const gsr_contrib_stats *stats, void *stream);
int gsr_forward_contrib(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                        int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                        gsr_grads *early_fill, const gsr_contrib_stats *stats, void *stream);

/* ---- Error-weighted blend statistics (additive: every call above keeps its meaning).  With a per-pixel error map E in [0, 1], the
 * image error a Gaussian g is responsible for in a view is E_g = sum over the pixels u of w_g(u) E(u), w = alpha T the blend weight
 * above ("Revising Densification in Gaussian Splatting" scores by the maximum of E_g over views, Taming-3DGS by its sum).
 * gsr_forward_render_contrib_error / gsr_forward_contrib_error are the _contrib calls that also add
 *   error_frame_q32[g] += E_g of this frame, in units of 2^-32
 * taken by the same kernel next to the three totals of *stats: per (tile, Gaussian) the products in a fixed order, then one more
 * 64-bit integer atomic add, so the result does not depend on the order of arrival.  pixel_error is read once per tile and depth
 * chunk, clamped to [0, 1] on the way (a NaN reads as 0); it is never written.  Range: E <= 1, so the bound of weight_sum_q32 holds.
 * err NULL: exactly the _contrib call.  err non-NULL: stats is required, as are both members when P > 0, and whole images (a slab is
 * refused as by the _contrib calls); each refusal is GSR_ERR_INVALID_ARGUMENT before any device work.  A frame that bins nothing
 * (P == 0, where both members may be NULL, or num_rendered == 0) reads no map and adds nothing: it runs the _contrib call's kernel.
 * gsr_contrib_error_fold closes a frame: for every g, q = error_frame_q32[g]; error_sum_q32[g] += q; error_max[g] = max(error_max[g],
 * (float)(q 2^-32)); error_frame_q32[g] = 0.  Call it on the same stream behind the frame (behind its LAST call, when a frame that
 * stopped with GSR_ERR_WORKSPACE is run again - restore error_frame_q32 with the arrays of *stats first).  All three arrays are the
 * caller's, [P] each, zeroed once.  P < 0, or a NULL pointer with P > 0, is GSR_ERR_INVALID_ARGUMENT; P == 0 launches nothing. */
typedef struct gsr_contrib_error {
    const float *pixel_error;     /* [H*W] row-major; read clamped to [0,1], NaN as 0 */
    uint64_t *error_frame_q32;    /* [P]  += this frame's sum of w * E, in units of 2^-32 */
} gsr_contrib_error;
int gsr_forward_render_contrib_error(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                                     void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color,
                                     const gsr_contrib_stats *stats, const gsr_contrib_error *err, void *stream);
int gsr_forward_contrib_error(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                              int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                              gsr_grads *early_fill, const gsr_contrib_stats *stats, const gsr_contrib_error *err, void *stream);
int gsr_contrib_error_fold(int64_t P, uint64_t *error_frame_q32, uint64_t *error_sum_q32, float *error_max, void *stream);

/* ---- Gradients for the camera: dL/dviewmatrix [4,4], dL/dprojmatrix [4,4], dL/dcampos [3] (additive: every call above keeps its
 * meaning).  Each is the gradient w.r.t. the tensor as the forward consumed it, in the header's row-vector convention; the three
 * are returned separately and the caller chains them to its own pose parametrisation (the library has none).  Column 3 of
 * dL/dviewmatrix and column 2 of dL/dprojmatrix are exact zeros (the forward never reads those entries); dL/dcampos is zero with
 * colors_precomp.  A clamped tx/tz (ty/tz) contributes nothing through that coordinate, exactly as for means3D.
 * gsr_backward_camera runs behind gsr_backward_geom / gsr_backward_geom_aux of the same frame, with the same screen_grads, and
 * visits the rows that call visits: binned_ranks / own_plan mean what they mean there; depth_chain != 0 (screen_grads came from
 * gsr_backward_render_aux) adds the depth map's chain through slot 9 to dL/dviewmatrix.  The sums over Gaussians are taken in a
 * fixed order (no atomics): the same frame gives the same bits.  workspace: gsr_camera_grad_workspace_size bytes (room for one
 * 27-float partial sum per block of 256 Gaussians, padded to 256 bytes).  A frame with nothing rendered writes zeros.  Whole images only
 * (tile_row_begin = tile_row_end = 0). */
typedef struct gsr_camera_grads {
    float *viewmatrix;     /* [16] */
    float *projmatrix;     /* [16] */
    float *campos;         /* [3]  */
} gsr_camera_grads;        /* any may be NULL (not wanted) */
int gsr_camera_grad_workspace_size(const gsr_frame_desc *desc, size_t *bytes);
int gsr_backward_camera(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                        const void *geom_ws, const float *screen_grads, int32_t binned_ranks, const gsr_frame_plan *own_plan,
                        int32_t depth_chain, void *workspace, const gsr_camera_grads *out, void *stream);

/* ---- Absgrad (AbsGS / Gaussian Opacity Fields; additive: every call above keeps its meaning): per Gaussian, the sum over pixels of
 * the ABSOLUTE value of that pixel's dL/dmean2D, per axis - what the signed sum in slots 0, 1 loses when a splat's pixels pull in
 * opposite directions.  It can only be formed inside the blend backward.
 * gsr_backward_render_abs is gsr_backward_render (same arguments, same work, the same values in slots 0..9) whose screen_grads slots
 * 10 and 11 receive the absolute sums, with the W/2, H/2 factors of slots 0 and 1.  Sums in a fixed order (no atomics): the same
 * frame gives the same bits.  Whole images only (tile_row_begin = tile_row_end = 0). */
int gsr_backward_render_abs(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                            const void *image_ws, void *rows_ws, const gsr_frame_plan *plan_host, const float *out_color,
                            const float *dL_dcolor, float *screen_grads, void *stream);
/* out [P,3] (laid out like gsr_grads.means2D) = (slot 10, slot 11, 0) of screen_grads for the rows gsr_backward_geom visits with
 * the same radii / binned_ranks / own_plan, zeros for every other row: every row of out is written.  Rows of screen_grads outside
 * the binned prefix are not read when that call would not read them (plan_host->screen_prezeroed == 2 never wrote them). */
int gsr_screen_absgrad(const gsr_frame_desc *desc, const int32_t *radii, const void *geom_ws, const float *screen_grads,
                       int32_t binned_ranks, const gsr_frame_plan *own_plan, float *out, void *stream);

/* Device pointers into a frame's geometry workspace (valid after gsr_forward_preprocess):
 *   depth_keys [P]  by Gaussian: the bits of its view depth (a positive binary32: ordered as an integer), 0xFFFFFFFF = not
 *                   visible.  Identical on every rank of a sharded render (visibility is that of the full image).
 *   depth_order [P] the depth order: plan->chunk_rank_begin[c] .. [c+1] holds chunk c's Gaussians, sorted by (depth, index)
 *                   for the chunks gsr_forward_render has run.
 * Either may be NULL (not wanted). */
int gsr_frame_arrays(const gsr_frame_desc *desc, const void *geom_ws, const uint32_t **depth_keys, const uint32_t **depth_order);

/* Multi-GPU gradient exchange (the "allreduce_screen" mode of sharded.py): after the ranks agreed on the largest
 * chunk end any of them binned (key_max, a depth key; n_rows = how many visible Gaussians have key <= key_max: exact, every
 * rank knows it), gather lists those Gaussians in index order (rows[n_rows]) and packs their 48-byte screen-gradient rows
 * (packed[n_rows, 12]) for ONE all-reduce; scatter writes the summed rows back.  Every rank builds the same list: the keys
 * do not depend on its slab.  Uses the frame's selection scratch inside geom_ws (idle after the forward). */
int gsr_exchange_rows_gather(const gsr_frame_desc *desc, void *geom_ws, uint32_t key_max, const float *screen_grads, int32_t n_rows,
                             int32_t *rows, float *packed, void *stream);
int gsr_exchange_rows_scatter(const gsr_frame_desc *desc, int32_t n_rows, const int32_t *rows, const float *packed, float *screen_grads,
                              void *stream);

/* `_C.mark_visible`: present[i] = 1 iff Gaussian i passes the near-plane test (A.1). */
int gsr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix,
                     uint8_t *present, void *stream);

/* Introspection for tests / profiling: copies of intermediate device arrays' ADDRESSES inside the
 * workspaces (no data is copied).  Any out-pointer may be NULL. */
typedef struct gsr_debug_views {
    const float *splat_records;   /* [P,12]: x, y, conicA, conicB, conicC, opacity, r, g, b, depth, packed tile rect (2) */
    const uint32_t *tiles_touched; /* [P,2] by Gaussian: (tiles touched, optical mass in 1/64 pixel-neper units) */
    const uint32_t *depth_order;   /* [P]  depth rank -> Gaussian (invisible ones last)                   */
    const uint32_t *point_offsets; /* [P]  inclusive scan of tiles touched, in depth order               */
    const uint8_t *clamped;        /* [P]  bit c set <=> channel c clamped */
    const uint32_t *sorted_gaussian; /* [<=R] per binned instance (chunks concatenated): Gaussian index in bits 0..27, in bits
                                        28..31 the mask of the tile's 8x8 quadrants the splat can reach (sub-tile culling) */
    const uint32_t *ranges;        /* [GSR_MAX_CHUNKS, Tn, 2] absolute [start, end) per chunk and tile   */
    const float *final_T;          /* [H*W] (negative sign marks a pixel that hit the cut-off)           */
    const int32_t *n_contrib;      /* [H*W] encoded: (chunk + 1) << 26 | position in that chunk's range  */
    const uint32_t *tile_walk;     /* [GSR_MAX_CHUNKS, Tn] entries of chunk c's range the blend backward walks on a tile (its deepest
                                      contributor there); defined where ranges[c][tile] is not empty      */
    const uint32_t *bwd_units;     /* the blend backward's work units (tile | chunk << 24, segment), appended by the forward's waves as they
                                      finish: per shard (= tile % 8) 17 lists, laid out [8][cap_full + 16 cap_part][2]: full segments, then
                                      the pairs' partial last segments in 16 length classes, longest first */
    const uint32_t *bwd_unit_count; /* [8, 17] units per shard and list */
    uint32_t bwd_unit_cap_full, bwd_unit_cap_part;
} gsr_debug_views;
int gsr_debug_get_views(const gsr_frame_desc *desc, const void *geom_ws, const void *binning_ws,
                        const void *image_ws, const gsr_frame_plan *plan_host, gsr_debug_views *views);

/* ---- the loss of the reference's timed window (train.py:104-105), fused.
 * loss = (1 - lambda) * mean|image - target| + lambda * (1 - mean SSIM(image, target)), SSIM exactly as
 * utils/loss_utils.py:33-63 (11x11 Gaussian window sigma 1.5, depthwise, zero padding, C1 = 1e-4, C2 = 9e-4).
 * image/target: [channels, H, W] fp32.  forward writes out3 = (loss, l1, ssim) (device) and keeps the
 * per-pixel SSIM derivatives in `workspace` for the backward; backward writes grad_image =
 * upstream[0] * dloss/dimage (upstream: device scalar, NULL = 1). */
int gsr_loss_workspace_size(int32_t channels, int32_t height, int32_t width, size_t *bytes);
int gsr_loss_l1_ssim_forward(int32_t channels, int32_t height, int32_t width, float lambda_dssim, const float *image,
                             const float *target, void *workspace, float *out3, void *stream);
int gsr_loss_l1_ssim_backward(int32_t channels, int32_t height, int32_t width, float lambda_dssim, const float *upstream,
                              const float *image, const float *target, const void *workspace, float *grad_image,
                              void *stream);
/* The two terms on their own, for a caller that composes the loss itself exactly as train.py:104-105 does
 * (Ll1 = l1_loss(image, gt); loss = (1 - lambda) * Ll1 + lambda * (1 - ssim(image, gt))): gsr_loss_l1_ssim_forward's
 * out3[1] / out3[2] ARE l1_loss / ssim of utils/loss_utils.py:17-18,33-63; d ssim / d image is gsr_loss_l1_ssim_backward
 * with lambda_dssim = 1 and the upstream negated; d l1_loss / d image = upstream[0] * sign(image - target) / n is this: */
int gsr_loss_l1_backward(int64_t n, const float *upstream, const float *image, const float *target, float *grad_image,
                         void *stream);
/* Multi-GPU slab variants (SURVEY 8e "slab-local loss"): this rank owns image rows [row_begin, row_end) of a
 * full-size image whose rows within 10 of the slab are valid.  forward_rows writes out2 = (sum |image - target|,
 * sum of the SSIM map) over the slab's rows — un-normalised: the caller adds the ranks' pairs and forms
 * loss = (1 - lambda) * l1 / n + lambda * (1 - ssim / n), n = channels * height * width — and the derivative
 * maps of the slab plus 5 rows either side.  backward_rows writes grad_image rows [row_begin, row_end) only:
 * the full d loss / d image of those rows (window contributions from the neighbouring slabs included). */
int gsr_loss_l1_ssim_forward_rows(int32_t channels, int32_t height, int32_t width, const float *image, const float *target,
                                  void *workspace, float *out2, int32_t row_begin, int32_t row_end, void *stream);
int gsr_loss_l1_ssim_backward_rows(int32_t channels, int32_t height, int32_t width, float lambda_dssim, const float *upstream,
                                   const float *image, const float *target, const void *workspace, float *grad_image,
                                   int32_t row_begin, int32_t row_end, void *stream);

/* ---- `simple_knn._C.distCUDA2` (scene/gaussian_model.py:144-145): mean of the squared
 * distances from each point to its 3 nearest other points (exact), used once to initialise the scales.
 * xyz[P,3] -> mean_dist2[P]. */
int gsr_dist2_workspace_size(int32_t P, size_t *bytes);
int gsr_dist2_knn3(int32_t P, const float *xyz, float *mean_dist2, void *workspace, void *stream);

/* ---- one torch.optim.Adam step (no weight decay / amsgrad; the reference uses eps = 1e-15,
 * scene/gaussian_model.py:173) over n contiguous fp32 elements in a single pass.  step = 1 for the first update.
 * This call and gsr_adam_step_split are gsr_adam_step_multi with one tensor (row_len = 0; row_len and split): same kernel, same bits. */
int gsr_adam_step(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                  float beta2, float eps, int64_t step, void *stream);
/* The same step over `rows` rows of `row_len` >= 4 contiguous elements whose first `split` elements use
 * lr_head and the rest lr_tail: the interleaved SH table [P, M, 3] (row_len = 3 M, split = 3), which stands for the
 * reference's two tensors _features_dc (lr = feature_lr) and _features_rest (lr = feature_lr / 20,
 * scene/gaussian_model.py:166-168).  Element for element the result equals two gsr_adam_step calls on the two tensors. */
int gsr_adam_step_split(int64_t rows, int32_t row_len, int32_t split, float *param, const float *grad, float *exp_avg,
                        float *exp_avg_sq, float lr_head, float lr_tail, float beta1, float beta2, float eps, int64_t step,
                        void *stream);

/* The whole optimizer step in ONE launch: up to GSR_ADAM_MAX_TENSORS tensors, each with its own learning rate(s) and step
 * count (the reference's six groups: five tensors here, the SH table with split rows).  tensors: HOST array.  Element for
 * element what the per-tensor calls compute. */
#define GSR_ADAM_MAX_TENSORS 8
typedef struct gsr_adam_tensor {
    float *param; const float *grad; float *exp_avg; float *exp_avg_sq;
    int64_t n;                  /* elements */
    float lr, lr_tail;          /* lr_tail: for elements [split, row_len) of every row (row_len > 0) */
    int64_t step;               /* this tensor's step count (>= 1), for the bias corrections */
    int32_t row_len, split;     /* row_len == 0: one learning rate for the whole tensor */
} gsr_adam_tensor;
int gsr_adam_step_multi(int32_t count, const gsr_adam_tensor *tensors, float beta1, float beta2, float eps, void *stream);

/* The same step over the rows a frame saw (upstream's optimizer_type = "sparse_adam"), still ONE launch.  Every tensor has `rows`
 * rows: n = rows * w with a width w >= 1 of its own, and row_len is 0 or w.  visible: DEVICE array of one entry per row, of
 * visible_elem_bytes = 1 (bool / uint8, non-zero = visible) or 4 (int32, > 0 = visible: the rasterizer's radii as they are).
 * An element of a visible row steps exactly as in gsr_adam_step_multi (an all-visible mask gives the same bits); of a hidden row,
 * param, exp_avg and exp_avg_sq keep their bits and grad is not read.  `step` counts every call, whatever the mask showed: it
 * enters the bias corrections only.  step = GSR_ADAM_STEP_UNCORRECTED applies none (step size lr, second moment as it is), which is
 * upstream's arithmetic.  rows == 0, count == 0 and an all-hidden mask touch nothing. */
#define GSR_ADAM_STEP_UNCORRECTED INT64_MAX
int gsr_adam_step_sparse_multi(int32_t count, const gsr_adam_tensor *tensors, int64_t rows,
                               const void *visible, int32_t visible_elem_bytes,
                               float beta1, float beta2, float eps, void *stream);

/* ---- the activations between the optimizer's raw parameters and the rasterizer's inputs, the
 * getters of scene/gaussian_model.py:101-125 (setup_functions :47-60):
 *   scales [P,3] = exp(scaling_raw)   rotations [P,4] = rotation_raw / max(|rotation_raw|_2, 1e-12)   opacities [P] = sigmoid(opacity_raw)
 * in one launch; a NULL input skips that tensor (its output must be NULL too).  Pointers 16-byte aligned. */
int gsr_activations_forward(int64_t P, const float *scaling_raw, const float *rotation_raw, const float *opacity_raw, float *scales,
                            float *rotations, float *opacities, void *stream);
/* Their backward in one launch: scales / opacities are the FORWARD OUTPUTS, rotation_raw the forward input.  A NULL
 * dL_d*_raw output skips that tensor. */
int gsr_activations_backward(int64_t P, const float *scales, const float *rotation_raw, const float *opacities,
                             const float *dL_dscales, const float *dL_drotations, const float *dL_dopacities,
                             float *dL_dscaling_raw, float *dL_drotation_raw, float *dL_dopacity_raw, void *stream);

/* ---- The latent structured model's composition (scene/latent_gaussian_model.py: LatentGaussianModel.forward), additive: every
 * call above keeps its meaning.  B structures each carry a mean [3], an opacity logit, a log-scale [3] and a raw rotation [4]; a
 * decoder gives every structure K children of D = 11 + 3 sh_coeffs floats: decoded [B, K D] contiguous, child k of structure b =
 * decoded[b, k D : (k + 1) D] = (xyz[3], opacity, scale[3], rotation[4], SH [sh_coeffs, 3]).  For child p = b K + k with row c:
 *   xyz[p] = c[0:3] + means[b]    opacity[p] = c[3] + opacities[b]    scaling[p] = c[4:7] + scales[b]       (one fp32 add each)
 *   rotation[p] = std(n(rotations[b]) (x) n(c[7:11]))    n(v) = v / max(|v|_2, 1e-12);  (x) = Hamilton product, real part first;
 *                                                        std(q) = -q where q_w < 0 (q_w == 0 is kept)
 *   features[p] = c[11 : 11 + 3 sh_coeffs]                                                                   (a copy)
 * The outputs are what gsr_gaussians takes with raw == 2 (means3D, opacities, scales, rotations, shs), P = B K of them.
 * One launch forward, one backward; no workspace, no host synchronisation, no state.  The backward recomputes what it needs from
 * decoded and rotations.  Every wanted gradient is written in full: a NULL incoming gradient counts as zeros.  A structure's
 * gradient is the sum over its K children taken in ascending k, ((g_0 + g_1) + g_2) + ..., without atomics: the same inputs give
 * the same bits.  B >= 0 (0: nothing is launched), K >= 1, sh_coeffs in {1, 4, 9, 16}, B K < 2^28.  The child tensors and their
 * gradients must be 16-byte aligned (decoded and its gradient: 4). */
typedef struct gsr_structured_desc { int32_t B, K, sh_coeffs; } gsr_structured_desc;
typedef struct gsr_structures {        /* [B,3] [B] [B,3] [B,4] */
    const float *means, *opacities, *scales, *rotations;
} gsr_structures;
typedef struct gsr_children {          /* [P,3] [P] [P,3] [P,4] [P,sh_coeffs,3] */
    float *xyz, *opacity, *scaling, *rotation, *features;
} gsr_children;
typedef struct gsr_children_grads {    /* incoming gradients, shaped as gsr_children; NULL = zero */
    const float *xyz, *opacity, *scaling, *rotation, *features;
} gsr_children_grads;
typedef struct gsr_structured_grads {  /* decoded [B, K D], the rest shaped as gsr_structures; NULL = not wanted */
    float *decoded, *means, *opacities, *scales, *rotations;
} gsr_structured_grads;
int gsr_structured_compose_forward(const gsr_structured_desc *desc, const float *decoded, const gsr_structures *structures,
                                   const gsr_children *out, void *stream);
int gsr_structured_compose_backward(const gsr_structured_desc *desc, const float *decoded, const gsr_structures *structures,
                                    const gsr_children_grads *grads_in, const gsr_structured_grads *out, void *stream);

/* ---- Anti-aliasing as an opacity compensation (upstream's `antialiasing` switch, the 2D filter of Mip-Splatting), additive: every
 * call above keeps its meaning, and the rasterizer itself does not change.  The forward low-passes every splat by adding
 * h = GSR_COV2D_DILATE (0.3 px^2) to the diagonal of its 2D covariance; the radius, the binning rectangle and the conic keep that
 * dilated covariance.  This op, run IN FRONT of the forward, scales the opacity so that the splat keeps its energy:
 *   det0 = a0 c0 - b^2     det1 = (a0 + h)(c0 + h) - b^2     (a0, b, c0: the 2D covariance BEFORE the dilation, same frustum clamp of
 *                                                             tx/tz, ty/tz and same scale_modifier as the preprocess)
 *   x = det0 / det1        rho = sqrt(max(GSR_AA_MIN_RATIO, x))        opacities_out[i] = opacities[i] rho
 * A Gaussian the preprocess culls before it has a covariance (view z <= GSR_NEAR_CUT), or one with det1 == 0, passes through:
 * opacities_out[i] = opacities[i], dL/dopacities[i] = grad_opacities_out[i], its other gradients are zero.  Where x is clamped
 * the geometry gradients are zero too.  g->raw != 0: opacities are logits, scales log-scales, rotations unnormalised (activated as
 * in the per-Gaussian kernels); opacities_out is then the LOGIT of sigmoid(opacities) rho and the gradients are those on the raw
 * tensors.  Read: desc (P, width, height, tanfovx, tanfovy, scale_modifier, debug), cam->viewmatrix, g->means3D, opacities, scales,
 * rotations (16-byte aligned), raw; the rest is ignored, except that g->cov3D_precomp != NULL is GSR_ERR_INVALID_ARGUMENT.
 * The backward takes grad_opacities_out [P] = dL/dopacities_out and writes grads->means3D [P,3], opacities [P], scales [P,3],
 * rotations [P,4] (any may be NULL: not wanted; the other fields of gsr_grads are ignored) in full; no gradient is returned for the
 * view matrix.  One launch each; every row depends on its own inputs only (no atomics): the same inputs give the same bits. */
int gsr_opacity_compensation_forward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, float *opacities_out,
                                     void *stream);
int gsr_opacity_compensation_backward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                                      const float *grad_opacities_out, const gsr_grads *grads, void *stream);

/* ---- The latent structured model's decoder (scene/latent_gaussian_model.py: Decoder), additive: every call above keeps its
 * meaning.  For each of B structures, with x = (pos_emb[b], latents[b]) of in_size floats (the positional dims in FRONT):
 *   h1 = relu(w0 x + b0)      h2 = relu((w1 h1 + b1) + h1)      decoded[b] = w2 h2 + b2
 * Weights have nn.Linear's layout: w0 [hidden, in_size], w1 [hidden, hidden], w2 [out_size, hidden], biases [rows].  pos_emb is
 * [B, in_size - latent_size], NULL exactly when in_size == latent_size; latents [B, latent_size]; decoded [B, out_size]; all
 * contiguous fp32.  Supported: hidden_size == 32, 1 <= latent_size <= in_size <= 128, 1 <= out_size <= 2^20, 0 <= B <= 2^30 (0: nothing is
 * launched); anything else is GSR_ERR_INVALID_ARGUMENT.  w1 and w2 must be 16-byte aligned.  Every product is an exact-f32 MFMA:
 * a fused multiply-add chain in ascending k that starts from the bias.
 * The backward recomputes h1 and h2 from the inputs (the forward saves nothing) and passes a gradient where the pre-activation is
 * > 0.  d_decoded [B, out_size] is required; pos_emb gets no gradient.  Each field of gsr_decoder_grads may be NULL (not wanted:
 * it costs nothing); the wanted ones are written in full.  The weight and bias gradients are sums over B: every block of
 * k_decoder_bwd walks a contiguous range of structures in ascending order and writes one partial to `workspace`
 * (gsr_decoder_workspace_size bytes, a function of the desc only; 16-byte aligned; may be NULL when only grads->latents is
 * wanted), and k_decoder_reduce adds the partials in ascending block order.  No atomics: the same inputs give the same bits. */
typedef struct gsr_decoder_desc   { int32_t B, in_size, latent_size, hidden_size, out_size; } gsr_decoder_desc;
typedef struct gsr_decoder_params { const float *w0, *b0, *w1, *b1, *w2, *b2; } gsr_decoder_params; /* nn.Linear layouts: w [out,in] */
typedef struct gsr_decoder_grads  { float *latents, *w0, *b0, *w1, *b1, *w2, *b2; } gsr_decoder_grads; /* NULL = not wanted */
int gsr_decoder_workspace_size(const gsr_decoder_desc *desc, size_t *bytes);
int gsr_decoder_forward(const gsr_decoder_desc *desc, const float *pos_emb, const float *latents, const gsr_decoder_params *params,
                        float *decoded, void *stream);
int gsr_decoder_backward(const gsr_decoder_desc *desc, const float *pos_emb, const float *latents, const gsr_decoder_params *params,
                         const float *d_decoded, const gsr_decoder_grads *grads, void *workspace, size_t workspace_bytes, void *stream);

/* ---- The MCMC densification strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy), additive: every
 * call above keeps its meaning.  The tensors are the raw parameters: opacity_raw [P] logits, scaling_raw [P,3] logs, rotation_raw
 * [P,4] unnormalised quaternions, xyz [P,3]; o = sigmoid(opacity_raw), s = exp(scaling_raw), q^ = q / max(|q|, 1e-12).
 *
 * gsr_mcmc_relocation: sampled [n] (int64, DEVICE, every entry in [0, P): not checked) lists the sources, one entry per Gaussian
 * that is to become a copy of it.  With N_j = min(GSR_MCMC_MAX_RATIO, 1 + occurrences of sampled[j] in sampled), and o, s of the
 * source BEFORE the call:
 *   o' = 1 - (1 - o)^(1/N)      D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k (k+1)^(-1/2) o'^(k+1)
 *   new_opacity_raw[j] = logit(clamp(o', min_opacity, 1 - 2^-23))      new_scaling_raw[j, :] = scaling_raw[sampled[j], :] + log(o / D)
 * (the clamp comes after D).  Evaluated in binary64 and rounded to binary32 once: the alternating sum loses up to 8e-5 in binary32.
 * workspace: gsr_mcmc_relocation_workspace_size(P) bytes, 4-byte aligned, contents irrelevant before and after (occurrence counters,
 * summed with integer atomics: the result does not depend on their order).  Only the two outputs are written.  Three launches over
 * n, none over P; no host synchronisation.  0 < min_opacity < 1.  P == 0 or n == 0: nothing is launched. */
int gsr_mcmc_relocation_workspace_size(int64_t P, size_t *bytes);
int gsr_mcmc_relocation(int64_t P, int64_t n, const float *opacity_raw, const float *scaling_raw, const int64_t *sampled,
                        float min_opacity, void *workspace, float *new_opacity_raw, float *new_scaling_raw, void *stream);

/* gsr_mcmc_relocate_rows: applies the result of gsr_mcmc_relocation (same sampled, same stream or ordered behind it) to up to
 * GSR_MCMC_MAX_TENSORS tensors of P rows.  tensors: HOST array; tensor t has `width` >= 1 contiguous floats per row and a role:
 *   GSR_MCMC_ROLE_OPACITY (width 1):  param[sampled[j]] = new_opacity_raw[j]
 *   GSR_MCMC_ROLE_SCALING (width 3):  param[sampled[j], :] = new_scaling_raw[j, :]
 *   GSR_MCMC_ROLE_COPY:               source rows keep their values
 * dead != NULL ([n] int64, DEVICE, distinct rows, none of them in sampled): row dead[j] of every tensor becomes row sampled[j] as it
 * is after the call (copied values bit for bit), and exp_avg / exp_avg_sq (both or neither NULL) of every SOURCE row are set to
 * zero; the dead rows' moments are left alone.  dead == NULL (growth: the caller appends the copies itself): only the new values
 * are written, no moment is touched.  ONE launch whatever n, P and count are; it reads nothing that it writes, a source listed k
 * times is written k times with one value, so the result does not depend on thread order.  P == 0, n == 0 or count == 0: nothing
 * is launched. */
#define GSR_MCMC_MAX_TENSORS 8
#define GSR_MCMC_ROLE_COPY    0
#define GSR_MCMC_ROLE_OPACITY 1
#define GSR_MCMC_ROLE_SCALING 2
typedef struct gsr_mcmc_tensor {
    float *param; float *exp_avg; float *exp_avg_sq;      /* [P, width]; the moments: both or neither NULL */
    int32_t width, role;
} gsr_mcmc_tensor;
int gsr_mcmc_relocate_rows(int32_t count, const gsr_mcmc_tensor *tensors, int64_t P, int64_t n, const int64_t *sampled,
                           const int64_t *dead, const float *new_opacity_raw, const float *new_scaling_raw, void *stream);

/* gsr_mcmc_inject_noise: xyz[i] += R(q^_i) diag(s_i^2) R(q^_i)^T (noise[i] g(o_i) c),  g(o) = 1 / (1 + exp(100 o - 0.5)), in
 * place; noise [P,3] is the caller's standard-normal draw, c a host scalar (noise_lr x the position learning rate).  Where the
 * exponential overflows g is 0 and the row keeps xyz + 0.  One launch, 56 B read and 12 B written per Gaussian, every row from its
 * own inputs (no atomics): the same inputs give the same bits.  All five tensors 16-byte aligned.  P == 0: nothing is launched.
 *
 * gsr_mcmc_reg_grads: the gradient of lambda_opacity mean(o) + lambda_scale mean(s) added in place:
 *   grad_opacity[i] += lambda_opacity / P o_i (1 - o_i)        grad_scaling[i, j] += lambda_scale / (3 P) s_ij
 * Either gradient may be NULL (its lambda and raw tensor are then ignored); a given one and its raw tensor are 16-byte aligned.
 * One launch.  The loss value itself is not computed. */
int gsr_mcmc_inject_noise(int64_t P, float *xyz, const float *scaling_raw, const float *rotation_raw, const float *opacity_raw,
                          const float *noise, float c, void *stream);
int gsr_mcmc_reg_grads(int64_t P, const float *opacity_raw, const float *scaling_raw, float lambda_opacity, float lambda_scale,
                       float *grad_opacity, float *grad_scaling, void *stream);

/* ---- The per-image bilateral grid (gsplat's lib_bilagrid): every training image
 * owns a grid of 3x4 affine colour transforms indexed by pixel position and luma, and the rendered image goes through its grid
 * before the loss.  grids is [N, 12, L, Gy, Gx] (gsplat's layout), image / out / grad_out / grad_image are [3, H, W], all contiguous
 * fp32; idx in [0, N) picks the grid.  For pixel (py, px) with in = (r, g, b, 1):
 *   fx = (px + 0.5) / W (Gx - 1)    fy = (py + 0.5) / H (Gy - 1)    fz = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1)
 *   per axis  i0 = clamp(floor f, 0, G - 1), i1 = min(i0 + 1, G - 1), t = f - i0  (an axis of size 1: t = 0)
 *   A_k = sum over the 8 corners of w grids[idx, k, z, y, x],  w = the product of the three (1 - t | t) factors
 *   out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3]
 * which is torch's grid_sample(mode="bilinear", padding_mode="border", align_corners=True) on a 5-D input and the affine product.
 *
 * gsr_bilagrid_forward: one launch.  gsr_bilagrid_backward: grad_grids [N, 12, L, Gy, Gx] (dense: the rows of every image but idx
 * are written as zero) and grad_image, either may be NULL (both NULL: nothing is launched).  One launch for grad_image and the
 * per-block partial sums of grad_grids (in `workspace`, backward_bytes of gsr_bilagrid_workspace_size; not read when grad_grids is
 * NULL), one that adds the partials in a fixed order.  The luma term of grad_image is zero where the luma is outside (0, 1).  No
 * floating-point atomics: the same inputs give the same bits.
 *
 * gsr_bilagrid_tv_forward: out[0] = the sum, over the grid axes (x, y, luma) longer than 1, of the mean squared forward difference
 * along the axis (gsplat's total_variation_loss; an axis of size 1 adds 0).  One launch.  `workspace` is tv_bytes of
 * gsr_bilagrid_workspace_size; its bytes must be ZERO before the first call and every call puts its ticket word back to zero, so a
 * workspace cleared once serves any number of calls, one in flight at a time.  gsr_bilagrid_tv_backward: grad_grids = grad_out[0]
 * d tv / d grids, one launch, every element gathered from its six neighbours.
 *
 * Every size of the grid is 1 .. 1024 and N 12 L Gy Gx < 2^31; H, W are 0 .. 32768 and H W == 0 returns GSR_OK with nothing
 * launched.  Arguments are checked before anything touches the device. */
int gsr_bilagrid_workspace_size(int32_t H, int32_t W, int32_t L, int32_t Gy, int32_t Gx, size_t *backward_bytes, size_t *tv_bytes);
int gsr_bilagrid_forward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, int32_t H, int32_t W, int32_t idx, const float *grids,
                         const float *image, float *out, void *stream);
int gsr_bilagrid_backward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, int32_t H, int32_t W, int32_t idx, const float *grids,
                          const float *image, const float *grad_out, float *grad_grids, float *grad_image, void *workspace,
                          size_t workspace_bytes, void *stream);
int gsr_bilagrid_tv_forward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, const float *grids, void *workspace, float *out,
                            void *stream);
int gsr_bilagrid_tv_backward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, const float *grids, const float *grad_out,
                             float *grad_grids, void *stream);

/* ---- Vector quantisation (csrc/gsr_vq.hip): Lloyd's two steps for a table x [P, D] against a codebook
 * [K, D], all contiguous fp32 device arrays.  What scene/compression.py clusters the higher-order SH rows with.
 *
 * gsr_vq_assign: idx[p] (int32) = the code nearest to x_p in squared Euclidean distance, ties to the LOWEST index, and dist2[p]
 * (fp32) that distance.  Per (point, code) the kernel evaluates  score = |c|^2 - 2 x.c  as one fmaf of the dot product and the
 * code's norm, takes the minimum, and returns  dist2 = max(0, |x|^2 + score).  The dot product is a k-ascending binary32 fmaf chain
 * from 0 (v_mfma_f32_32x32x2_f32), each norm the same chain of the row with itself, so with
 *   B(p) = (D + 4) 2^-24 (|x_p| + max_k |c_k|)^2
 * the chosen code is within 2 B(p) of the true minimum distance and dist2[p] within B(p) of the true distance to the chosen code
 * (DESIGN.md section 18 derives the count); a point that equals a code bit for bit gets dist2 == 0.  Distances lose digits when the
 * cloud sits far from the origin (B grows with the norms): centre the table first, as diff_gaussian_rasterization.vq.kmeans does.
 * The P x K distances are never written.  Two launches (the codes' norms into the workspace, the fused product + argmin).  x and
 * codebook are only read.  P == 0 returns GSR_OK with nothing launched.
 *
 * gsr_vq_update: new_codebook[k] = the mean of the rows x_p with idx[p] == k, counts[k] (int32) their number; a code without a
 * member keeps codebook[k] bit for bit; an idx[p] outside [0, K) is no one's member.  The rows of a code are added one by one in
 * ascending p (the library's stable radix sort of (idx, p) puts them in one run) and divided by the count: no floating-point
 * atomics, the same inputs give the same bits.  new_codebook may be codebook itself.
 *
 * `workspace`: gsr_vq_workspace_size(P, K, D) bytes, 16-byte aligned, scratch (one size serves both calls; nothing is kept between
 * calls).  1 <= D <= 128, 1 <= K <= 2^30, 0 <= P <= 2^30: anything else is refused with the argument's name in gsr_last_error(),
 * before anything touches the device.  Non-finite inputs are the caller's business. */
int gsr_vq_workspace_size(int64_t P, int32_t K, int32_t D, size_t *bytes);
int gsr_vq_assign(int64_t P, int32_t K, int32_t D, const float *x, const float *codebook, int32_t *idx, float *dist2,
                  void *workspace, size_t workspace_bytes, void *stream);
int gsr_vq_update(int64_t P, int32_t K, int32_t D, const float *x, const int32_t *idx, const float *codebook,
                  float *new_codebook, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream);

/* ---- Mip-Splatting's 3D smoothing filter (the world-space half of its anti-aliasing; the 2D half is the opacity compensation
 * above), additive: every call above keeps its meaning.  DESIGN.md section 19.
 *
 * gsr_filter3d_compute: `cameras` is a device table [C,16] of floats, 16-byte aligned: per camera the 12 entries of its row-vector
 * view matrix V that the rule reads, coordinate by coordinate (V00 V10 V20 V30, V01 V11 V21 V31, V02 V12 V22 V32), then fx, fy, W,
 * H (focal lengths and image size in pixels).  For Gaussian p with (x, y, z) = xyz_p V[:3,:3] + V[3,:3]:
 *   valid(p,c) = z > GSR_NEAR_CUT  and  |x fx| <= (0.5 + GSR_F3D_MARGIN) W z  and  |y fy| <= (0.5 + GSR_F3D_MARGIN) H z
 *   d_p = min over the valid cameras of z;  a Gaussian no camera saw takes the maximum d over the others
 *   filter_out[p] = d_p sqrt(GSR_F3D_VARIANCE) / focal_max          (focal_max: the largest fx of the table, the caller's number)
 * min and max are exact: the same inputs give the same bits, in any order of the cameras.  Two launches whatever C is.
 * `workspace`: gsr_filter3d_workspace_size(P) bytes, 4-byte aligned, scratch.  any_seen (host pointer, may be NULL): when given, the
 * call synchronises the stream and writes 1 if any Gaussian was seen by any camera, else 0 (every filter_out is then 0); NULL: no
 * synchronisation.  xyz [P,3] and filter_out [P] need 4-byte alignment.
 *
 * gsr_filter3d_apply_forward, with f = filter[p], per axis s' = sqrt(s^2 + f^2) and o' = o sqrt(prod s^2 / prod s'^2):
 *   raw == 0: opacities [P] and scales [P,3] are activated, so are the outputs;
 *   raw != 0: logits and log-scales in, the logit of o' and log s' out (what the raw mode of gsr_gaussians takes).
 * A row with f <= 0 passes through bit for bit.  gsr_filter3d_apply_backward recomputes from the same inputs; grad_opacities_out [P]
 * and grad_scales_out [P,3] are the incoming gradients (NULL = zero), grad_opacities [P] and grad_scales [P,3] the results (NULL =
 * not wanted, both NULL: nothing runs).  No gradient goes to the filter.  One launch each, no atomics: the same inputs give the same
 * bits.  All pointers need 4-byte alignment.
 *
 * Refused with the argument's name in gsr_last_error(), before anything touches the device: P < 0 or P > 2^30, C <= 0, a focal_max
 * that is not positive and finite, a required pointer that is NULL, a misaligned pointer, a workspace that is too small.  P == 0
 * returns GSR_OK and reads nothing. */
int gsr_filter3d_workspace_size(int64_t P, size_t *bytes);
int gsr_filter3d_compute(int64_t P, int32_t C, const float *cameras, float focal_max, const float *xyz, float *filter_out,
                         void *workspace, size_t workspace_bytes, int32_t *any_seen, void *stream);
int gsr_filter3d_apply_forward(int64_t P, int32_t raw, const float *opacities, const float *scales, const float *filter,
                               float *opacities_out, float *scales_out, void *stream);
int gsr_filter3d_apply_backward(int64_t P, int32_t raw, const float *opacities, const float *scales, const float *filter,
                                const float *grad_opacities_out, const float *grad_scales_out, float *grad_opacities,
                                float *grad_scales, void *stream);

/* ---- the densification bookkeeping of one training iteration (train.py:127-130,
 * scene/gaussian_model.py:415-417) in one pass without a host synchronisation: for every Gaussian with
 * radii[i] > 0:  max_radii2D[i] = max(max_radii2D[i], radii[i]);  xyz_gradient_accum[i] += |viewspace_grad[i, :2]|;
 * denom[i] += 1.  viewspace_grad is [P,3] (the means2D gradient of the rasterizer). */
int gsr_densify_stats(int32_t P, const int32_t *radii, const float *viewspace_grad, float *max_radii2D,
                      float *xyz_gradient_accum, float *denom, void *stream);

/* Test hook for the hand-written radix sort (csrc/gsr_sort.hip): stable sort of n (key, value) u32 pairs on
 * key bits [0, end_bit).  keys0/vals0 hold the input; *result_buffer says which pair of buffers holds the
 * output.  count_on_device != 0 reads n from a device word (as the progressive binning does). */
int gsr_debug_sort_temp_bytes(size_t *bytes);
int gsr_debug_sort_pairs(uint32_t *keys0, uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, int64_t n, int32_t end_bit,
                         int32_t count_on_device, void *temp, int32_t *result_buffer, void *stream);
/* The same sort as the per-chunk tile sort calls it: the count n and the base offset are read from the device; n_max (>= n)
 * sizes the grid and picks the scatter variant (>= 4 Mi: the LDS-reordering one); pairs live at [base, base + n) of each
 * buffer; vals2_0 / vals2_1 (both or neither) is a second payload that travels with vals; even_passes != 0 returns the result
 * in buffer 0 whatever the pass count.  temp: gsr_debug_sort_temp_bytes. */
int gsr_debug_sort_pairs_ex(uint32_t *keys0, uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, uint32_t *vals2_0, uint32_t *vals2_1,
                            int64_t n, int64_t n_max, int64_t base, int32_t end_bit, int32_t even_passes, void *temp,
                            int32_t *result_buffer, void *stream);

/* Per-kernel device timing (hipEvent pairs recorded on the caller's stream around every kernel this
 * library launches, from any thread).  Off by default; the only process-wide state of the library,
 * mutex-protected, meant for benchmarks (one frame in flight).  gsr_profile_enable(1) resets the
 * accumulators.  gsr_profile_read synchronises the recorded events and returns up to `max_entries`
 * (name, total milliseconds, launch count) rows; returns the number of rows written. */
#define GSR_PROFILE_NAME_LEN 32
int gsr_profile_enable(int enable);
int gsr_profile_read(int max_entries, char (*names)[GSR_PROFILE_NAME_LEN], float *total_ms, int32_t *launches);

/* Normal maps for surface regularisation (per-Gaussian normals, depth normals, the normal-consistency loss): the entry points are
 * part of this ABI and of libgsrast.so, declared in a header of their own that this one brings in. */
#include "gsrast_normals.h"

/* A second colour triple inside the colour frame (three per-Gaussian values blended with the colour's weights, differentiable): the
 * entry points are part of this ABI and of libgsrast.so, declared in a header of their own that this one brings in. */
#include "gsrast_extra.h"

/* The median depth map of an aux frame (the depth of the splat at which a pixel's accumulated opacity crosses one half, differentiable
 * in that splat's depth): the entry points are part of this ABI and of libgsrast.so, declared in a header of their own. */
#include "gsrast_median.h"

/* TSDF fusion of depth maps and mesh extraction by surface nets: the entry points are part of this ABI and of libgsrast.so, declared
 * in a header of their own that this one brings in. */
#include "gsrast_tsdf.h"

/* Mesh cleaning (connected components of a triangle mesh, removal of small pieces and of unused vertices): the entry points are part
 * of this ABI and of libgsrast.so, declared in a header of their own that this one brings in. */
#include "gsrast_mesh.h"

/* The depth-distortion loss (per-Gaussian depth moments, the distortion map of a rendered moments map, its mean as a fused loss): the
 * entry points are part of this ABI and of libgsrast.so, declared in a header of their own that this one brings in. */
#include "gsrast_distortion.h"

/* The sparse (brick-allocated) TSDF volume: allocation from depth maps, fusion and mesh extraction over the allocated bricks alone.
 * The entry points are part of this ABI and of libgsrast.so, declared in a header of their own that this one brings in. */
#include "gsrast_tsdf_sparse.h"

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_H */
