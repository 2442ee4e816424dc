/* gsrast_median.h — the median depth map of an aux frame (included by gsrast.h; its conventions hold: device pointers, contiguous
 * fp32, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * A "median" frame is an aux frame (gsr_forward_aux: colour, radii, depth, alpha - all bit for bit those of the aux call) whose blend
 * also selects, per pixel, the depth of the splat at which the accumulated opacity crosses one half.  Over the
 * splats the colour composites (the alpha >= 1/255 test, the 0.99 clamp, the stop rule; the stopping splat is not composited), with
 * T_i the blend's own float32 transmittance in front of splat i (the value that multiplies alpha_i to form w_i):
 *     median = z_m,  m = the LAST composited splat with T_m > 0.5,  z the view depth the depth map blends
 * A pixel with a composited splat always has one (the first has T = 1); where the opacity never reaches one half it is the farthest
 * composited splat.  A pixel nothing composited gets +0.0.  Not normalised, no background term: mask by alpha.
 * median:     [H,W] float, written by the forward.
 * median_enc: [H,W] int32, written by the forward, read by the backward: which list entry the median is
 *             ((chunk + 1) << 26 | position in the chunk's tile list + 1; 0 = none).  Opaque to callers.
 * aux:        as for gsr_forward_aux (the same one-plane ckpt_ws: the median needs no checkpoint).  Required.
 * Whole images only (tile_row_begin = tile_row_end = 0).  No atomic is used: the same frame gives the same bits.
 */
#ifndef GSRAST_MEDIAN_H
#define GSRAST_MEDIAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* gsr_forward_render_aux / gsr_forward_aux that also write median and median_enc. */
int gsr_forward_render_median(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                              void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color,
                              const gsr_aux_outputs *aux, float *median, int32_t *median_enc, void *stream);
int gsr_forward_median(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                       int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                       gsr_grads *early_fill, const gsr_aux_outputs *aux, float *median, int32_t *median_enc, void *stream);

/* gsr_backward_render_aux of a median frame.  aux, median_enc: what its forward was given / wrote.  dL_dcolor [3,H,W], dL_ddepth
 * [H,W], dL_dalpha [H,W], dL_dmedian [H,W]: any may be NULL (zero).  The selection is piecewise constant: dL_dmedian of a pixel is
 * added to dL/dz of that pixel's median splat and to nothing else (not to opacity, conic, means2D or colour).  screen_grads as
 * gsr_backward_render_aux leaves it (slot 9 = dL/dz, now including the median's share); gsr_backward_geom_aux (and
 * gsr_backward_camera with depth_chain) follow as for an aux frame.  With dL_dmedian NULL the result is gsr_backward_render_aux's,
 * bit for bit. */
int gsr_backward_render_median(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                               const void *image_ws, void *rows_ws, const gsr_frame_plan *plan_host, const float *out_color,
                               const gsr_aux_outputs *aux, const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                               const int32_t *median_enc, const float *dL_dmedian, float *screen_grads, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_MEDIAN_H */
