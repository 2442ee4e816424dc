/* gsrast_extra.h — a second colour triple inside the colour frame (included by gsrast.h; its conventions hold: device pointers,
 * contiguous fp32, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * An "extra" frame is an aux frame (gsr_forward_aux: colour, radii, depth, alpha - all bit for bit those of the aux call) whose blend
 * also renders three more linear channels with the colour's own weights.  For one pixel, over the splats the
 * colour composites, w_i = alpha_i T_i:
 *     extra_map[k] = sum_i w_i extra[i][k]      k = 0, 1, 2; no background term; bit for bit the colour of the same frame rendered
 *                                               with colors_precomp = extra over a zero background
 * extra:     [P] rows of FOUR floats (e0, e1, e2, unused), 16-byte aligned: any three per-Gaussian values - view-space normals, a
 *            feature triple, (z^2, ., .) for a distortion term.
 * extra_map: [3,H,W], written by the forward, read by the backward.
 * aux:       as for gsr_forward_aux, except that aux->ckpt_ws holds gsr_extra_workspace_size bytes (four checkpoint planes - the
 *            depth's and the three extra channels' - where the aux frame has one: 4 KB per 128 instances plus
 *            4 (GSR_MAX_CHUNKS - 1) KB per 16x16 tile).  Required (an extra frame is an aux frame).
 * Whole images only (tile_row_begin = tile_row_end = 0).  No floating-point atomic is used: the same frame gives the same bits.
 */
#ifndef GSRAST_EXTRA_H
#define GSRAST_EXTRA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int gsr_extra_workspace_size(const gsr_frame_desc *desc, int64_t binning_capacity, size_t *bytes);
/* bytes of the backward's second row plane: one float4 per instance of gsr_backward_rows_size's bound */
int gsr_extra_rows_size(const gsr_frame_desc *desc, const gsr_frame_plan *plan_host, size_t *bytes);

/* gsr_forward_render_aux / gsr_forward_aux that also write extra_map. */
int gsr_forward_render_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                             void *binning_ws, void *image_ws, gsr_frame_plan *plan_host, float *out_color,
                             const gsr_aux_outputs *aux, const float *extra, float *extra_map, void *stream);
int gsr_forward_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                      int32_t *radii, gsr_frame_plan *plan_host, void *binning_ws, int64_t binning_capacity, float *out_color,
                      gsr_grads *early_fill, const gsr_aux_outputs *aux, const float *extra, float *extra_map, void *stream);

/* gsr_backward_render_aux of an extra frame.  aux, extra, extra_map: what its forward was given.  dL_dcolor [3,H,W], dL_ddepth [H,W],
 * dL_dalpha [H,W], dL_dextra_map [3,H,W]: any may be NULL (zero).  screen_grads as gsr_backward_render_aux leaves it (slot 9 = dL/dz):
 * the extra channels' share of the geometry's gradient is in it, and gsr_backward_geom_aux follows as for an aux frame.
 * extra_rows_ws: gsr_extra_rows_size bytes of scratch.  dL_dextra [P,3] receives sum w dL_dextra_map per Gaussian, the rows added in
 * the fixed order of the other slots; a Gaussian without a row gets exactly 0. */
int gsr_backward_render_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                              const void *image_ws, void *rows_ws, const gsr_frame_plan *plan_host, const float *out_color,
                              const gsr_aux_outputs *aux, const float *extra, const float *extra_map, const float *dL_dcolor,
                              const float *dL_ddepth, const float *dL_dalpha, const float *dL_dextra_map, float *screen_grads,
                              void *extra_rows_ws, float *dL_dextra, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_EXTRA_H */
