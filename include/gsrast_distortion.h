/* gsrast_distortion.h — the depth-distortion loss in libgsrast.so's C ABI (included by gsrast.h; its conventions hold: device
 * pointers, contiguous fp32, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * Mip-NeRF 360's distortion term in the squared form 2DGS trains with.  Per pixel, over the splats the colour
 * composites, with w_i = alpha_i T_i and a per-splat depth value m_i:
 *     D = sum_{i<j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,    A = sum w_i,  M1 = sum w_i m_i,  M2 = sum w_i m_i^2
 * A is the alpha map of an aux frame; M1 and M2 are two linear channels: render gsr_depth_moments_forward's rows as the extra
 * colours of an extra frame (gsrast_extra.h; its `extra` rows are FOUR floats wide, these are three) and hand the extra map here.
 * No atomic is used: the same inputs give the same bits.  Row-vector matrices (p_view = p V[:3,:3] + V[3,:3]).
 */
#ifndef GSRAST_DISTORTION_H
#define GSRAST_DISTORTION_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSR_DISTORTION_NDC 0       /* m = far (z - near) / ((far - near) z), in [0, 1): 2DGS's choice */
#define GSR_DISTORTION_LINEAR 1    /* m = z: gsplat's */

/* Per-Gaussian depth moments, moments_out [P,3] = (m, m m, +0.0): z = the view depth of means3D [P,3] under viewmatrix [4,4]
 * (z = x V02 + y V12 + z V22 + V32), m by `mapping`; where z <= near_plane (NDC) or z <= 0 (LINEAR), m = +0.0.  0 < near_plane <
 * far_plane, finite, under either mapping.  P = 0: nothing is read.
 * The backward recomputes z and m; grad_means3D [P,3] = (grad_moments[0] + 2 m grad_moments[1]) dm/dz (V02, V12, V22), exactly +0.0
 * where m was set to 0; it is the only gradient (the camera is a constant). */
int gsr_depth_moments_forward(int64_t P, const float *means3D, const float *viewmatrix, int32_t mapping, float near_plane,
                              float far_plane, float *moments_out, void *stream);
int gsr_depth_moments_backward(int64_t P, const float *means3D, const float *viewmatrix, int32_t mapping, float near_plane,
                               float far_plane, const float *grad_moments, float *grad_means3D, void *stream);

/* The distortion map, distortion_out [H,W] = fma(A, M2, -(M1 M1)), not clamped: M1, M2 = planes 0 and 1 of moments_map [3,H,W]
 * (plane 2 is never read), A = alpha [H,W].  H = 0 or W = 0: nothing is read.
 * The backward reads grad_distortion [H,W] = g and writes grad_moments_map [3,H,W] = (-2 g M1, g A, +0.0) and grad_alpha [H,W] =
 * g M2 (either may be NULL: not wanted). */
int gsr_distortion_map_forward(int32_t H, int32_t W, const float *moments_map, const float *alpha, float *distortion_out, void *stream);
int gsr_distortion_map_backward(int32_t H, int32_t W, const float *moments_map, const float *alpha, const float *grad_distortion,
                                float *grad_moments_map, float *grad_alpha, void *stream);

/* The loss, loss_out [1] = mean over the H W pixels of the map above, which is never stored: sums of 1 024 consecutive pixels in
 * binary32 in a fixed order, then those sums in binary64 in a fixed order by a second launch behind the first.
 * `workspace`: gsr_distortion_loss_workspace_size(H, W) bytes, 4-byte aligned, of any content; two calls in flight must not share one.
 * The backward reads grad_loss [1] and is the map's backward with g = grad_loss / (H W) at every pixel. */
int gsr_distortion_loss_workspace_size(int32_t H, int32_t W, size_t *bytes);
int gsr_distortion_loss_forward(int32_t H, int32_t W, const float *moments_map, const float *alpha, void *workspace, size_t workspace_bytes,
                                float *loss_out, void *stream);
int gsr_distortion_loss_backward(int32_t H, int32_t W, const float *moments_map, const float *alpha, const float *grad_loss,
                                 float *grad_moments_map, float *grad_alpha, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_DISTORTION_H */
