/* gsrast_normals.h — the normal-map entry points of libgsrast.so's C ABI (included by gsrast.h; its conventions hold: device
 * pointers, contiguous fp32, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * Three ops for the normal-consistency term of 2DGS, Gaussian Opacity Fields, RaDe-GS, PGSR and DN-Splatter.
 * Every one is one kernel launch; no floating-point atomic is used, so the same inputs give the same bits.  Conventions: row-vector
 * matrices (p_view = p V[:3,:3] + V[3,:3]); fx = W / (2 tanfovx), fy = H / (2 tanfovy); pixel (x, y) has its centre at x + 0.5, so
 * px = x + 0.5 - W/2, py = y + 0.5 - H/2; the view space is x right, y down, z forward; quaternions are (w, x, y, z).
 */
#ifndef GSRAST_NORMALS_H
#define GSRAST_NORMALS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-Gaussian normals in the view space, normals_out [P,3]: with k = argmin_j scales[p,j] (ties to the lowest j; scales or
 * log-scales alike), n_w = column k of R(q / |q|) (rotations [P,4], raw or unit), turned to the camera (n_w = -n_w when
 * <n_w, means3D_p - campos> > 0; exactly 0 does not flip), the output is n_w V[:3,:3].  rotations and grad_rotations are read and
 * written as 16-byte rows.  P = 0: nothing is read.
 * The backward recomputes k and the sign from the inputs; grad_rotations [P,4] is the only gradient (k and the sign are piecewise
 * constant; the camera is a constant). */
int gsr_gaussian_normals_forward(int64_t P, const float *scales, const float *rotations, const float *means3D, const float *viewmatrix,
                                 const float *campos, float *normals_out, void *stream);
int gsr_gaussian_normals_backward(int64_t P, const float *scales, const float *rotations, const float *means3D, const float *viewmatrix,
                                  const float *campos, const float *grad_normals, float *grad_rotations, void *stream);

/* The normal map implied by a rendered depth, normal_out [3,H,W].  depth and alpha are the [H,W] maps of gsr_forward_aux (depth: the
 * unnormalised weighted sum).  A pixel is valid when alpha >= alpha_min and depth > 0, and then z = depth / alpha.  The output at
 * (x, y) is non-zero only when 1 <= x <= W-2, 1 <= y <= H-2 and the four axis neighbours are valid (the centre's own validity is
 * not asked); then with Dx = z(x+1,y) - z(x-1,y), Sx = z(x+1,y) + z(x-1,y), Dy and Sy likewise along y,
 *     m = (fx Sy Dx, fy Sx Dy, -(Sx Sy + px Sy Dx + py Sx Dy)),   n = m / |m|
 * (a fronto-parallel surface gives (0, 0, -1)).  Everywhere else the output is +0.0.  H = 0 or W = 0: nothing is read.
 * The backward is a gather: grad_depth / grad_alpha [H,W] (either may be NULL: not wanted) at a valid pixel are the chain through
 * z of what the normals of its four neighbours take from it, added in the order left, right, up, down; +0.0 at any other pixel. */
int gsr_depth_normal_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth, const float *alpha,
                             float *normal_out, void *stream);
int gsr_depth_normal_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth, const float *alpha,
                              const float *grad_normal, float *grad_depth, float *grad_alpha, void *stream);

/* The normal-consistency loss L = (1 / (H W)) sum_p (1 - alpha_p <N_p, n_p>), loss_out [1]: N = normal_map [3,H,W] (the rendered,
 * alpha-weighted normals), n the map of gsr_depth_normal_forward (never stored; a pixel without one adds 1), alpha a constant as a
 * factor and differentiated through z.  Per-block sums in binary32, then the blocks' sums in block order in binary64.
 * `workspace`: gsr_normal_consistency_workspace_size(H, W) bytes, 256-byte aligned, whose first word is zero before the first call
 * and is left zero by every call (one workspace per stream: two calls in flight must not share one).
 * The backward reads grad_loss [1] and writes grad_normal_map [3,H,W] = -grad_loss alpha n / (H W), grad_depth and grad_alpha [H,W]
 * (any may be NULL: not wanted). */
int gsr_normal_consistency_workspace_size(int32_t H, int32_t W, size_t *bytes);
int gsr_normal_consistency_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *normal_map,
                                   const float *depth, const float *alpha, void *workspace, size_t workspace_bytes, float *loss_out,
                                   void *stream);
int gsr_normal_consistency_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *normal_map,
                                    const float *depth, const float *alpha, const float *grad_loss, float *grad_normal_map,
                                    float *grad_depth, float *grad_alpha, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_NORMALS_H */
