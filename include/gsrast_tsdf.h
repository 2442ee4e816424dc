/* gsrast_tsdf.h — TSDF fusion and mesh extraction in libgsrast.so's C ABI (included by gsrast.h; its conventions hold: device
 * pointers, contiguous fp32, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * Depth maps are fused into a truncated signed distance volume and a triangle mesh is extracted from it: the end
 * of the surface pipeline of 2DGS, Gaussian Opacity Fields, RaDe-GS and PGSR.  The volume is three arrays of nx ny nz voxels, x
 * fastest: tsdf [nz,ny,nx], weight [nz,ny,nx], color [3,nz,ny,nx]; voxel (ix, iy, iz) has its centre at origin + voxel_size (ix, iy,
 * iz); nx ny nz <= 2^31 - 1.  No atomic is used anywhere: the same inputs give the same bits.  Conventions: row-vector matrices
 * (p_view = p V[:3,:3] + V[3,:3]); fx = W / (2 tanfovx), fy = H / (2 tanfovy); pixel (x, y) has its centre at x + 0.5.
 */
#ifndef GSRAST_TSDF_H
#define GSRAST_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Fuses one frame into the volume: one kernel launch, a thread per voxel, no host synchronisation.  depth and alpha are the [H,W] maps
 * of gsr_forward_aux (depth: the unnormalised weighted sum), color is the frame's image [3,H,W], viewmatrix [16] is device memory.
 * Per voxel, in this order:
 *   1. p_view of the voxel's centre; skipped unless z > 0;
 *   2. u = fx x / z + W/2, v = fy y / z + H/2, px = floor(u), py = floor(v); skipped unless the pixel is inside the image;
 *   3. the pixel is valid when alpha >= alpha_min and depth > 0, and then d = depth / alpha; skipped when it is invalid or d > depth_max;
 *   4. s = d - z; skipped unless s > -sdf_trunc;
 *   5. t = min(1, s / sdf_trunc); tsdf = (tsdf w + t) / (w + 1), each colour channel likewise with the pixel's colour, w = w + 1.
 * A skipped voxel's state is neither read nor written.  depth_max may be +infinity.  H = 0 or W = 0: nothing is read. */
int gsr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       float sdf_trunc, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, float depth_max,
                       const float *viewmatrix, const float *depth, const float *alpha, const float *color, float *tsdf,
                       float *weight, float *vol_color, void *stream);

/* Mesh extraction by naive surface nets, in three stages (classify and count per block, scan the block counts, emit).  A voxel is
 * observed when weight >= min_weight and inside when tsdf < 0; a cell (the cube of 8 neighbouring voxels) is active when its 8 voxels
 * are observed and both signs occur.  An active cell owns one vertex: the mean of the crossing points a + (b - a) f_a / (f_a - f_b) of
 * its sign-changing edges (x edges, then y, then z, each by ascending corner index), its colour the mean of the same interpolation of
 * the corners' colours.  A grid edge between two observed voxels of different sign emits one quad over its four adjacent cells'
 * vertices when all four exist and are active, as two triangles split along a fixed diagonal and wound so that (v1 - v0) x (v2 - v0)
 * points from the inside voxel to the outside one.  Vertices come in ascending cell index, faces in ascending (voxel index, axis).
 *
 * gsr_tsdf_mesh_count runs the first two stages and reads the two totals back (the one host synchronisation); gsr_tsdf_mesh_emit,
 * with the same volume, min_weight and workspace, writes vertices [V,3], faces [F,3] (int32) and colors [V,3].  A volume thinner than
 * 2 voxels along an axis has no cell: both totals are 0 and nothing is read.  `workspace`: gsr_tsdf_mesh_workspace_size bytes,
 * 256-byte aligned; it needs no initialisation. */
int gsr_tsdf_mesh_workspace_size(int32_t nx, int32_t ny, int32_t nz, size_t *bytes);
int gsr_tsdf_mesh_count(int32_t nx, int32_t ny, int32_t nz, float min_weight, const float *tsdf, const float *weight, void *workspace,
                        size_t workspace_bytes, int64_t *num_vertices, int64_t *num_faces, void *stream);
int gsr_tsdf_mesh_emit(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                       float min_weight, const float *tsdf, const float *weight, const float *vol_color, void *workspace,
                       size_t workspace_bytes, int64_t num_vertices, int64_t num_faces, float *vertices, int32_t *faces, float *colors,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_TSDF_H */
