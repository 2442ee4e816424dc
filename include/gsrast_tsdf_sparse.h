/* gsrast_tsdf_sparse.h — the sparse (brick-allocated) TSDF volume in libgsrast.so's C ABI (included by gsrast.h; its conventions and
 * those of gsrast_tsdf.h hold: device pointers, contiguous fp32 / int32, `stream` a hipStream_t as void *, 0 = ok, negative =
 * gsr_status, message via gsr_last_error()).
 *
 * The volume keeps gsrast_tsdf.h's virtual grid (origin, voxel_size, nx ny nz, sdf_trunc), cut into bricks of 8 x 8 x 8 voxels: brick
 * (bx, by, bz) holds the voxels 8 bx .. 8 bx + 7 along x and likewise along y and z; nx, ny, nz <= 32768 each and need not be
 * multiples of 8.  With nbx = ceil(nx / 8) and so on, its state is
 *   brick_table  [nbz,nby,nbx] int32   the slot of an allocated brick, -1 elsewhere; at most 2^31 - 1 entries
 *   marks        [nbz,nby,nbx] int32   non-zero: the brick was marked since the last commit
 *   brick_coords [B,3] int32           (bx, by, bz) of every slot
 *   brick_order  [B] int32             the slots in ascending brick linear index ((bz nby + by) nbx + bx)
 *   brick_rank   [B] int32             its inverse: brick_order[brick_rank[slot]] == slot
 *   tsdf, weight [B,8,8,8], color [B,3,8,8,8]      a brick's voxels [z,y,x]; B 512 <= 2^31 - 1
 * A voxel of an unallocated brick is unobserved (weight 0); a voxel of an allocated brick that lies beyond nx, ny, nz is never written.
 * No atomic is used anywhere: marks are plain stores of one value, every slot and every output position comes from an ordered count.
 * The same frames give the same bits, and - apart from the slots themselves - so does any order of allocation.
 */
#ifndef GSRAST_TSDF_SPARSE_H
#define GSRAST_TSDF_SPARSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Marks the bricks a frame's depth map can reach: one launch, a thread per pixel, no host synchronisation.  A pixel is valid when
 * alpha >= alpha_min and depth > 0 and d = depth / alpha <= depth_max (gsr_tsdf_integrate's steps 3).  Its frustum piece - the
 * footprint [px, px + 1] x [py, py + 1] between the view depths max(d - sdf_trunc, 0) and d + sdf_trunc - goes to world space by its
 * eight corners through viewmatrix_inverse [16] (device memory: the inverse of the view matrix's affine part, p_world = p_view
 * M[:3,:3] + M[3,:3]); the axis-aligned box of the corners in voxel-index coordinates is grown by `pad` voxels (>= 1.25) on every side,
 * and every brick that holds an integer voxel coordinate of the grid inside the box is marked.  H = 0 or W = 0: nothing is read. */
int gsr_tsdf_sparse_allocate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                             float sdf_trunc, float pad, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min,
                             float depth_max, const float *viewmatrix_inverse, const float *depth, const float *alpha, int32_t *marks,
                             void *stream);

/* Committing the marks, in two calls around the one host readback.  gsr_tsdf_sparse_commit_count counts the marked bricks that have
 * no slot yet (a count per 256 table entries, then the scan of gsr_tsdf_mesh_count) and reads the total back.  The caller makes room
 * for num_bricks + num_new slots (capacity: what the per-slot arrays hold), and gsr_tsdf_sparse_commit_assign, with the same
 * workspace, gives the new bricks the slots num_bricks, num_bricks + 1, ... in ascending brick linear index, writes their
 * brick_coords, rewrites brick_order and brick_rank for all num_bricks + num_new slots and clears every mark.  Allocated bricks keep
 * their slots.  `workspace`: gsr_tsdf_sparse_commit_workspace_size bytes, 256-byte aligned; it needs no initialisation. */
int gsr_tsdf_sparse_commit_workspace_size(int32_t nx, int32_t ny, int32_t nz, size_t *bytes);
int gsr_tsdf_sparse_commit_count(int32_t nx, int32_t ny, int32_t nz, const int32_t *marks, const int32_t *brick_table, void *workspace,
                                 size_t workspace_bytes, int64_t *num_new, void *stream);
int gsr_tsdf_sparse_commit_assign(int32_t nx, int32_t ny, int32_t nz, int64_t num_bricks, int64_t capacity, int32_t *marks,
                                  int32_t *brick_table, void *workspace, size_t workspace_bytes, int32_t *brick_coords,
                                  int32_t *brick_order, int32_t *brick_rank, void *stream);

/* gsr_tsdf_integrate's rule (the same per-voxel functions, free-space carving included) on every voxel of every allocated brick: one
 * launch, a block per brick, no host synchronisation.  A skipped voxel is neither read nor written.  A brick whose bounding sphere
 * lies wholly behind the camera or wholly outside one side of the frustum, with a margin for the rounding of both tests, returns
 * as a whole: every voxel it holds would have been skipped. */
int gsr_tsdf_sparse_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                              float sdf_trunc, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, float depth_max,
                              int64_t num_bricks, const float *viewmatrix, const float *depth, const float *alpha, const float *color,
                              const int32_t *brick_coords, float *tsdf, float *weight, float *vol_color, void *stream);

/* gsrast_tsdf.h's surface nets through the brick table: an unallocated brick, a voxel outside nx ny nz and a voxel with weight <
 * min_weight are unobserved.  Vertices come in ascending (brick linear index, local voxel index) of their cell's lowest corner, faces
 * in ascending (that order, axis): the mesh does not depend on the slots.  `cells` may be NULL; otherwise [V,3] int32 receives the
 * lowest-corner voxel (ix, iy, iz) of every vertex's cell.  Count and emit as gsr_tsdf_mesh_count and gsr_tsdf_mesh_emit. */
int gsr_tsdf_sparse_mesh_workspace_size(int64_t num_bricks, size_t *bytes);
int gsr_tsdf_sparse_mesh_count(int32_t nx, int32_t ny, int32_t nz, int64_t num_bricks, float min_weight, const float *tsdf,
                               const float *weight, const int32_t *brick_table, const int32_t *brick_coords, const int32_t *brick_order,
                               const int32_t *brick_rank, void *workspace, size_t workspace_bytes, int64_t *num_vertices,
                               int64_t *num_faces, void *stream);
int gsr_tsdf_sparse_mesh_emit(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                              int64_t num_bricks, float min_weight, const float *tsdf, const float *weight, const float *vol_color,
                              const int32_t *brick_table, const int32_t *brick_coords, const int32_t *brick_order,
                              const int32_t *brick_rank, void *workspace, size_t workspace_bytes, int64_t num_vertices, int64_t num_faces,
                              float *vertices, int32_t *faces, float *colors, int32_t *cells, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_TSDF_SPARSE_H */
