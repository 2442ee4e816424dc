/* gsrast_mesh.h — mesh cleaning in libgsrast.so's C ABI (included by gsrast.h; its conventions hold: device pointers, contiguous
 * arrays, `stream` a hipStream_t as void *, 0 = ok, negative = gsr_status, message via gsr_last_error()).
 *
 * The connected pieces of a triangle mesh are labelled, the small ones dropped, then the vertices nobody uses: the
 * last step of the surface pipeline of 2DGS, Gaussian Opacity Fields, RaDe-GS and PGSR, after gsrast_tsdf.h's extraction.  The rule:
 * a mesh is faces [F,3] int32 over V vertices, V and F <= 2^31 - 1.
 *   - A face is valid when its three indices lie in [0, V) and are pairwise different.  Any other face is invalid: it joins nothing,
 *     belongs to no component and is always dropped.
 *   - Two valid faces are connected when they share a vertex (not an edge: sheets that touch in one point are one component).
 *   - A component's label is the smallest vertex index it contains.  labels [F] int32 holds it per face, -1 for an invalid face.
 *   - sizes [V] int32 holds at index `label` the number of faces of that component, and 0 elsewhere.
 *   - A face is kept when it is valid and sizes[label] >= threshold; a vertex is kept when a kept face names it.  Kept faces and kept
 *     vertices keep their relative order, and the faces are re-indexed.
 * The kernels move integers only: positions, colours and any other per-vertex attribute are gathered by the caller with vertex_src.
 * No atomic decides an order or a label, so the same mesh gives the same integers.  F = 0 or V = 0: nothing is read, every total is 0.
 *
 * `workspace`: gsr_mesh_clean_workspace_size bytes, 256-byte aligned; one size serves all three calls, and it needs no
 * initialisation.  gsr_mesh_components leaves in it what gsr_mesh_clean_count reports (below), so the calls of one cleaning share it.
 */
#ifndef GSRAST_MESH_H
#define GSRAST_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int gsr_mesh_clean_workspace_size(int32_t V, int32_t F, size_t *bytes);

/* Labels the components: a lock-free union-find over the vertices (the larger root is hung under the smaller with one 32-bit
 * compare-and-swap), then a pass that writes labels [F] and counts sizes [V].  Three kernel launches whatever the mesh, no host loop,
 * no readback, no host synchronisation.  Both of its loops are bounded by what their proof allows (V steps, V tries); a lane that
 * reaches a bound sets a give-up word in the workspace and returns: labels and sizes are then unspecified, and the next
 * gsr_mesh_clean_count on the same workspace fails. */
int gsr_mesh_components(int32_t V, int32_t F, const int32_t *faces, int32_t *labels, int32_t *sizes, void *workspace,
                        size_t workspace_bytes, void *stream);

/* Cleaning in three ordered stages (classify and count per block, scan the block counts, emit).  gsr_mesh_clean_count, behind
 * gsr_mesh_components on the same stream with its labels, sizes and workspace, reads the threshold from the device word
 * *threshold_dev (int32: choosing it costs no synchronisation), marks the kept faces and the vertices they name, counts both and reads
 * the two totals and the give-up word back: the one host synchronisation.  A set give-up word is GSR_ERR_HIP with a message.
 * gsr_mesh_clean_emit, with the same mesh and workspace and the two totals, writes vertex_src [num_vertices] and face_src [num_faces]
 * (int32: the old index of every kept row, ascending) and faces_out [num_faces,3] (int32, indices into the kept vertices); nothing is
 * written past the totals. */
int gsr_mesh_clean_count(int32_t V, int32_t F, const int32_t *faces, const int32_t *labels, const int32_t *sizes,
                         const int32_t *threshold_dev, void *workspace, size_t workspace_bytes, int64_t *num_vertices,
                         int64_t *num_faces, void *stream);
int gsr_mesh_clean_emit(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes, int64_t num_vertices,
                        int64_t num_faces, int32_t *vertex_src, int32_t *face_src, int32_t *faces_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* GSRAST_MESH_H */
