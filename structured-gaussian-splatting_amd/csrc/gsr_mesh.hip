// gsr_mesh.hip — mesh cleaning: connected components of a triangle mesh by a lock-free union-find, then an ordered compaction of the
// kept faces and of the vertices they name (include/gsrast_mesh.h).  The rule, the union-find's invariant and why
// its loops end are stated once, in gsr_mesh_math.h; the kernels here load, call, store and count.  Integers only.
//
// Components (gsr_mesh_components: three launches whatever the mesh, no readback):
//   k_mesh_init            a thread per vertex: parent[v] = v, sizes[v] = 0; the give-up word is cleared.
//   k_mesh_link            a thread per face: link (i0, i1) and (i0, i2) (gsr_mesh_math.h mesh_link: one 32-bit atomicCAS per try).
//   k_mesh_label           a thread per face: labels[f] = the root above i0, counted into sizes with an integer atomicAdd per distinct
//                          label of a wave (integer adds commute: the sums do not depend on the order or on the grouping).
// Cleaning (gsr_mesh_clean_count: four launches and the one readback; gsr_mesh_clean_emit: two launches).  No atomic: every output
// position comes from an ordered count.
//   k_mesh_clear_used      the vertices' used flags, a byte each, cleared 16 bytes a thread.
//   k_mesh_classify        a thread per face, 256 faces per block: the keep flag (the threshold is a device word), a wave's flags as
//                          one ballot word, the block's count; a kept face marks its three vertices used - plain stores of the same 1.
//   k_mesh_count_vertices  a thread per vertex, 256 per block: the block's count of used vertices.
//   k_mesh_scan            one block of 1024 threads walks the blocks' counts of kept faces, then those of used vertices, eight per
//                          thread and round: exclusive prefixes per block, the two totals into the control block.
//   k_mesh_emit_vertices   a used vertex's rank = block prefix + the block-wide scan of the flags: vertex_src[rank] = v, remap[v] = rank.
//   k_mesh_emit_faces      a kept face's rank = block prefix + the set bits below it: face_src[rank] = f, faces_out[rank] = remap[faces[f]].
#include "gsr_internal.h"
#include "gsr_mesh_math.h"
#include "../../include/gsrast_mesh.h"

namespace gsr {

constexpr int kMeshBlock = 256, kMeshWaves = kMeshBlock / kWave;
constexpr int kMeshScanBlock = 1024, kMeshScanItems = 8;      // the scan's one block takes 8192 block counts a round

struct MeshCtrl { uint32_t give_up, num_vertices, num_faces, pad; };      // what gsr_mesh_clean_count reads back (totals < 2^31)

struct MeshWS {                                       // the workspace, carved (nbv, nbf = blocks of 256 vertices, faces)
    int32_t *parent;                                  // [V] the union-find
    int32_t *remap;                                   // [V] old vertex index -> new (written for used vertices only)
    uint8_t *used;                                    // [V, padded to 256] 1 = a kept face names the vertex
    unsigned long long *keep_bits;                    // [4 nbf] bit l of word w: face 64 w + l is kept
    uint32_t *face_counts, *face_prefix;              // [nbf] kept faces of the block, of all blocks in front of it
    uint32_t *vertex_counts, *vertex_prefix;          // [nbv] the same of used vertices
    MeshCtrl *ctrl;
    size_t total;
};

static size_t mesh_blocks(int32_t n) { return ((size_t)n + kMeshBlock - 1) / kMeshBlock; }

static MeshWS mesh_carve(void *base, int32_t V, int32_t F)
{
    MeshWS w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    const auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += align_up(bytes); return q; };
    const size_t nbv = mesh_blocks(V), nbf = mesh_blocks(F);
    w.parent = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.remap = reinterpret_cast<int32_t *>(take((size_t)V * 4));
    w.used = reinterpret_cast<uint8_t *>(take((size_t)V));
    w.keep_bits = reinterpret_cast<unsigned long long *>(take(nbf * kMeshWaves * 8));
    w.face_counts = reinterpret_cast<uint32_t *>(take(nbf * 4));
    w.face_prefix = reinterpret_cast<uint32_t *>(take(nbf * 4));
    w.vertex_counts = reinterpret_cast<uint32_t *>(take(nbv * 4));
    w.vertex_prefix = reinterpret_cast<uint32_t *>(take(nbv * 4));
    w.ctrl = reinterpret_cast<MeshCtrl *>(take(sizeof(MeshCtrl)));
    w.total = off;
    return w;
}

// ---- components -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshBlock) void k_mesh_init(int32_t V, int32_t *__restrict__ parent, int32_t *__restrict__ sizes,
                                                          MeshCtrl *__restrict__ ctrl)
{
    const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (v == 0) ctrl->give_up = 0u;
    if (v >= (size_t)V) return;
    parent[v] = (int32_t)v;
    sizes[v] = 0;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_link(int32_t V, int32_t F, const int32_t *__restrict__ faces, int32_t *parent,
                                                          MeshCtrl *ctrl)
{
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (f >= (size_t)F) return;
    mesh_link_face(parent, faces + 3 * f, V, mesh_caps(V), &ctrl->give_up);
}

// sizes[label] += 1 for every lane of the wave that holds a label (>= 0), one atomicAdd per distinct label of the wave: neighbouring
// faces mostly share a component, and 64 single adds to one word would queue up behind each other.  At most 64 rounds (every round
// retires its leader); every lane of the wave is here.
__device__ __forceinline__ void mesh_count_wave(int32_t label, int32_t *sizes)
{
    const int lane = threadIdx.x & (kWave - 1);
    unsigned long long todo = __ballot(label >= 0);
    while (todo) {                                                  // (uniform: todo is the same in every lane)
        const int leader = __ffsll(todo) - 1;
        const int32_t l = __shfl(label, leader);
        const unsigned long long same = __ballot(label == l) & todo;
        if (lane == leader) atomicAdd(sizes + l, (int32_t)__popcll(same));
        todo &= ~same;
    }
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_label(int32_t V, int32_t F, const int32_t *__restrict__ faces, int32_t *parent,
                                                           int32_t *__restrict__ labels, int32_t *sizes, MeshCtrl *ctrl)
{
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    int32_t label = -1;
    if (f < (size_t)F) labels[f] = label = mesh_face_root(parent, faces + 3 * f, V, mesh_caps(V).find_steps, &ctrl->give_up);
    mesh_count_wave(label, sizes);
}

// ---- cleaning ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMeshBlock) void k_mesh_clear_used(size_t words16, uint4 *__restrict__ used16)
{
    const size_t i = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (i < words16) used16[i] = make_uint4(0u, 0u, 0u, 0u);
}

// the block's sum of one count per wave (lane 0 of every wave holds its wave's), into out[blockIdx.x]
__device__ __forceinline__ void mesh_block_count(uint32_t wave_count, uint32_t *sh_wave, uint32_t *__restrict__ out)
{
    if ((threadIdx.x & (kWave - 1)) == 0) sh_wave[threadIdx.x >> 6] = wave_count;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < kMeshWaves; ++w) s += sh_wave[w];
        out[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_classify(int32_t V, int32_t F, const int32_t *__restrict__ faces,
                                                              const int32_t *__restrict__ labels, const int32_t *__restrict__ sizes,
                                                              const int32_t *__restrict__ threshold_dev,
                                                              unsigned long long *__restrict__ keep_bits, uint32_t *__restrict__ face_counts,
                                                              uint8_t *used)
{
    __shared__ uint32_t sh_wave[kMeshWaves];
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    bool keep = false;
    int32_t a = 0, b = 0, c = 0;
    if (f < (size_t)F) {
        a = faces[3 * f]; b = faces[3 * f + 1]; c = faces[3 * f + 2];
        const bool valid = mesh_face_valid(a, b, c, V);
        keep = mesh_face_kept(valid, valid ? labels[f] : -1, V, sizes, *threshold_dev);
    }
    const unsigned long long bits = __ballot(keep);                  // (every thread of the block is here)
    if ((threadIdx.x & (kWave - 1)) == 0) keep_bits[(size_t)blockIdx.x * kMeshWaves + (threadIdx.x >> 6)] = bits;
    mesh_block_count((uint32_t)__popcll(bits), sh_wave, face_counts);
    if (keep) { used[a] = 1; used[b] = 1; used[c] = 1; }             // a kept face is valid: 0 <= a, b, c < V
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_count_vertices(int32_t V, const uint8_t *__restrict__ used,
                                                                    uint32_t *__restrict__ vertex_counts)
{
    __shared__ uint32_t sh_wave[kMeshWaves];
    const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const unsigned long long bits = __ballot(v < (size_t)V && used[v] != 0);
    mesh_block_count((uint32_t)__popcll(bits), sh_wave, vertex_counts);
}

// exclusive prefixes of counts[0 .. nb) by the one block -> their sum
__device__ __forceinline__ uint32_t mesh_scan_counts(size_t nb, const uint32_t *__restrict__ counts, uint32_t *__restrict__ prefix,
                                                     uint32_t *sh_wave)
{
    uint32_t carry = 0;
    for (size_t b0 = 0; b0 < nb; b0 += (size_t)kMeshScanBlock * kMeshScanItems) {
        const size_t first = b0 + (size_t)threadIdx.x * kMeshScanItems;
        uint32_t v[kMeshScanItems], sum = 0;
#pragma unroll
        for (int k = 0; k < kMeshScanItems; ++k) v[k] = first + k < nb ? counts[first + k] : 0u;      // (independent loads: all in flight)
#pragma unroll
        for (int k = 0; k < kMeshScanItems; ++k) sum += v[k];
        uint32_t total;
        __syncthreads();                                            // (uniform) the previous scan's reads of sh_wave are done
        uint32_t run = carry + block_incl_scan<kMeshScanBlock / kWave>(sum, sh_wave, total) - sum;
#pragma unroll
        for (int k = 0; k < kMeshScanItems; ++k) {
            if (first + k < nb) prefix[first + k] = run;
            run += v[k];
        }
        carry += total;
    }
    return carry;
}

__global__ __launch_bounds__(kMeshScanBlock) void k_mesh_scan(size_t nbf, const uint32_t *__restrict__ face_counts,
                                                              uint32_t *__restrict__ face_prefix, size_t nbv,
                                                              const uint32_t *__restrict__ vertex_counts,
                                                              uint32_t *__restrict__ vertex_prefix, MeshCtrl *__restrict__ ctrl)
{
    __shared__ uint32_t sh_wave[kMeshScanBlock / kWave];
    const uint32_t nf = mesh_scan_counts(nbf, face_counts, face_prefix, sh_wave);
    const uint32_t nv = mesh_scan_counts(nbv, vertex_counts, vertex_prefix, sh_wave);
    if (threadIdx.x == 0) { ctrl->num_faces = nf; ctrl->num_vertices = nv; }
}

// nv, nf: what the outputs were sized for (the totals of the count stage); nothing is written past them
__global__ __launch_bounds__(kMeshBlock) void k_mesh_emit_vertices(int32_t V, const uint8_t *__restrict__ used,
                                                                   const uint32_t *__restrict__ vertex_prefix, size_t nv,
                                                                   int32_t *__restrict__ vertex_src, int32_t *__restrict__ remap)
{
    __shared__ uint32_t sh_wave[kMeshWaves];
    const size_t v = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    const uint32_t flag = v < (size_t)V && used[v] != 0 ? 1u : 0u;
    uint32_t total;
    const uint32_t rank = block_incl_scan<kMeshWaves>(flag, sh_wave, total) - flag;      // (every thread of the block is here)
    if (!flag) return;
    const size_t r = (size_t)vertex_prefix[blockIdx.x] + rank;
    remap[v] = (int32_t)r;
    if (r < nv) vertex_src[r] = (int32_t)v;
}

__global__ __launch_bounds__(kMeshBlock) void k_mesh_emit_faces(int32_t V, int32_t F, const int32_t *__restrict__ faces,
                                                                const unsigned long long *__restrict__ keep_bits,
                                                                const uint32_t *__restrict__ face_prefix, const int32_t *__restrict__ remap,
                                                                size_t nf, int32_t *__restrict__ face_src, int32_t *__restrict__ faces_out)
{
    const size_t f = (size_t)blockIdx.x * kMeshBlock + threadIdx.x;
    if (f >= (size_t)F) return;
    const size_t word = f >> 6;
    const unsigned long long bits = keep_bits[word];
    if (!((bits >> (f & 63)) & 1ull)) return;
    size_t r = face_prefix[blockIdx.x];
    for (size_t w = (size_t)blockIdx.x * kMeshWaves; w < word; ++w) r += (size_t)__popcll(keep_bits[w]);
    r += (size_t)__popcll(bits & ((1ull << (f & 63)) - 1ull));
    const int32_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (r >= nf || !mesh_face_valid(a, b, c, V)) return;            // (a kept face is valid: the test guards remap against another mesh)
    face_src[r] = (int32_t)f;
    faces_out[3 * r] = remap[a]; faces_out[3 * r + 1] = remap[b]; faces_out[3 * r + 2] = remap[c];
}

}  // namespace gsr

using namespace gsr;

static int mesh_check_ptr(const char *who, const char *name, const void *p, uintptr_t align)
{
    if (!p) { set_error("%s: %s is NULL", who, name); return GSR_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<uintptr_t>(p) & (align - 1)) { set_error("%s: %s must be %d-byte aligned", who, name, (int)align); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int mesh_check_dims(const char *who, int32_t V, int32_t F)
{
    if (V < 0 || F < 0) { set_error("%s: V = %d, F = %d (0 .. 2^31 - 1 each)", who, V, F); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int mesh_check_workspace(const char *who, int32_t V, int32_t F, const void *workspace, size_t workspace_bytes)
{
    if (int rc = mesh_check_ptr(who, "workspace", workspace, 256)) return rc;
    const size_t need = mesh_carve(nullptr, V, F).total;
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    return GSR_OK;
}

extern "C" int gsr_mesh_clean_workspace_size(int32_t V, int32_t F, size_t *bytes)
{
    const char *who = "gsr_mesh_clean_workspace_size";
    if (int rc = mesh_check_dims(who, V, F)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = V > 0 ? mesh_carve(nullptr, V, F).total : 0;
    return GSR_OK;
}

extern "C" int gsr_mesh_components(int32_t V, int32_t F, const int32_t *faces, int32_t *labels, int32_t *sizes, void *workspace,
                                   size_t workspace_bytes, void *stream)
{
    const char *who = "gsr_mesh_components";
    if (int rc = mesh_check_dims(who, V, F)) return rc;
    if (V == 0) {                                                   // no vertex: every face is invalid, and nothing is read
        if (F > 0) {
            if (int rc = mesh_check_ptr(who, "labels", labels, 4)) return rc;
            GSR_HIP_CHECK(hipMemsetAsync(labels, 0xff, (size_t)F * 4, (hipStream_t)stream));
        }
        return GSR_OK;
    }
    if (int rc = mesh_check_ptr(who, "sizes", sizes, 4)) return rc;
    if (F > 0) {
        if (int rc = mesh_check_ptr(who, "faces", faces, 4)) return rc;
        if (int rc = mesh_check_ptr(who, "labels", labels, 4)) return rc;
    }
    if (int rc = mesh_check_workspace(who, V, F, workspace, workspace_bytes)) return rc;
    const MeshWS ws = mesh_carve(workspace, V, F);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("mesh_init", s);
        hipLaunchKernelGGL(k_mesh_init, dim3((unsigned)mesh_blocks(V)), dim3(kMeshBlock), 0, s, V, ws.parent, sizes, ws.ctrl);
        GSR_LAUNCH_CHECK("mesh_init", false, s);
    }
    if (F == 0) return GSR_OK;
    {
        ProfileScope prof("mesh_link", s);
        hipLaunchKernelGGL(k_mesh_link, dim3((unsigned)mesh_blocks(F)), dim3(kMeshBlock), 0, s, V, F, faces, ws.parent, ws.ctrl);
        GSR_LAUNCH_CHECK("mesh_link", false, s);
    }
    {
        ProfileScope prof("mesh_label", s);
        hipLaunchKernelGGL(k_mesh_label, dim3((unsigned)mesh_blocks(F)), dim3(kMeshBlock), 0, s, V, F, faces, ws.parent, labels, sizes, ws.ctrl);
        GSR_LAUNCH_CHECK("mesh_label", false, s);
    }
    return GSR_OK;
}

extern "C" int gsr_mesh_clean_count(int32_t V, int32_t F, const int32_t *faces, const int32_t *labels, const int32_t *sizes,
                                    const int32_t *threshold_dev, void *workspace, size_t workspace_bytes, int64_t *num_vertices,
                                    int64_t *num_faces, void *stream)
{
    const char *who = "gsr_mesh_clean_count";
    if (int rc = mesh_check_dims(who, V, F)) return rc;
    if (!num_vertices || !num_faces) { set_error("%s: num_vertices or num_faces is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *num_vertices = *num_faces = 0;
    if (V == 0 || F == 0) return GSR_OK;
    if (int rc = mesh_check_ptr(who, "faces", faces, 4)) return rc;
    if (int rc = mesh_check_ptr(who, "labels", labels, 4)) return rc;
    if (int rc = mesh_check_ptr(who, "sizes", sizes, 4)) return rc;
    if (int rc = mesh_check_ptr(who, "threshold_dev", threshold_dev, 4)) return rc;
    if (int rc = mesh_check_workspace(who, V, F, workspace, workspace_bytes)) return rc;
    const MeshWS ws = mesh_carve(workspace, V, F);
    const size_t nbv = mesh_blocks(V), nbf = mesh_blocks(F);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("mesh_clear_used", s);
        const size_t words16 = align_up((size_t)V) / 16;            // (the carved array is padded to 256 bytes)
        hipLaunchKernelGGL(k_mesh_clear_used, dim3((unsigned)((words16 + kMeshBlock - 1) / kMeshBlock)), dim3(kMeshBlock), 0, s, words16,
                           reinterpret_cast<uint4 *>(ws.used));
        GSR_LAUNCH_CHECK("mesh_clear_used", false, s);
    }
    {
        ProfileScope prof("mesh_classify", s);
        hipLaunchKernelGGL(k_mesh_classify, dim3((unsigned)nbf), dim3(kMeshBlock), 0, s, V, F, faces, labels, sizes, threshold_dev, ws.keep_bits,
                           ws.face_counts, ws.used);
        GSR_LAUNCH_CHECK("mesh_classify", false, s);
    }
    {
        ProfileScope prof("mesh_count_vertices", s);
        hipLaunchKernelGGL(k_mesh_count_vertices, dim3((unsigned)nbv), dim3(kMeshBlock), 0, s, V, ws.used, ws.vertex_counts);
        GSR_LAUNCH_CHECK("mesh_count_vertices", false, s);
    }
    {
        ProfileScope prof("mesh_scan", s);
        hipLaunchKernelGGL(k_mesh_scan, dim3(1), dim3(kMeshScanBlock), 0, s, nbf, ws.face_counts, ws.face_prefix, nbv, ws.vertex_counts,
                           ws.vertex_prefix, ws.ctrl);
        GSR_LAUNCH_CHECK("mesh_scan", false, s);
    }
    MeshCtrl ctrl{};
    GSR_HIP_CHECK(hipMemcpyAsync(&ctrl, ws.ctrl, sizeof ctrl, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    if (ctrl.give_up) {
        set_error("%s: the union-find of gsr_mesh_components gave up at a loop bound (V = %d, F = %d): labels and sizes are unspecified", who, V, F);
        return GSR_ERR_HIP;
    }
    *num_vertices = (int64_t)ctrl.num_vertices;
    *num_faces = (int64_t)ctrl.num_faces;
    return GSR_OK;
}

extern "C" int gsr_mesh_clean_emit(int32_t V, int32_t F, const int32_t *faces, void *workspace, size_t workspace_bytes, int64_t num_vertices,
                                   int64_t num_faces, int32_t *vertex_src, int32_t *face_src, int32_t *faces_out, void *stream)
{
    const char *who = "gsr_mesh_clean_emit";
    if (int rc = mesh_check_dims(who, V, F)) return rc;
    if (num_vertices < 0 || num_faces < 0 || num_vertices > V || num_faces > F) {
        set_error("%s: num_vertices = %lld, num_faces = %lld (gsr_mesh_clean_count's: at most V = %d, F = %d)", who, (long long)num_vertices,
                  (long long)num_faces, V, F);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (V == 0 || F == 0 || num_faces == 0) return GSR_OK;
    if (int rc = mesh_check_ptr(who, "faces", faces, 4)) return rc;
    if (int rc = mesh_check_workspace(who, V, F, workspace, workspace_bytes)) return rc;
    if (int rc = mesh_check_ptr(who, "vertex_src", vertex_src, 4)) return rc;
    if (int rc = mesh_check_ptr(who, "face_src", face_src, 4)) return rc;
    if (int rc = mesh_check_ptr(who, "faces_out", faces_out, 4)) return rc;
    const MeshWS ws = mesh_carve(workspace, V, F);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("mesh_emit_vertices", s);
        hipLaunchKernelGGL(k_mesh_emit_vertices, dim3((unsigned)mesh_blocks(V)), dim3(kMeshBlock), 0, s, V, ws.used, ws.vertex_prefix,
                           (size_t)num_vertices, vertex_src, ws.remap);
        GSR_LAUNCH_CHECK("mesh_emit_vertices", false, s);
    }
    {
        ProfileScope prof("mesh_emit_faces", s);
        hipLaunchKernelGGL(k_mesh_emit_faces, dim3((unsigned)mesh_blocks(F)), dim3(kMeshBlock), 0, s, V, F, faces, ws.keep_bits, ws.face_prefix,
                           ws.remap, (size_t)num_faces, face_src, faces_out);
        GSR_LAUNCH_CHECK("mesh_emit_faces", false, s);
    }
    return GSR_OK;
}
