// gsr_tsdf.hip — TSDF fusion of depth maps and mesh extraction by surface nets (include/gsrast_tsdf.h).  The
// arithmetic of one voxel, one cell and one edge lives in gsr_tsdf_math.h; the kernels here load, call, store and count.  No atomic
// anywhere: one thread owns a voxel, and every output position comes from an ordered count, so the same inputs give the same bits.
//
//   k_tsdf_integrate    one launch per frame, a thread per voxel (x fastest: a wave covers 64 consecutive voxels of a row).  A voxel
//                       that is skipped - behind the camera, outside the image, an invalid pixel, beyond the truncation - returns
//                       before it touches the volume: the frame costs 40 B per updated voxel and the maps once.
//   k_sn_classify       a thread per voxel, 256 voxels per block: what the voxel owns (gsr_tsdf_math.h sn_classify).  A wave's vertex
//                       flags are one ballot word (the cells' vertex indices are recovered from these words: no index per voxel is
//                       stored); the block's counts of vertices and quads go out packed as one 64-bit word.
//   k_sn_scan           one block of 1024 threads walks the blocks' packed counts, eight per thread and round: exclusive prefixes per
//                       block, the totals last.
//   k_sn_emit           the classify pass again, now with positions: a vertex at the cell's rank (block prefix + the set bits below
//                       it), a voxel's quads at the block's prefix + the block-wide scan of the threads' quad counts, axis by axis.
#include "gsr_internal.h"
#include "gsr_tsdf_math.h"
#include "gsr_tsdf_sparse_math.h"
#include "../../include/gsrast_tsdf.h"
#include "../../include/gsrast_tsdf_sparse.h"

namespace gsr {

constexpr int kTsdfBlock = 256;
constexpr int kSnBlock = 256, kSnWaves = kSnBlock / kWave;
constexpr int kSnScanBlock = 1024, kSnScanItems = 8;      // the scan's one block takes 8192 block counts a round
constexpr int kSnQuadBits = 33;                       // packed counts: quads in the low 33 bits (<= 3 (2^31 - 1)), vertices above (< 2^31)
constexpr unsigned long long kSnQuadMask = (1ull << kSnQuadBits) - 1ull;

__global__ __launch_bounds__(kTsdfBlock) void k_tsdf_integrate(TsdfGrid g, TsdfFrame f, const float *__restrict__ V,
                                                               const float *__restrict__ depth, const float *__restrict__ alpha,
                                                               const float *__restrict__ image, float *__restrict__ tsdf,
                                                               float *__restrict__ weight, float *__restrict__ color)
{
    const size_t n = (size_t)g.nx * g.ny * g.nz;
    const size_t i = (size_t)blockIdx.x * kTsdfBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = (uint32_t)i / (uint32_t)g.nx;                                  // (n < 2^31)
    const int ix = (int)((uint32_t)i - row * (uint32_t)g.nx), iy = (int)(row % (uint32_t)g.ny), iz = (int)(row / (uint32_t)g.ny);
    int px, py;
    float z, t;
    if (!tsdf_project(g, f, V, ix, iy, iz, px, py, z)) return;
    const size_t hw = (size_t)f.H * f.W, p = (size_t)py * f.W + px;
    if (!tsdf_sample(f, g.trunc, depth[p], alpha[p], z, t)) return;
    const float w = weight[i];
    tsdf[i] = tsdf_mean(tsdf[i], w, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) color[c * n + i] = tsdf_mean(color[c * n + i], w, image[c * hw + p]);
    weight[i] = w + 1.f;
}

struct SnVolume {                                     // the accessors of gsr_tsdf_math.h over the volume
    const float *tsdf, *weight, *color;
    SnDims d; float min_weight; size_t n;
    __device__ __forceinline__ size_t idx(int x, int y, int z) const { return ((size_t)z * d.ny + y) * d.nx + x; }
    __device__ __forceinline__ bool operator()(int x, int y, int z, float &f) const
    {
        const size_t i = idx(x, y, z);
        f = tsdf[i];
        return weight[i] >= min_weight;
    }
};
struct SnColor {
    SnVolume v;
    __device__ __forceinline__ float operator()(int x, int y, int z, int c) const { return v.color[c * v.n + v.idx(x, y, z)]; }
};

struct SnWS {                                         // the workspace, carved (nb = blocks of 256 voxels)
    unsigned long long *vertex_bits;                  // [4 nb] bit l of word w: voxel 64 w + l owns a vertex
    unsigned long long *block_counts;                 // [nb] vertices << 33 | quads of the block
    unsigned long long *block_prefix;                 // [nb] the same of all blocks in front of it
    unsigned long long *totals;                       // [1]
    size_t total;
};

static SnWS sn_carve(void *base, size_t nb)
{
    SnWS w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    const auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += align_up(bytes); return q; };
    w.vertex_bits = reinterpret_cast<unsigned long long *>(take(nb * kSnWaves * 8));
    w.block_counts = reinterpret_cast<unsigned long long *>(take(nb * 8));
    w.block_prefix = reinterpret_cast<unsigned long long *>(take(nb * 8));
    w.totals = reinterpret_cast<unsigned long long *>(take(8));
    w.total = off;
    return w;
}

// voxel i of the block's thread (i >= n: none) -> what it owns
__device__ __forceinline__ unsigned sn_own(const SnVolume &vol, size_t i, int &ix, int &iy, int &iz)
{
    ix = iy = iz = 0;
    if (i >= vol.n) return 0u;
    const uint32_t row = (uint32_t)i / (uint32_t)vol.d.nx;
    ix = (int)((uint32_t)i - row * (uint32_t)vol.d.nx); iy = (int)(row % (uint32_t)vol.d.ny); iz = (int)(row / (uint32_t)vol.d.ny);
    return sn_classify(vol.d, ix, iy, iz, vol);
}

__global__ __launch_bounds__(kSnBlock) void k_sn_classify(SnVolume vol, unsigned long long *__restrict__ vertex_bits,
                                                          unsigned long long *__restrict__ block_counts)
{
    __shared__ unsigned long long sh_wave[kSnWaves];
    const size_t i = (size_t)blockIdx.x * kSnBlock + threadIdx.x;
    int ix, iy, iz;
    const unsigned own = sn_own(vol, i, ix, iy, iz);
    const unsigned long long bits = __ballot((own & kSnVertex) != 0u);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const unsigned long long quads = wave_sum((unsigned long long)__popc(own & 7u));
    if (lane == 0) {
        vertex_bits[(size_t)blockIdx.x * kSnWaves + wave] = bits;
        sh_wave[wave] = ((unsigned long long)__popcll(bits) << kSnQuadBits) | quads;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kSnWaves; ++w) s += sh_wave[w];
        block_counts[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kSnScanBlock) void k_sn_scan(size_t nb, const unsigned long long *__restrict__ block_counts,
                                                          unsigned long long *__restrict__ block_prefix, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long sh_wave[kSnScanBlock / kWave];
    unsigned long long carry = 0;
    for (size_t b0 = 0; b0 < nb; b0 += (size_t)kSnScanBlock * kSnScanItems) {
        const size_t first = b0 + (size_t)threadIdx.x * kSnScanItems;
        unsigned long long v[kSnScanItems], sum = 0;
#pragma unroll
        for (int k = 0; k < kSnScanItems; ++k) v[k] = first + k < nb ? block_counts[first + k] : 0ull;      // (independent loads: all in flight)
#pragma unroll
        for (int k = 0; k < kSnScanItems; ++k) sum += v[k];
        unsigned long long total;
        if (b0) __syncthreads();                                    // (uniform) the previous round's reads of sh_wave are done
        unsigned long long run = carry + block_incl_scan<kSnScanBlock / kWave>(sum, sh_wave, total) - sum;
#pragma unroll
        for (int k = 0; k < kSnScanItems; ++k) {
            if (first + k < nb) block_prefix[first + k] = run;
            run += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) totals[0] = carry;
}

// the vertex index of the active cell whose lowest corner is voxel i
__device__ __forceinline__ int32_t sn_vertex_index(const SnWS &ws, size_t i)
{
    const size_t blk = i / kSnBlock, word = i >> 6;
    unsigned long long before = ws.block_prefix[blk] >> kSnQuadBits;
    for (size_t w = blk * kSnWaves; w < word; ++w) before += (unsigned long long)__popcll(ws.vertex_bits[w]);
    before += (unsigned long long)__popcll(ws.vertex_bits[word] & ((1ull << (i & 63)) - 1ull));
    return (int32_t)before;
}

// nv, nquads: what the outputs were sized for (the totals of the count stage); nothing is written past them
__global__ __launch_bounds__(kSnBlock) void k_sn_emit(SnVolume vol, TsdfGrid g, SnWS ws, size_t nv, size_t nquads, float *__restrict__ vertices,
                                                      int32_t *__restrict__ faces, float *__restrict__ colors)
{
    __shared__ uint32_t sh_wave[kSnWaves];
    const size_t i = (size_t)blockIdx.x * kSnBlock + threadIdx.x;
    int ix, iy, iz;
    const unsigned own = sn_own(vol, i, ix, iy, iz);
    uint32_t total;
    const uint32_t nq = (uint32_t)__popc(own & 7u);
    const uint32_t rank = block_incl_scan<kSnWaves>(nq, sh_wave, total) - nq;       // (every thread of the block is here)
    if (own & kSnVertex) {
        float pos[3], rgb[3];
        sn_vertex(g, ix, iy, iz, vol, SnColor{vol}, pos, rgb);
        const size_t v = (size_t)sn_vertex_index(ws, i);
        if (v < nv) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { vertices[3 * v + j] = pos[j]; colors[3 * v + j] = rgb[j]; }
        }
    }
    if (!nq) return;
    size_t quad = (size_t)(ws.block_prefix[blockIdx.x] & kSnQuadMask) + rank;
    const bool inside = vol.tsdf[i] < 0.f;
    for (int a = 0; a < 3; ++a) {
        if (!(own & (1u << a)) || quad >= nquads) continue;
        int cells[4][3];
        sn_quad_cells(a, ix, iy, iz, cells);
        int32_t v[4], tri[6];
        for (int k = 0; k < 4; ++k) v[k] = sn_vertex_index(ws, vol.idx(cells[k][0], cells[k][1], cells[k][2]));
        sn_quad_faces(v, inside, tri);
        for (int k = 0; k < 6; ++k) faces[6 * quad + k] = tri[k];
        ++quad;
    }
}

}  // namespace gsr

using namespace gsr;

static int tsdf_check_ptr(const char *who, const char *name, const void *p, uintptr_t align)
{
    if (!p) { set_error("%s: %s is NULL", who, name); return GSR_ERR_INVALID_ARGUMENT; }
    if (reinterpret_cast<uintptr_t>(p) & (align - 1)) { set_error("%s: %s must be %d-byte aligned", who, name, (int)align); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int tsdf_check_dims(const char *who, int32_t nx, int32_t ny, int32_t nz, bool empty_ok)
{
    const int32_t lo = empty_ok ? 0 : 1;
    if (nx < lo || ny < lo || nz < lo || (long long)nx * ny > 0x7fffffffLL || (long long)nx * ny * nz > 0x7fffffffLL) {
        set_error("%s: a volume of %d x %d x %d voxels (each dimension >= %d, at most 2^31 - 1 voxels)", who, nx, ny, nz, lo);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int tsdf_check_grid(const char *who, float ox, float oy, float oz, float voxel_size)
{
    if (!isfinite(ox) || !isfinite(oy) || !isfinite(oz) || !(voxel_size > 0.f) || isinf(voxel_size)) {
        set_error("%s: origin = (%g, %g, %g), voxel_size = %g (finite, the size positive)", who, ox, oy, oz, voxel_size);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

extern "C" int gsr_tsdf_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                                  float sdf_trunc, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, float depth_max,
                                  const float *viewmatrix, const float *depth, const float *alpha, const float *color, float *tsdf,
                                  float *weight, float *vol_color, void *stream)
{
    const char *who = "gsr_tsdf_integrate";
    if (int rc = tsdf_check_dims(who, nx, ny, nz, false)) return rc;
    if (int rc = tsdf_check_grid(who, origin_x, origin_y, origin_z, voxel_size)) return rc;
    if (!(sdf_trunc > 0.f) || isinf(sdf_trunc)) { set_error("%s: sdf_trunc = %g (positive and finite)", who, sdf_trunc); return GSR_ERR_INVALID_ARGUMENT; }
    if (H < 0 || W < 0 || H > 32768 || W > 32768) {
        set_error("%s: image height = %d, width = %d (0 .. 32768 each)", who, H, W);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f) || isinf(tanfovx) || isinf(tanfovy)) {
        set_error("%s: tanfovx = %g, tanfovy = %g (positive and finite)", who, tanfovx, tanfovy);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(alpha_min > 0.f) || isinf(alpha_min)) {
        set_error("%s: alpha_min = %g (positive and finite: d = depth / alpha is taken where alpha >= alpha_min)", who, alpha_min);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(depth_max > 0.f)) { set_error("%s: depth_max = %g (positive; +infinity cuts nothing)", who, depth_max); return GSR_ERR_INVALID_ARGUMENT; }
    if (H == 0 || W == 0) return GSR_OK;
    if (int rc = tsdf_check_ptr(who, "viewmatrix", viewmatrix, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "color", color, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "tsdf", tsdf, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "weight", weight, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "vol_color", vol_color, 4)) return rc;
    const TsdfGrid g{nx, ny, nz, origin_x, origin_y, origin_z, voxel_size, sdf_trunc};
    const TsdfFrame f = tsdf_frame(H, W, tanfovx, tanfovy, alpha_min, depth_max);
    const size_t n = (size_t)nx * ny * nz;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_integrate", s);
    hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)((n + kTsdfBlock - 1) / kTsdfBlock)), dim3(kTsdfBlock), 0, s, g, f, viewmatrix, depth, alpha,
                       color, tsdf, weight, vol_color);
    GSR_LAUNCH_CHECK("tsdf_integrate", false, s);
    return GSR_OK;
}

static bool sn_has_cells(int32_t nx, int32_t ny, int32_t nz) { return nx >= 2 && ny >= 2 && nz >= 2; }
static size_t sn_blocks(int32_t nx, int32_t ny, int32_t nz) { return ((size_t)nx * ny * nz + kSnBlock - 1) / kSnBlock; }

extern "C" int gsr_tsdf_mesh_workspace_size(int32_t nx, int32_t ny, int32_t nz, size_t *bytes)
{
    const char *who = "gsr_tsdf_mesh_workspace_size";
    if (int rc = tsdf_check_dims(who, nx, ny, nz, true)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = sn_has_cells(nx, ny, nz) ? sn_carve(nullptr, sn_blocks(nx, ny, nz)).total : 0;
    return GSR_OK;
}

static int sn_check_volume(const char *who, int32_t nx, int32_t ny, int32_t nz, float min_weight, const float *tsdf, const float *weight,
                           const void *workspace, size_t workspace_bytes)
{
    if (isnan(min_weight)) { set_error("%s: min_weight is NaN", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = tsdf_check_ptr(who, "tsdf", tsdf, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "weight", weight, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "workspace", workspace, 256)) return rc;
    const size_t need = sn_carve(nullptr, sn_blocks(nx, ny, nz)).total;
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    return GSR_OK;
}

extern "C" int gsr_tsdf_mesh_count(int32_t nx, int32_t ny, int32_t nz, float min_weight, const float *tsdf, const float *weight, void *workspace,
                                   size_t workspace_bytes, int64_t *num_vertices, int64_t *num_faces, void *stream)
{
    const char *who = "gsr_tsdf_mesh_count";
    if (int rc = tsdf_check_dims(who, nx, ny, nz, true)) return rc;
    if (!num_vertices || !num_faces) { set_error("%s: num_vertices or num_faces is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *num_vertices = *num_faces = 0;
    if (!sn_has_cells(nx, ny, nz)) return GSR_OK;
    if (int rc = sn_check_volume(who, nx, ny, nz, min_weight, tsdf, weight, workspace, workspace_bytes)) return rc;
    const size_t nb = sn_blocks(nx, ny, nz);
    const SnWS ws = sn_carve(workspace, nb);
    const SnVolume vol{tsdf, weight, nullptr, SnDims{nx, ny, nz}, min_weight, (size_t)nx * ny * nz};
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("tsdf_mesh_classify", s);
        hipLaunchKernelGGL(k_sn_classify, dim3((unsigned)nb), dim3(kSnBlock), 0, s, vol, ws.vertex_bits, ws.block_counts);
        GSR_LAUNCH_CHECK("tsdf_mesh_classify", false, s);
    }
    {
        ProfileScope prof("tsdf_mesh_scan", s);
        hipLaunchKernelGGL(k_sn_scan, dim3(1), dim3(kSnScanBlock), 0, s, nb, ws.block_counts, ws.block_prefix, ws.totals);
        GSR_LAUNCH_CHECK("tsdf_mesh_scan", false, s);
    }
    unsigned long long packed = 0;
    GSR_HIP_CHECK(hipMemcpyAsync(&packed, ws.totals, sizeof packed, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *num_vertices = (int64_t)(packed >> kSnQuadBits);
    *num_faces = 2 * (int64_t)(packed & kSnQuadMask);
    return GSR_OK;
}

extern "C" int gsr_tsdf_mesh_emit(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                                  float min_weight, const float *tsdf, const float *weight, const float *vol_color, void *workspace,
                                  size_t workspace_bytes, int64_t num_vertices, int64_t num_faces, float *vertices, int32_t *faces, float *colors,
                                  void *stream)
{
    const char *who = "gsr_tsdf_mesh_emit";
    if (int rc = tsdf_check_dims(who, nx, ny, nz, true)) return rc;
    if (int rc = tsdf_check_grid(who, origin_x, origin_y, origin_z, voxel_size)) return rc;
    if (num_vertices < 0 || num_faces < 0 || (num_faces & 1)) {
        set_error("%s: num_vertices = %lld, num_faces = %lld (gsr_tsdf_mesh_count's)", who, (long long)num_vertices, (long long)num_faces);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!sn_has_cells(nx, ny, nz) || num_vertices == 0) return GSR_OK;
    if (int rc = sn_check_volume(who, nx, ny, nz, min_weight, tsdf, weight, workspace, workspace_bytes)) return rc;
    if (int rc = tsdf_check_ptr(who, "vol_color", vol_color, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "vertices", vertices, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "colors", colors, 4)) return rc;
    if (num_faces) if (int rc = tsdf_check_ptr(who, "faces", faces, 4)) return rc;
    const size_t nb = sn_blocks(nx, ny, nz);
    const SnWS ws = sn_carve(workspace, nb);
    const SnVolume vol{tsdf, weight, vol_color, SnDims{nx, ny, nz}, min_weight, (size_t)nx * ny * nz};
    const TsdfGrid g{nx, ny, nz, origin_x, origin_y, origin_z, voxel_size, 0.f};
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_mesh_emit", s);
    hipLaunchKernelGGL(k_sn_emit, dim3((unsigned)nb), dim3(kSnBlock), 0, s, vol, g, ws, (size_t)num_vertices,
                       (size_t)(num_faces / 2), vertices, faces, colors);
    GSR_LAUNCH_CHECK("tsdf_mesh_emit", false, s);
    return GSR_OK;
}

// ---- the sparse volume (include/gsrast_tsdf_sparse.h) -----------------------------------------------------------
// The same grid cut into bricks of 8 x 8 x 8 voxels behind a dense brick table; the marking rule and the brick arithmetic live in
// gsr_tsdf_sparse_math.h, the per-voxel rules are gsr_tsdf_math.h's, called as the dense kernels call them.  Still no atomic: a mark
// is a plain store of 1, slots and output positions come from ordered counts through k_sn_scan.
//
//   k_brick_mark        a thread per pixel: the bricks of brick_mark_box get marks[e] = 1.
//   k_brick_count       a thread per table entry, 256 per block: the block's bricks that are live after the commit (allocated or
//                       marked) and those that are new (marked, no slot yet), packed as k_sn_classify packs vertices and quads.
//   k_brick_assign      the same pass with positions: a new brick's slot is first_slot + the new ones in front of it, a live brick's
//                       rank the live ones in front of it; marks are cleared.
//   k_tsdfs_integrate   a block per allocated brick, a thread per voxel: a wave covers one z slice of the brick, 64 consecutive
//                       floats of each array.  The brick's cull is computed from blockIdx and the arguments alone: wave-uniform.
//   k_sns_classify, k_sns_emit   k_sn_classify and k_sn_emit over the virtual index 512 rank + local (two blocks per brick), every
//                       voxel read through the brick table.
namespace gsr {

constexpr int kBrickBlock = 256, kBrickWaves = kBrickBlock / kWave;

__global__ __launch_bounds__(kBrickBlock) void k_brick_mark(TsdfGrid g, TsdfFrame f, float pad, const float *__restrict__ Vinv,
                                                            const float *__restrict__ depth, const float *__restrict__ alpha,
                                                            int32_t *__restrict__ marks)
{
    const size_t p = (size_t)blockIdx.x * kBrickBlock + threadIdx.x;
    if (p >= (size_t)f.H * f.W) return;
    const int py = (int)((uint32_t)p / (uint32_t)f.W), px = (int)((uint32_t)p - (uint32_t)py * (uint32_t)f.W);
    BrickBox box;
    if (!brick_mark_box(g, f, Vinv, px, py, depth[p], alpha[p], pad, box)) return;
    const BrickDims bd = brick_dims(g.nx, g.ny, g.nz);                  // (the box is cut to the grid: every brick of it exists)
    for (int bz = box.lo[2]; bz <= box.hi[2]; ++bz)
        for (int by = box.lo[1]; by <= box.hi[1]; ++by)
            for (int bx = box.lo[0]; bx <= box.hi[0]; ++bx) marks[brick_linear(bd, bx, by, bz)] = 1;
}

// entry e of the block's thread (e >= ne: none) -> live << 33 | fresh, each 0 or 1
__device__ __forceinline__ unsigned long long brick_flags(size_t e, size_t ne, const int32_t *marks, const int32_t *table, int32_t &slot, bool &marked)
{
    slot = -1; marked = false;
    if (e >= ne) return 0ull;
    slot = table[e];
    marked = marks[e] != 0;
    const bool fresh = marked && slot < 0;
    return ((unsigned long long)(slot >= 0 || fresh) << kSnQuadBits) | (unsigned long long)fresh;
}

__global__ __launch_bounds__(kBrickBlock) void k_brick_count(size_t ne, const int32_t *__restrict__ marks, const int32_t *__restrict__ table,
                                                             unsigned long long *__restrict__ block_counts)
{
    __shared__ unsigned long long sh_wave[kBrickWaves];
    int32_t slot;
    bool marked;
    const unsigned long long v = brick_flags((size_t)blockIdx.x * kBrickBlock + threadIdx.x, ne, marks, table, slot, marked);
    unsigned long long total;
    block_incl_scan<kBrickWaves>(v, sh_wave, total);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBrickBlock) void k_brick_assign(size_t ne, BrickDims bd, size_t first_slot, size_t capacity,
                                                              const unsigned long long *__restrict__ block_prefix, int32_t *__restrict__ marks,
                                                              int32_t *__restrict__ table, int32_t *__restrict__ coords,
                                                              int32_t *__restrict__ order, int32_t *__restrict__ rank)
{
    __shared__ unsigned long long sh_wave[kBrickWaves];
    const size_t e = (size_t)blockIdx.x * kBrickBlock + threadIdx.x;
    int32_t slot;
    bool marked;
    const unsigned long long v = brick_flags(e, ne, marks, table, slot, marked);
    unsigned long long total;
    const unsigned long long before = block_prefix[blockIdx.x] + block_incl_scan<kBrickWaves>(v, sh_wave, total) - v;
    if (marked) marks[e] = 0;
    if (!v) return;
    if (v & kSnQuadMask) {
        const size_t fresh = first_slot + (size_t)(before & kSnQuadMask);
        if (fresh >= capacity) return;                                  // (the caller made room: never taken)
        slot = (int32_t)fresh;
        table[e] = slot;
        int bx, by, bz;
        brick_of_linear(bd, e, bx, by, bz);
        coords[3 * fresh] = bx; coords[3 * fresh + 1] = by; coords[3 * fresh + 2] = bz;
    }
    const size_t r = (size_t)(before >> kSnQuadBits);
    if (r >= capacity || (size_t)slot >= capacity) return;
    order[r] = slot;
    rank[slot] = (int32_t)r;
}

// Conservative and wave-uniform: true only when every voxel of brick (bx, by, bz) fails tsdf_project's tests.  The brick's voxel
// centres lie within r = 3.5 sqrt(3) voxels of its centre c; a linear form n . p of the world point moves by at most r |n| over
// them, so z <= 0 everywhere when z(c) + r |n_z| <= 0, and u < 0 everywhere in front of the camera when (x + tanfovx z)(c) +
// r |n_x + tanfovx n_z| < 0, and so on for the other three sides.  m pays for the rounding of both evaluations: tsdf_project's x, y, z
// carry a few units of 2^-24 of `mag`, the largest sum of magnitudes that enters them, and m is 1e-4 of it.
__device__ __forceinline__ bool brick_outside(const TsdfGrid &g, const TsdfFrame &f, const float *__restrict__ V, int bx, int by, int bz)
{
    const float c[3] = {fmaf(g.voxel, 8.f * (float)bx + 3.5f, g.ox), fmaf(g.voxel, 8.f * (float)by + 3.5f, g.oy), fmaf(g.voxel, 8.f * (float)bz + 3.5f, g.oz)};
    const float r = 6.0622f * g.voxel * 1.001f;
    const float tx = f.cx / f.fx, ty = f.cy / f.fy;
    float pc[3], nn[3], big = 0.f;
    for (int j = 0; j < 3; ++j) {
        pc[j] = c[0] * V[j] + c[1] * V[4 + j] + c[2] * V[8 + j] + V[12 + j];
        nn[j] = V[j] * V[j] + V[4 + j] * V[4 + j] + V[8 + j] * V[8 + j];
        big = fmaxf(big, fmaxf(fmaxf(fabsf(V[j]), fabsf(V[4 + j])), fmaxf(fabsf(V[8 + j]), fabsf(V[12 + j]))));
    }
    const float mag = (fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]) + 3.f * r + 1.f) * big;
    const float m = 1e-4f * mag * (1.f + fmaxf(tx, ty));
    const float dot_xz = V[0] * V[2] + V[4] * V[6] + V[8] * V[10], dot_yz = V[1] * V[2] + V[5] * V[6] + V[9] * V[10];
    if (pc[2] + r * sqrtf(nn[2]) + m <= 0.f) return true;
    const float nxp = sqrtf(fmaxf(nn[0] + 2.f * tx * dot_xz + tx * tx * nn[2], 0.f)), nxm = sqrtf(fmaxf(nn[0] - 2.f * tx * dot_xz + tx * tx * nn[2], 0.f));
    const float nyp = sqrtf(fmaxf(nn[1] + 2.f * ty * dot_yz + ty * ty * nn[2], 0.f)), nym = sqrtf(fmaxf(nn[1] - 2.f * ty * dot_yz + ty * ty * nn[2], 0.f));
    if (pc[0] + tx * pc[2] + r * nxp + m < 0.f) return true;            // u < 0 for every voxel in front of the camera
    if (pc[0] - tx * pc[2] - r * nxm - m > 0.f) return true;            // u >= W
    if (pc[1] + ty * pc[2] + r * nyp + m < 0.f) return true;            // v < 0
    if (pc[1] - ty * pc[2] - r * nym - m > 0.f) return true;            // v >= H
    return false;
}

__global__ __launch_bounds__(kBrickVoxels) void k_tsdfs_integrate(TsdfGrid g, TsdfFrame f, const float *__restrict__ V,
                                                                   const float *__restrict__ depth, const float *__restrict__ alpha,
                                                                   const float *__restrict__ image, const int32_t *__restrict__ coords,
                                                                   float *__restrict__ tsdf, float *__restrict__ weight, float *__restrict__ color)
{
    const size_t slot = blockIdx.x;
    const int bx = coords[3 * slot], by = coords[3 * slot + 1], bz = coords[3 * slot + 2];
    if (brick_outside(g, f, V, bx, by, bz)) return;
    int ix, iy, iz;
    brick_voxel(bx, by, bz, (int)threadIdx.x, ix, iy, iz);
    if (ix >= g.nx || iy >= g.ny || iz >= g.nz) return;
    int px, py;
    float z, t;
    if (!tsdf_project(g, f, V, ix, iy, iz, px, py, z)) return;
    const size_t hw = (size_t)f.H * f.W, p = (size_t)py * f.W + px;
    if (!tsdf_sample(f, g.trunc, depth[p], alpha[p], z, t)) return;
    const size_t i = slot * kBrickVoxels + threadIdx.x, ci = slot * (3 * kBrickVoxels) + threadIdx.x;
    const float w = weight[i];
    tsdf[i] = tsdf_mean(tsdf[i], w, t);
#pragma unroll
    for (int c = 0; c < 3; ++c) color[ci + c * kBrickVoxels] = tsdf_mean(color[ci + c * kBrickVoxels], w, image[c * hw + p]);
    weight[i] = w + 1.f;
}

struct SnSparse {                                     // the accessors of gsr_tsdf_math.h through the brick table
    const float *tsdf, *weight, *color;
    const int32_t *table, *coords, *order, *rank;
    SnDims d; BrickDims bd; float min_weight; size_t nbricks;
    __device__ __forceinline__ int32_t slot_of(int x, int y, int z) const { return table[brick_linear(bd, x >> kBrickShift, y >> kBrickShift, z >> kBrickShift)]; }
    __device__ __forceinline__ bool operator()(int x, int y, int z, float &f) const
    {
        const int32_t s = slot_of(x, y, z);
        f = 0.f;
        if (s < 0) return false;
        const size_t i = (size_t)s * kBrickVoxels + brick_local(x, y, z);
        f = tsdf[i];
        return weight[i] >= min_weight;
    }
    // 512 rank + local of a voxel of an allocated brick: where the classify pass left its vertex bit
    __device__ __forceinline__ size_t virtual_index(int x, int y, int z) const
    {
        const int32_t s = slot_of(x, y, z);
        return s < 0 ? 0 : (size_t)rank[s] * kBrickVoxels + brick_local(x, y, z);
    }
};
struct SnSparseColor {
    SnSparse v;
    __device__ __forceinline__ float operator()(int x, int y, int z, int c) const
    {
        const int32_t s = v.slot_of(x, y, z);
        return s < 0 ? 0.f : v.color[((size_t)s * 3 + c) * kBrickVoxels + brick_local(x, y, z)];
    }
};

// virtual voxel i of the block's thread (512 rank + local; past the last brick or beyond the grid: none) -> what it owns
__device__ __forceinline__ unsigned sns_own(const SnSparse &vol, size_t i, int &ix, int &iy, int &iz, size_t &pool)
{
    ix = iy = iz = 0; pool = 0;
    const size_t r = i / kBrickVoxels;
    if (r >= vol.nbricks) return 0u;
    const size_t s = (size_t)vol.order[r];
    const int l = (int)(i % kBrickVoxels);
    brick_voxel(vol.coords[3 * s], vol.coords[3 * s + 1], vol.coords[3 * s + 2], l, ix, iy, iz);
    if (ix >= vol.d.nx || iy >= vol.d.ny || iz >= vol.d.nz) return 0u;
    pool = s * kBrickVoxels + l;
    return sn_classify(vol.d, ix, iy, iz, vol);
}

__global__ __launch_bounds__(kSnBlock) void k_sns_classify(SnSparse vol, unsigned long long *__restrict__ vertex_bits,
                                                           unsigned long long *__restrict__ block_counts)
{
    __shared__ unsigned long long sh_wave[kSnWaves];
    const size_t i = (size_t)blockIdx.x * kSnBlock + threadIdx.x;
    int ix, iy, iz;
    size_t pool;
    const unsigned own = sns_own(vol, i, ix, iy, iz, pool);
    const unsigned long long bits = __ballot((own & kSnVertex) != 0u);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const unsigned long long quads = wave_sum((unsigned long long)__popc(own & 7u));
    if (lane == 0) {
        vertex_bits[(size_t)blockIdx.x * kSnWaves + wave] = bits;
        sh_wave[wave] = ((unsigned long long)__popcll(bits) << kSnQuadBits) | quads;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < kSnWaves; ++w) s += sh_wave[w];
        block_counts[blockIdx.x] = s;
    }
}

__global__ __launch_bounds__(kSnBlock) void k_sns_emit(SnSparse vol, TsdfGrid g, SnWS ws, size_t nv, size_t nquads, float *__restrict__ vertices,
                                                       int32_t *__restrict__ faces, float *__restrict__ colors, int32_t *__restrict__ cells_out)
{
    __shared__ uint32_t sh_wave[kSnWaves];
    const size_t i = (size_t)blockIdx.x * kSnBlock + threadIdx.x;
    int ix, iy, iz;
    size_t pool;
    const unsigned own = sns_own(vol, i, ix, iy, iz, pool);
    uint32_t total;
    const uint32_t nq = (uint32_t)__popc(own & 7u);
    const uint32_t rank = block_incl_scan<kSnWaves>(nq, sh_wave, total) - nq;       // (every thread of the block is here)
    if (own & kSnVertex) {
        float pos[3], rgb[3];
        sn_vertex(g, ix, iy, iz, vol, SnSparseColor{vol}, pos, rgb);
        const size_t v = (size_t)sn_vertex_index(ws, i);
        if (v < nv) {
#pragma unroll
            for (int j = 0; j < 3; ++j) { vertices[3 * v + j] = pos[j]; colors[3 * v + j] = rgb[j]; }
            if (cells_out) { cells_out[3 * v] = ix; cells_out[3 * v + 1] = iy; cells_out[3 * v + 2] = iz; }
        }
    }
    if (!nq) return;
    size_t quad = (size_t)(ws.block_prefix[blockIdx.x] & kSnQuadMask) + rank;
    const bool inside = vol.tsdf[pool] < 0.f;
    for (int a = 0; a < 3; ++a) {
        if (!(own & (1u << a)) || quad >= nquads) continue;
        int cells[4][3];
        sn_quad_cells(a, ix, iy, iz, cells);
        int32_t v[4], tri[6];
        for (int k = 0; k < 4; ++k) v[k] = sn_vertex_index(ws, vol.virtual_index(cells[k][0], cells[k][1], cells[k][2]));
        sn_quad_faces(v, inside, tri);
        for (int k = 0; k < 6; ++k) faces[6 * quad + k] = tri[k];
        ++quad;
    }
}

struct BrickWS {                                      // the commit's workspace, carved (nb = blocks of 256 table entries)
    unsigned long long *block_counts, *block_prefix, *totals;
    size_t total;
};

static BrickWS brick_carve(void *base, size_t nb)
{
    BrickWS w;
    char *p = static_cast<char *>(base);
    size_t off = 0;
    const auto take = [&](size_t bytes) { char *q = p ? p + off : nullptr; off += align_up(bytes); return q; };
    w.block_counts = reinterpret_cast<unsigned long long *>(take(nb * 8));
    w.block_prefix = reinterpret_cast<unsigned long long *>(take(nb * 8));
    w.totals = reinterpret_cast<unsigned long long *>(take(8));
    w.total = off;
    return w;
}

}  // namespace gsr

constexpr int64_t kSparseMaxBricks = 0x7fffffffLL / kBrickVoxels;       // the pool's limit: 512 B <= 2^31 - 1

static int tsdfs_check_dims(const char *who, int32_t nx, int32_t ny, int32_t nz)
{
    const BrickDims bd = brick_dims(nx > 0 ? nx : 1, ny > 0 ? ny : 1, nz > 0 ? nz : 1);
    if (nx < 1 || ny < 1 || nz < 1 || nx > 32768 || ny > 32768 || nz > 32768 || (long long)bd.nbx * bd.nby * bd.nbz > 0x7fffffffLL) {
        set_error("%s: a sparse volume of %d x %d x %d voxels (each dimension 1 .. 32768, a brick table of at most 2^31 - 1 entries)", who, nx, ny, nz);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int tsdfs_check_bricks(const char *who, int64_t num_bricks, int64_t limit)
{
    if (num_bricks < 0 || num_bricks > limit) {
        set_error("%s: num_bricks = %lld (0 .. %lld)", who, (long long)num_bricks, (long long)limit);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static size_t tsdfs_entries(int32_t nx, int32_t ny, int32_t nz)
{
    const BrickDims bd = brick_dims(nx, ny, nz);
    return (size_t)bd.nbx * bd.nby * bd.nbz;
}

static int tsdfs_check_frame(const char *who, float sdf_trunc, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, float depth_max)
{
    if (!(sdf_trunc > 0.f) || isinf(sdf_trunc)) { set_error("%s: sdf_trunc = %g (positive and finite)", who, sdf_trunc); return GSR_ERR_INVALID_ARGUMENT; }
    if (H < 0 || W < 0 || H > 32768 || W > 32768) {
        set_error("%s: image height = %d, width = %d (0 .. 32768 each)", who, H, W);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f) || isinf(tanfovx) || isinf(tanfovy)) {
        set_error("%s: tanfovx = %g, tanfovy = %g (positive and finite)", who, tanfovx, tanfovy);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(alpha_min > 0.f) || isinf(alpha_min)) { set_error("%s: alpha_min = %g (positive and finite)", who, alpha_min); return GSR_ERR_INVALID_ARGUMENT; }
    if (!(depth_max > 0.f)) { set_error("%s: depth_max = %g (positive; +infinity cuts nothing)", who, depth_max); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_allocate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                                        float sdf_trunc, float pad, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min,
                                        float depth_max, const float *viewmatrix_inverse, const float *depth, const float *alpha,
                                        int32_t *marks, void *stream)
{
    const char *who = "gsr_tsdf_sparse_allocate";
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (int rc = tsdf_check_grid(who, origin_x, origin_y, origin_z, voxel_size)) return rc;
    if (int rc = tsdfs_check_frame(who, sdf_trunc, H, W, tanfovx, tanfovy, alpha_min, depth_max)) return rc;
    if (!(pad >= 1.25f) || isinf(pad)) { set_error("%s: pad = %g voxels (at least 1.25 and finite: 1 for the stencils, 0.25 for the rounding)", who, pad); return GSR_ERR_INVALID_ARGUMENT; }
    if (H == 0 || W == 0) return GSR_OK;
    if (int rc = tsdf_check_ptr(who, "viewmatrix_inverse", viewmatrix_inverse, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "marks", marks, 4)) return rc;
    const TsdfGrid g{nx, ny, nz, origin_x, origin_y, origin_z, voxel_size, sdf_trunc};
    const TsdfFrame f = tsdf_frame(H, W, tanfovx, tanfovy, alpha_min, depth_max);
    const size_t n = (size_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_sparse_allocate", s);
    hipLaunchKernelGGL(k_brick_mark, dim3((unsigned)((n + kBrickBlock - 1) / kBrickBlock)), dim3(kBrickBlock), 0, s, g, f, pad, viewmatrix_inverse,
                       depth, alpha, marks);
    GSR_LAUNCH_CHECK("tsdf_sparse_allocate", false, s);
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_commit_workspace_size(int32_t nx, int32_t ny, int32_t nz, size_t *bytes)
{
    const char *who = "gsr_tsdf_sparse_commit_workspace_size";
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = brick_carve(nullptr, (tsdfs_entries(nx, ny, nz) + kBrickBlock - 1) / kBrickBlock).total;
    return GSR_OK;
}

static int tsdfs_check_commit(const char *who, int32_t nx, int32_t ny, int32_t nz, const int32_t *marks, const int32_t *table, const void *workspace,
                              size_t workspace_bytes, size_t &nb)
{
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (int rc = tsdf_check_ptr(who, "marks", marks, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_table", table, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "workspace", workspace, 256)) return rc;
    nb = (tsdfs_entries(nx, ny, nz) + kBrickBlock - 1) / kBrickBlock;
    const size_t need = brick_carve(nullptr, nb).total;
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_commit_count(int32_t nx, int32_t ny, int32_t nz, const int32_t *marks, const int32_t *brick_table, void *workspace,
                                            size_t workspace_bytes, int64_t *num_new, void *stream)
{
    const char *who = "gsr_tsdf_sparse_commit_count";
    if (!num_new) { set_error("%s: num_new is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *num_new = 0;
    size_t nb;
    if (int rc = tsdfs_check_commit(who, nx, ny, nz, marks, brick_table, workspace, workspace_bytes, nb)) return rc;
    const BrickWS ws = brick_carve(workspace, nb);
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("tsdf_sparse_commit_count", s);
        hipLaunchKernelGGL(k_brick_count, dim3((unsigned)nb), dim3(kBrickBlock), 0, s, tsdfs_entries(nx, ny, nz), marks, brick_table, ws.block_counts);
        GSR_LAUNCH_CHECK("tsdf_sparse_commit_count", false, s);
    }
    {
        ProfileScope prof("tsdf_sparse_commit_scan", s);
        hipLaunchKernelGGL(k_sn_scan, dim3(1), dim3(kSnScanBlock), 0, s, nb, ws.block_counts, ws.block_prefix, ws.totals);
        GSR_LAUNCH_CHECK("tsdf_sparse_commit_scan", false, s);
    }
    unsigned long long packed = 0;
    GSR_HIP_CHECK(hipMemcpyAsync(&packed, ws.totals, sizeof packed, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *num_new = (int64_t)(packed & kSnQuadMask);
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_commit_assign(int32_t nx, int32_t ny, int32_t nz, int64_t num_bricks, int64_t capacity, int32_t *marks,
                                             int32_t *brick_table, void *workspace, size_t workspace_bytes, int32_t *brick_coords,
                                             int32_t *brick_order, int32_t *brick_rank, void *stream)
{
    const char *who = "gsr_tsdf_sparse_commit_assign";
    size_t nb;
    if (int rc = tsdfs_check_commit(who, nx, ny, nz, marks, brick_table, workspace, workspace_bytes, nb)) return rc;
    if (int rc = tsdfs_check_bricks(who, capacity, kSparseMaxBricks)) return rc;
    if (int rc = tsdfs_check_bricks(who, num_bricks, capacity)) return rc;
    if (capacity) {
        if (int rc = tsdf_check_ptr(who, "brick_coords", brick_coords, 4)) return rc;
        if (int rc = tsdf_check_ptr(who, "brick_order", brick_order, 4)) return rc;
        if (int rc = tsdf_check_ptr(who, "brick_rank", brick_rank, 4)) return rc;
    }
    const BrickWS ws = brick_carve(workspace, nb);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_sparse_commit_assign", s);
    hipLaunchKernelGGL(k_brick_assign, dim3((unsigned)nb), dim3(kBrickBlock), 0, s, tsdfs_entries(nx, ny, nz), brick_dims(nx, ny, nz), (size_t)num_bricks,
                       (size_t)capacity, ws.block_prefix, marks, brick_table, brick_coords, brick_order, brick_rank);
    GSR_LAUNCH_CHECK("tsdf_sparse_commit_assign", false, s);
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_integrate(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                                         float sdf_trunc, int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, float depth_max,
                                         int64_t num_bricks, const float *viewmatrix, const float *depth, const float *alpha, const float *color,
                                         const int32_t *brick_coords, float *tsdf, float *weight, float *vol_color, void *stream)
{
    const char *who = "gsr_tsdf_sparse_integrate";
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (int rc = tsdf_check_grid(who, origin_x, origin_y, origin_z, voxel_size)) return rc;
    if (int rc = tsdfs_check_frame(who, sdf_trunc, H, W, tanfovx, tanfovy, alpha_min, depth_max)) return rc;
    if (int rc = tsdfs_check_bricks(who, num_bricks, kSparseMaxBricks)) return rc;
    if (H == 0 || W == 0 || num_bricks == 0) return GSR_OK;
    if (int rc = tsdf_check_ptr(who, "viewmatrix", viewmatrix, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "color", color, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_coords", brick_coords, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "tsdf", tsdf, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "weight", weight, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "vol_color", vol_color, 4)) return rc;
    const TsdfGrid g{nx, ny, nz, origin_x, origin_y, origin_z, voxel_size, sdf_trunc};
    const TsdfFrame f = tsdf_frame(H, W, tanfovx, tanfovy, alpha_min, depth_max);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_sparse_integrate", s);
    hipLaunchKernelGGL(k_tsdfs_integrate, dim3((unsigned)num_bricks), dim3(kBrickVoxels), 0, s, g, f, viewmatrix, depth, alpha, color, brick_coords,
                       tsdf, weight, vol_color);
    GSR_LAUNCH_CHECK("tsdf_sparse_integrate", false, s);
    return GSR_OK;
}

static size_t sns_blocks(int64_t num_bricks) { return (size_t)num_bricks * (kBrickVoxels / kSnBlock); }

extern "C" int gsr_tsdf_sparse_mesh_workspace_size(int64_t num_bricks, size_t *bytes)
{
    const char *who = "gsr_tsdf_sparse_mesh_workspace_size";
    if (int rc = tsdfs_check_bricks(who, num_bricks, kSparseMaxBricks)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = num_bricks ? sn_carve(nullptr, sns_blocks(num_bricks)).total : 0;
    return GSR_OK;
}

static int sns_check_volume(const char *who, int64_t num_bricks, float min_weight, const float *tsdf, const float *weight, const int32_t *table,
                            const int32_t *coords, const int32_t *order, const int32_t *rank, const void *workspace, size_t workspace_bytes)
{
    if (isnan(min_weight)) { set_error("%s: min_weight is NaN", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = tsdf_check_ptr(who, "tsdf", tsdf, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "weight", weight, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_table", table, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_coords", coords, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_order", order, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "brick_rank", rank, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "workspace", workspace, 256)) return rc;
    const size_t need = sn_carve(nullptr, sns_blocks(num_bricks)).total;
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_mesh_count(int32_t nx, int32_t ny, int32_t nz, int64_t num_bricks, float min_weight, const float *tsdf,
                                          const float *weight, const int32_t *brick_table, const int32_t *brick_coords, const int32_t *brick_order,
                                          const int32_t *brick_rank, void *workspace, size_t workspace_bytes, int64_t *num_vertices,
                                          int64_t *num_faces, void *stream)
{
    const char *who = "gsr_tsdf_sparse_mesh_count";
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (int rc = tsdfs_check_bricks(who, num_bricks, kSparseMaxBricks)) return rc;
    if (!num_vertices || !num_faces) { set_error("%s: num_vertices or num_faces is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *num_vertices = *num_faces = 0;
    if (!sn_has_cells(nx, ny, nz) || num_bricks == 0) return GSR_OK;
    if (int rc = sns_check_volume(who, num_bricks, min_weight, tsdf, weight, brick_table, brick_coords, brick_order, brick_rank, workspace, workspace_bytes)) return rc;
    const size_t nb = sns_blocks(num_bricks);
    const SnWS ws = sn_carve(workspace, nb);
    const SnSparse vol{tsdf, weight, nullptr, brick_table, brick_coords, brick_order, brick_rank, SnDims{nx, ny, nz}, brick_dims(nx, ny, nz), min_weight, (size_t)num_bricks};
    hipStream_t s = (hipStream_t)stream;
    {
        ProfileScope prof("tsdf_sparse_mesh_classify", s);
        hipLaunchKernelGGL(k_sns_classify, dim3((unsigned)nb), dim3(kSnBlock), 0, s, vol, ws.vertex_bits, ws.block_counts);
        GSR_LAUNCH_CHECK("tsdf_sparse_mesh_classify", false, s);
    }
    {
        ProfileScope prof("tsdf_sparse_mesh_scan", s);
        hipLaunchKernelGGL(k_sn_scan, dim3(1), dim3(kSnScanBlock), 0, s, nb, ws.block_counts, ws.block_prefix, ws.totals);
        GSR_LAUNCH_CHECK("tsdf_sparse_mesh_scan", false, s);
    }
    unsigned long long packed = 0;
    GSR_HIP_CHECK(hipMemcpyAsync(&packed, ws.totals, sizeof packed, hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    *num_vertices = (int64_t)(packed >> kSnQuadBits);
    *num_faces = 2 * (int64_t)(packed & kSnQuadMask);
    return GSR_OK;
}

extern "C" int gsr_tsdf_sparse_mesh_emit(int32_t nx, int32_t ny, int32_t nz, float origin_x, float origin_y, float origin_z, float voxel_size,
                                         int64_t num_bricks, float min_weight, const float *tsdf, const float *weight, const float *vol_color,
                                         const int32_t *brick_table, const int32_t *brick_coords, const int32_t *brick_order,
                                         const int32_t *brick_rank, void *workspace, size_t workspace_bytes, int64_t num_vertices, int64_t num_faces,
                                         float *vertices, int32_t *faces, float *colors, int32_t *cells, void *stream)
{
    const char *who = "gsr_tsdf_sparse_mesh_emit";
    if (int rc = tsdfs_check_dims(who, nx, ny, nz)) return rc;
    if (int rc = tsdf_check_grid(who, origin_x, origin_y, origin_z, voxel_size)) return rc;
    if (int rc = tsdfs_check_bricks(who, num_bricks, kSparseMaxBricks)) return rc;
    if (num_vertices < 0 || num_faces < 0 || (num_faces & 1)) {
        set_error("%s: num_vertices = %lld, num_faces = %lld (gsr_tsdf_sparse_mesh_count's)", who, (long long)num_vertices, (long long)num_faces);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!sn_has_cells(nx, ny, nz) || num_bricks == 0 || num_vertices == 0) return GSR_OK;
    if (int rc = sns_check_volume(who, num_bricks, min_weight, tsdf, weight, brick_table, brick_coords, brick_order, brick_rank, workspace, workspace_bytes)) return rc;
    if (int rc = tsdf_check_ptr(who, "vol_color", vol_color, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "vertices", vertices, 4)) return rc;
    if (int rc = tsdf_check_ptr(who, "colors", colors, 4)) return rc;
    if (num_faces) if (int rc = tsdf_check_ptr(who, "faces", faces, 4)) return rc;
    if (cells && (reinterpret_cast<uintptr_t>(cells) & 3)) { set_error("%s: cells must be 4-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    const size_t nb = sns_blocks(num_bricks);
    const SnWS ws = sn_carve(workspace, nb);
    const SnSparse vol{tsdf, weight, vol_color, brick_table, brick_coords, brick_order, brick_rank, SnDims{nx, ny, nz}, brick_dims(nx, ny, nz), min_weight, (size_t)num_bricks};
    const TsdfGrid g{nx, ny, nz, origin_x, origin_y, origin_z, voxel_size, 0.f};
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("tsdf_sparse_mesh_emit", s);
    hipLaunchKernelGGL(k_sns_emit, dim3((unsigned)nb), dim3(kSnBlock), 0, s, vol, g, ws, (size_t)num_vertices, (size_t)(num_faces / 2), vertices,
                       faces, colors, cells);
    GSR_LAUNCH_CHECK("tsdf_sparse_mesh_emit", false, s);
    return GSR_OK;
}
