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
#include "../../include/gsrast_tsdf.h"

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
