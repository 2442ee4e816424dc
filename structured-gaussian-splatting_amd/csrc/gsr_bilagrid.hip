// gsr_bilagrid.hip — the per-image bilateral grid between the rasterizer and the loss (gsplat's lib_bilagrid; include/gsrast.h
// gsr_bilagrid_*).  The arithmetic of one pixel lives in gsr_bilagrid_math.h; the kernels here load, call, store
// and sum.  No floating-point atomic anywhere: every sum has an order the program fixes, so the same inputs give the same bits.
//
//   k_bilagrid_fwd      one launch, a block per tile of 64 x 16 pixels, four pixels per thread: 12 B read, 12 B written per pixel.  The
//                       grid nodes a tile reads (its footprint) are at most 3 x 3 where a grid cell is larger than the tile: they are
//                       staged in LDS, coefficients side by side, and a pixel's 96 coefficients are LDS reads.  Where the footprint
//                       does not fit (more nodes than pixels: up to the whole grid) the pixels read the grid through L1 / L2.
//   k_bilagrid_bwd      one launch, the same tiles.  Phase A, a thread per pixel (four each): dimage from the same staged footprint,
//                       and the pixel's tap and its six values staged in LDS.  Phase B: the footprint's nodes are dealt to the
//                       block's four waves; a wave walks the tile's 1 024 staged pixels, 16 per lane in a fixed order, with the
//                       weight of its node on each (zero for most), the luma levels as the innermost loop, and ends with one wave
//                       sum per (level, coefficient).  The sums go to the block's own slice of the workspace.
//   k_bilagrid_reduce   one launch, a thread per element of the gradient [N, 12, L, Gy, Gx]: image idx adds the partials of the blocks
//                       whose footprint holds the element's node, in block order; every other image is written as zero.
//   k_bilagrid_tv_fwd   one launch: per-thread, per-wave and per-block sums of the squared forward differences (binary32), the
//                       block's three sums to the workspace, a ticket; the wave that draws the last ticket adds the blocks' sums in
//                       block order (binary64) and writes the value.
//   k_bilagrid_tv_bwd   one launch, a thread per element: the 3-axis stencil gathered, nothing scattered.
#include "gsr_internal.h"
#include "gsr_bilagrid_math.h"

namespace gsr {

constexpr int kBgBlock = 256;
constexpr int kBgTileW = 64, kBgTileH = 16, kBgTilePx = kBgTileW * kBgTileH;
constexpr int kBgLev = 8;                 // luma levels a wave accumulates at once (the default L): 96 sums in registers
constexpr int kBgStage = 10;              // staged words per pixel: packed (x0, y0, z0), tx, ty, tz, r, g, b, go[3]
constexpr int kBgStageFloats = 2304;      // LDS floats for a tile's footprint of the grid: 3 x 4 nodes of the default 8 x 12
constexpr int kBgMaxAxis = 1024;          // nodes per axis: 10 bits each in the packed word
constexpr int kTvBlock = 256, kTvMaxBlocks = 512;

struct BgTiles { int nbx, nby, nx_cap, ny_cap; };      // tiles of the image; the most nodes per axis a tile's footprint can hold

__device__ __forceinline__ void tile_footprint(const BilaDims &d, const BgTiles &t, int bx, int by, int &xlo, int &nxb, int &ylo, int &nyb)
{
    int xhi, yhi;
    const int px1 = min(bx * kBgTileW + kBgTileW - 1, d.W - 1), py1 = min(by * kBgTileH + kBgTileH - 1, d.H - 1);
    bila_span(bx * kBgTileW, px1, d.W, d.Gx, xlo, xhi);
    bila_span(by * kBgTileH, py1, d.H, d.Gy, ylo, yhi);
    nxb = min(xhi - xlo + 1, t.nx_cap);      // (the caps hold by construction, see bilagrid_tiles: the min keeps every index inside
    nyb = min(yhi - ylo + 1, t.ny_cap);      // the block's slice whatever the arithmetic does)
}

// The footprint's nodes into LDS, [ny, nx, L, 12] (BilaTileView); the walk follows the grid's own layout, x fastest
__device__ __forceinline__ void stage_footprint(const BilaDims &d, const float *__restrict__ grid, int xlo, int nxb, int ylo, int nyb, float *sg)
{
    const int nodes = nxb * nyb, total = nodes * d.L * 12;
    for (int e = threadIdx.x; e < total; e += kBgBlock) {
        const int nx = e % nxb, ny = e / nxb % nyb, z = e / nodes % d.L, k = e / (nodes * d.L);
        sg[((ny * nxb + nx) * d.L + z) * 12 + k] = grid[(((size_t)k * d.L + z) * d.Gy + ylo + ny) * d.Gx + xlo + nx];
    }
}

// STAGED: the tile's footprint fits kBgStageFloats (the host decides, from the caps): the 96 coefficients of a pixel come from LDS,
// three 16-byte reads per corner, instead of 96 loads that a wave with mixed lumas spreads over eight cache lines each
template <bool STAGED>
__global__ __launch_bounds__(kBgBlock) void k_bilagrid_fwd(BilaDims d, BgTiles tl, const float *__restrict__ grid,
                                                           const float *__restrict__ image, float *__restrict__ out)
{
    __shared__ __align__(16) float sg[STAGED ? kBgStageFloats : 4];
    const int bx = blockIdx.x % tl.nbx, by = blockIdx.x / tl.nbx;
    const size_t n = (size_t)d.H * d.W;
    int xlo = 0, nxb = 0, ylo = 0, nyb = 0;
    if constexpr (STAGED) {
        tile_footprint(d, tl, bx, by, xlo, nxb, ylo, nyb);
        stage_footprint(d, grid, xlo, nxb, ylo, nyb, sg);
        __syncthreads();
    }
    for (int q = threadIdx.x; q < kBgTilePx; q += kBgBlock) {
        const int px = bx * kBgTileW + (q & (kBgTileW - 1)), py = by * kBgTileH + (q / kBgTileW);
        if (px >= d.W || py >= d.H) continue;
        const size_t i = (size_t)py * d.W + px;
        const float in[3] = {image[i], image[n + i], image[2 * n + i]};
        const BilaTap t = bila_tap(d, py, px, in[0], in[1], in[2]);
        float o[3];
        if constexpr (STAGED) bila_forward_one(BilaTileView{sg, d.L, xlo, ylo, nxb}, t, in, o);
        else bila_forward_one(BilaGridView{grid, d.L, d.Gy, d.Gx}, t, in, o);
        out[i] = o[0]; out[n + i] = o[1]; out[2 * n + i] = o[2];
    }
}

template <bool STAGED>
__global__ __launch_bounds__(kBgBlock) void k_bilagrid_bwd(BilaDims d, BgTiles tl, const float *__restrict__ grid,
                                                           const float *__restrict__ image, const float *__restrict__ gout,
                                                           float *__restrict__ dimage, float *__restrict__ partials)
{
    __shared__ float sh[kBgStage][kBgTilePx];
    __shared__ __align__(16) float sg[STAGED ? kBgStageFloats : 4];
    const int bx = blockIdx.x % tl.nbx, by = blockIdx.x / tl.nbx;
    const size_t n = (size_t)d.H * d.W;
    int xlo, nxb, ylo, nyb;
    tile_footprint(d, tl, bx, by, xlo, nxb, ylo, nyb);
    if constexpr (STAGED) {
        if (dimage) {                                        // (uniform over the grid: a kernel argument)
            stage_footprint(d, grid, xlo, nxb, ylo, nyb, sg);
            __syncthreads();
        }
    }
    // ---- phase A: dimage; stage the tile (a pixel outside the image is staged with zero weights and values)
    for (int q = threadIdx.x; q < kBgTilePx; q += kBgBlock) {
        const int px = bx * kBgTileW + (q & (kBgTileW - 1)), py = by * kBgTileH + (q / kBgTileW);
        float in[3] = {0.f, 0.f, 0.f}, go[3] = {0.f, 0.f, 0.f}, tx = 0.f, ty = 0.f, tz = 0.f;
        uint32_t packed = 0;
        if (px < d.W && py < d.H) {
            const size_t i = (size_t)py * d.W + px;
            in[0] = image[i]; in[1] = image[n + i]; in[2] = image[2 * n + i];
            go[0] = gout[i]; go[1] = gout[n + i]; go[2] = gout[2 * n + i];
            const BilaTap t = bila_tap(d, py, px, in[0], in[1], in[2]);
            if (dimage) {
                float di[3];
                if constexpr (STAGED) bila_backward_image_one(d.L, BilaTileView{sg, d.L, xlo, ylo, nxb}, t, in, go, di);
                else bila_backward_image_one(d.L, BilaGridView{grid, d.L, d.Gy, d.Gx}, t, in, go, di);
                dimage[i] = di[0]; dimage[n + i] = di[1]; dimage[2 * n + i] = di[2];
            }
            packed = (uint32_t)t.x.i0 | (uint32_t)t.y.i0 << 10 | (uint32_t)t.z.i0 << 20;
            tx = t.x.t; ty = t.y.t; tz = t.z.t;
        }
        if (partials) {
            sh[0][q] = __uint_as_float(packed); sh[1][q] = tx; sh[2][q] = ty; sh[3][q] = tz;
            sh[4][q] = in[0]; sh[5][q] = in[1]; sh[6][q] = in[2];
            sh[7][q] = go[0]; sh[8][q] = go[1]; sh[9][q] = go[2];
        }
    }
    if (!partials) return;                                   // (uniform over the grid: a kernel argument)
    __syncthreads();
    // ---- phase B: the footprint's nodes, one wave each
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    float *pb = partials + (size_t)blockIdx.x * tl.nx_cap * tl.ny_cap * d.L * 12;
    for (int nl = wave; nl < nxb * nyb; nl += kBgBlock / kWave) {
        const int ny = ylo + nl / nxb, nx = xlo + nl % nxb;
        for (int l0 = 0; l0 < d.L; l0 += kBgLev) {
            float acc[kBgLev][12];
#pragma unroll
            for (int l = 0; l < kBgLev; ++l)
#pragma unroll
                for (int k = 0; k < 12; ++k) acc[l][k] = 0.f;
            for (int q = lane; q < kBgTilePx; q += kWave) {
                const uint32_t packed = __float_as_uint(sh[0][q]);
                BilaAxis ax, ay, az;
                ax.i0 = (int)(packed & 1023u); ax.i1 = min(ax.i0 + 1, d.Gx - 1); ax.t = sh[1][q];
                ay.i0 = (int)(packed >> 10 & 1023u); ay.i1 = min(ay.i0 + 1, d.Gy - 1); ay.t = sh[2][q];
                az.i0 = (int)(packed >> 20 & 1023u); az.i1 = min(az.i0 + 1, d.L - 1); az.t = sh[3][q];
                const float wxy = bila_axis_weight(ax, nx) * bila_axis_weight(ay, ny);
                if (wxy != 0.f) {
                    const float in4[4] = {sh[4][q], sh[5][q], sh[6][q], 1.f};
                    float v[12];
#pragma unroll
                    for (int c = 0; c < 3; ++c)
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[4 * c + j] = sh[7 + c][q] * in4[j];
#pragma unroll
                    for (int l = 0; l < kBgLev; ++l) {
                        const float w = wxy * bila_axis_weight(az, l0 + l);
#pragma unroll
                        for (int k = 0; k < 12; ++k) acc[l][k] += w * v[k];
                    }
                }
            }
            // 96 wave sums; lane e % 64 keeps sum e, so that the slice is written with two coalesced stores
            float mine[(kBgLev * 12 + kWave - 1) / kWave];
#pragma unroll
            for (int r = 0; r < (kBgLev * 12 + kWave - 1) / kWave; ++r) mine[r] = 0.f;
#pragma unroll
            for (int l = 0; l < kBgLev; ++l)
#pragma unroll
                for (int k = 0; k < 12; ++k) {
                    const float s = wave_sum(acc[l][k]);
                    if (lane == ((l * 12 + k) & (kWave - 1))) mine[(l * 12 + k) / kWave] = s;
                }
#pragma unroll
            for (int r = 0; r < (kBgLev * 12 + kWave - 1) / kWave; ++r) {
                const int e = r * kWave + lane;                      // = l * 12 + k of the chunk
                if (e < kBgLev * 12 && l0 + e / 12 < d.L) pb[((size_t)nl * d.L + l0) * 12 + e] = mine[r];
            }
        }
    }
}

__global__ __launch_bounds__(kBgBlock) void k_bilagrid_reduce(BilaDims d, BgTiles tl, int N, int idx, const float *__restrict__ partials,
                                                              float *__restrict__ dgrids)
{
    const int64_t per_image = (int64_t)12 * d.L * d.Gy * d.Gx;
    const int64_t t = (int64_t)blockIdx.x * kBgBlock + threadIdx.x;
    if (t >= per_image * N) return;
    const int img = (int)(t / per_image);
    if (img != idx) { dgrids[t] = 0.f; return; }
    // within the image the thread index walks (node, level, coefficient): a block's slice is read in whole lines
    const int64_t e = t - (int64_t)img * per_image;
    const int k = (int)(e % 12), l = (int)(e / 12 % d.L), node = (int)(e / (12 * (int64_t)d.L));
    const int y = node / d.Gx, x = node % d.Gx;
    // the tiles whose footprint holds the node: a range per axis (footprints move with the tile)
    int bx0 = tl.nbx, bx1 = -1, by0 = tl.nby, by1 = -1, lo, hi;
    for (int bx = 0; bx < tl.nbx; ++bx) {
        bila_span(bx * kBgTileW, min(bx * kBgTileW + kBgTileW - 1, d.W - 1), d.W, d.Gx, lo, hi);
        if (lo <= x && x <= hi) { bx0 = min(bx0, bx); bx1 = bx; }
    }
    for (int by = 0; by < tl.nby; ++by) {
        bila_span(by * kBgTileH, min(by * kBgTileH + kBgTileH - 1, d.H - 1), d.H, d.Gy, lo, hi);
        if (lo <= y && y <= hi) { by0 = min(by0, by); by1 = by; }
    }
    const size_t slice = (size_t)tl.nx_cap * tl.ny_cap * d.L * 12;
    float s = 0.f;
    for (int by = by0; by <= by1; ++by)
        for (int bx = bx0; bx <= bx1; ++bx) {
            int xlo, nxb, ylo, nyb;
            tile_footprint(d, tl, bx, by, xlo, nxb, ylo, nyb);
            const int rx = x - xlo, ry = y - ylo;
            if (rx < 0 || rx >= nxb || ry < 0 || ry >= nyb) continue;
            s += partials[(size_t)(by * tl.nbx + bx) * slice + ((size_t)(ry * nxb + rx) * d.L + l) * 12 + k];
        }
    dgrids[(int64_t)img * per_image + ((int64_t)k * d.L + l) * d.Gy * d.Gx + node] = s;
}

// workspace: sums [kTvMaxBlocks][3] floats, then the ticket word (zero between calls: the last block puts the zero back)
__global__ __launch_bounds__(kTvBlock) void k_bilagrid_tv_fwd(int64_t n, int L, int Gy, int Gx, const float *__restrict__ g, float *sums,
                                                              unsigned int *ticket, double ix, double iy, double iz, float *__restrict__ out)
{
    __shared__ float sh[kTvBlock / kWave][3];
    float sx = 0.f, sy = 0.f, sz = 0.f;
    const int64_t plane = (int64_t)Gy * Gx;
    for (int64_t e = (int64_t)blockIdx.x * kTvBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kTvBlock) {
        const int x = (int)(e % Gx), y = (int)(e / Gx % Gy), z = (int)(e / plane % L);
        const float v = g[e];
        if (x + 1 < Gx) { const float t = g[e + 1] - v; sx += t * t; }
        if (y + 1 < Gy) { const float t = g[e + Gx] - v; sy += t * t; }
        if (z + 1 < L) { const float t = g[e + plane] - v; sz += t * t; }
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    if (lane == 0) { sh[wave][0] = sx; sh[wave][1] = sy; sh[wave][2] = sz; }
    __syncthreads();
    if (wave != 0) return;
    // wave 0: the block's sums in wave order, published; the ticket (release: the sums are visible to whoever reads it; acquire:
    // the last block sees every other block's)
    int last = 0;
    if (lane == 0) {
        float b[3] = {0.f, 0.f, 0.f};
        for (int w = 0; w < kTvBlock / kWave; ++w) { b[0] += sh[w][0]; b[1] += sh[w][1]; b[2] += sh[w][2]; }
        sums[3 * blockIdx.x] = b[0]; sums[3 * blockIdx.x + 1] = b[1]; sums[3 * blockIdx.x + 2] = b[2];
        const unsigned int drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = drawn == gridDim.x - 1;
    }
    if (!__shfl(last, 0)) return;
    double tx = 0.0, ty = 0.0, tz = 0.0;
    for (int b = lane; b < (int)gridDim.x; b += kWave) {
        tx += (double)__hip_atomic_load(&sums[3 * b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ty += (double)__hip_atomic_load(&sums[3 * b + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tz += (double)__hip_atomic_load(&sums[3 * b + 2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    tx = wave_sum(tx); ty = wave_sum(ty); tz = wave_sum(tz);
    if (lane == 0) {
        out[0] = (float)(tx * ix + ty * iy + tz * iz);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kTvBlock) void k_bilagrid_tv_bwd(int64_t n, int L, int Gy, int Gx, const float *__restrict__ g,
                                                              const float *__restrict__ gout, float kx, float ky, float kz,
                                                              float *__restrict__ dg)
{
    const int64_t e = (int64_t)blockIdx.x * kTvBlock + threadIdx.x;
    if (e >= n) return;
    const int x = (int)(e % Gx), y = (int)(e / Gx % Gy), z = (int)(e / ((int64_t)Gy * Gx) % L);
    const float u = gout[0];
    dg[e] = bila_tv_backward_one(g, e, z, y, x, L, Gy, Gx, kx * u, ky * u, kz * u);
}

}  // namespace gsr

using namespace gsr;

// The most nodes a tile's footprint holds on one axis: a tile of T pixels spans (T - 1) (G - 1) / n grid cells, its pixels' lower
// nodes at most floor(span) + 2 values, the upper node of the last one more.
static int axis_cap(int tile, int n, int G)
{
    const long long cap = (long long)(tile - 1) * (G - 1) / n + 3;
    return (int)(cap < G ? cap : G);
}

static BgTiles bilagrid_tiles(const BilaDims &d)
{
    BgTiles t;
    t.nbx = (d.W + kBgTileW - 1) / kBgTileW; t.nby = (d.H + kBgTileH - 1) / kBgTileH;
    t.nx_cap = axis_cap(kBgTileW, d.W, d.Gx); t.ny_cap = axis_cap(kBgTileH, d.H, d.Gy);
    return t;
}

// the footprint of every tile fits the LDS stage
static bool bilagrid_staged(const BilaDims &d, const BgTiles &t) { return (long long)t.nx_cap * t.ny_cap * d.L * 12 <= kBgStageFloats; }

static size_t bilagrid_partial_bytes(const BilaDims &d)
{
    const BgTiles t = bilagrid_tiles(d);
    return align_up((size_t)t.nbx * t.nby * t.nx_cap * t.ny_cap * d.L * 12 * sizeof(float));
}

constexpr size_t kTvWorkspaceBytes = 8192;      // kTvMaxBlocks x 3 floats and the ticket word behind them
static_assert(kTvMaxBlocks * 3 * sizeof(float) + sizeof(unsigned int) <= kTvWorkspaceBytes, "the TV workspace holds the sums and the ticket");

static int validate_grid(const char *who, int N, int L, int Gy, int Gx)
{
    if (N < 1 || L < 1 || Gy < 1 || Gx < 1 || L > kBgMaxAxis || Gy > kBgMaxAxis || Gx > kBgMaxAxis ||
        (long long)N * 12 * L * Gy * Gx > 0x7fffffffLL) {
        set_error("%s: grids [N=%d, 12, L=%d, Gy=%d, Gx=%d]: every size is 1 .. %d and the tensor holds fewer than 2^31 floats", who, N, L, Gy, Gx,
                  kBgMaxAxis);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int validate_image(const char *who, int H, int W)
{
    if (H < 0 || W < 0 || H > 32768 || W > 32768) {
        set_error("%s: image height = %d, width = %d (0 .. 32768 each)", who, H, W);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

extern "C" int gsr_bilagrid_workspace_size(int32_t H, int32_t W, int32_t L, int32_t Gy, int32_t Gx, size_t *backward_bytes, size_t *tv_bytes)
{
    const char *who = "gsr_bilagrid_workspace_size";
    if (int rc = validate_grid(who, 1, L, Gy, Gx)) return rc;
    if (int rc = validate_image(who, H, W)) return rc;
    if (!backward_bytes && !tv_bytes) { set_error("%s: backward_bytes and tv_bytes are both NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    const BilaDims d{L, Gy, Gx, H, W};
    if (backward_bytes) *backward_bytes = (H == 0 || W == 0) ? 0 : bilagrid_partial_bytes(d);
    if (tv_bytes) *tv_bytes = kTvWorkspaceBytes;
    return GSR_OK;
}

extern "C" int gsr_bilagrid_forward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, int32_t H, int32_t W, int32_t idx, const float *grids,
                                    const float *image, float *out, void *stream)
{
    const char *who = "gsr_bilagrid_forward";
    if (int rc = validate_grid(who, N, L, Gy, Gx)) return rc;
    if (int rc = validate_image(who, H, W)) return rc;
    if (idx < 0 || idx >= N) { set_error("%s: idx = %d is outside [0, %d)", who, idx, N); return GSR_ERR_INVALID_ARGUMENT; }
    if (H == 0 || W == 0) return GSR_OK;
    if (!grids || !image || !out) { set_error("%s: NULL pointer (grids, image and out are required)", who); return GSR_ERR_INVALID_ARGUMENT; }
    const BilaDims d{L, Gy, Gx, H, W};
    hipStream_t s = (hipStream_t)stream;
    const BgTiles tl = bilagrid_tiles(d);
    const float *grid = grids + (size_t)idx * 12 * L * Gy * Gx;
    const dim3 blocks((unsigned)(tl.nbx * tl.nby)), threads(kBgBlock);
    ProfileScope prof("bilagrid_fwd", s);
    if (bilagrid_staged(d, tl)) hipLaunchKernelGGL(k_bilagrid_fwd<true>, blocks, threads, 0, s, d, tl, grid, image, out);
    else hipLaunchKernelGGL(k_bilagrid_fwd<false>, blocks, threads, 0, s, d, tl, grid, image, out);
    GSR_LAUNCH_CHECK("bilagrid_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_bilagrid_backward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, int32_t H, int32_t W, int32_t idx, const float *grids,
                                     const float *image, const float *grad_out, float *grad_grids, float *grad_image, void *workspace,
                                     size_t workspace_bytes, void *stream)
{
    const char *who = "gsr_bilagrid_backward";
    if (int rc = validate_grid(who, N, L, Gy, Gx)) return rc;
    if (int rc = validate_image(who, H, W)) return rc;
    if (idx < 0 || idx >= N) { set_error("%s: idx = %d is outside [0, %d)", who, idx, N); return GSR_ERR_INVALID_ARGUMENT; }
    if (H == 0 || W == 0 || (!grad_grids && !grad_image)) return GSR_OK;
    if (!grids || !image || !grad_out) { set_error("%s: NULL pointer (grids, image and grad_out are required)", who); return GSR_ERR_INVALID_ARGUMENT; }
    const BilaDims d{L, Gy, Gx, H, W};
    const BgTiles tl = bilagrid_tiles(d);
    if (grad_grids) {
        if (!workspace) { set_error("%s: grad_grids needs the workspace (gsr_bilagrid_workspace_size)", who); return GSR_ERR_INVALID_ARGUMENT; }
        if (workspace_bytes < bilagrid_partial_bytes(d)) {
            set_error("%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, bilagrid_partial_bytes(d));
            return GSR_ERR_WORKSPACE;
        }
    }
    hipStream_t s = (hipStream_t)stream;
    const float *grid = grids + (size_t)idx * 12 * L * Gy * Gx;
    float *partials = grad_grids ? static_cast<float *>(workspace) : nullptr;
    {
        ProfileScope prof("bilagrid_bwd", s);
        const dim3 blocks((unsigned)(tl.nbx * tl.nby)), threads(kBgBlock);
        if (bilagrid_staged(d, tl)) hipLaunchKernelGGL(k_bilagrid_bwd<true>, blocks, threads, 0, s, d, tl, grid, image, grad_out, grad_image, partials);
        else hipLaunchKernelGGL(k_bilagrid_bwd<false>, blocks, threads, 0, s, d, tl, grid, image, grad_out, grad_image, partials);
        GSR_LAUNCH_CHECK("bilagrid_bwd", false, s);
    }
    if (grad_grids) {
        const long long total = (long long)N * 12 * L * Gy * Gx;
        ProfileScope prof("bilagrid_reduce", s);
        hipLaunchKernelGGL(k_bilagrid_reduce, dim3((unsigned)((total + kBgBlock - 1) / kBgBlock)), dim3(kBgBlock), 0, s, d, tl, N, idx, partials, grad_grids);
        GSR_LAUNCH_CHECK("bilagrid_reduce", false, s);
    }
    return GSR_OK;
}

// 1 / (the number of differences along an axis), 0 for an axis of size 1
static void tv_counts(int N, int L, int Gy, int Gx, double inv[3])
{
    const double all = (double)N * 12;
    inv[0] = Gx > 1 ? 1.0 / (all * L * Gy * (Gx - 1)) : 0.0;
    inv[1] = Gy > 1 ? 1.0 / (all * L * (Gy - 1) * Gx) : 0.0;
    inv[2] = L > 1 ? 1.0 / (all * (L - 1) * Gy * Gx) : 0.0;
}

extern "C" int gsr_bilagrid_tv_forward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, const float *grids, void *workspace, float *out, void *stream)
{
    const char *who = "gsr_bilagrid_tv_forward";
    if (int rc = validate_grid(who, N, L, Gy, Gx)) return rc;
    if (!grids || !workspace || !out) { set_error("%s: NULL pointer (grids, workspace and out are required)", who); return GSR_ERR_INVALID_ARGUMENT; }
    const int64_t n = (int64_t)N * 12 * L * Gy * Gx;
    int64_t nb = (n + 4 * kTvBlock - 1) / (4 * kTvBlock);
    nb = nb < 1 ? 1 : (nb > kTvMaxBlocks ? kTvMaxBlocks : nb);
    double inv[3];
    tv_counts(N, L, Gy, Gx, inv);
    hipStream_t s = (hipStream_t)stream;
    float *sums = static_cast<float *>(workspace);
    ProfileScope prof("bilagrid_tv_fwd", s);
    hipLaunchKernelGGL(k_bilagrid_tv_fwd, dim3((unsigned)nb), dim3(kTvBlock), 0, s, n, L, Gy, Gx, grids, sums,
                       reinterpret_cast<unsigned int *>(sums + 3 * kTvMaxBlocks), inv[0], inv[1], inv[2], out);
    GSR_LAUNCH_CHECK("bilagrid_tv_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_bilagrid_tv_backward(int32_t N, int32_t L, int32_t Gy, int32_t Gx, const float *grids, const float *grad_out, float *grad_grids,
                                        void *stream)
{
    const char *who = "gsr_bilagrid_tv_backward";
    if (int rc = validate_grid(who, N, L, Gy, Gx)) return rc;
    if (!grids || !grad_out || !grad_grids) { set_error("%s: NULL pointer (grids, grad_out and grad_grids are required)", who); return GSR_ERR_INVALID_ARGUMENT; }
    const int64_t n = (int64_t)N * 12 * L * Gy * Gx;
    double inv[3];
    tv_counts(N, L, Gy, Gx, inv);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("bilagrid_tv_bwd", s);
    hipLaunchKernelGGL(k_bilagrid_tv_bwd, dim3((unsigned)((n + kTvBlock - 1) / kTvBlock)), dim3(kTvBlock), 0, s, n, L, Gy, Gx, grids, grad_out,
                       (float)(2.0 * inv[0]), (float)(2.0 * inv[1]), (float)(2.0 * inv[2]), grad_grids);
    GSR_LAUNCH_CHECK("bilagrid_tv_bwd", false, s);
    return GSR_OK;
}
