// gsr_normals.hip — normal maps for surface regularisation (2DGS's normal-consistency term; include/gsrast_normals.h; DESIGN section
// 23).  The arithmetic of one Gaussian and of one pixel lives in gsr_normals_math.h; the kernels here load, call, store and sum.  No
// floating-point atomic anywhere: every sum has an order the program fixes, so the same inputs give the same bits.
//
//   k_gaussian_normals_fwd / _bwd   one launch each, a thread per Gaussian: 40 B read and 12 B written forward; the backward reads
//                       the same 40 B and dL/dnormal, recomputes the axis and the sign, and writes dL/drotation (16 B).
//   k_depth_normal_fwd<LOSS>        one launch, a block per tile of 64 x 16 pixels, four pixels per thread.  The tile's view depths
//                       z = depth / alpha and a halo of one pixel are staged in LDS (an invalid or outside pixel as a negative
//                       sentinel); every pixel then reads its four neighbours from LDS.  LOSS = false writes n [3,H,W]; LOSS = true
//                       forms 1 - alpha <N, n> instead: at most 1 024 blocks walk the tiles, each sums its terms per thread, wave
//                       and block (binary32), leaves the sum in the workspace and draws a ticket; the block that draws the last adds
//                       the blocks' sums in a fixed order (binary64).
//   k_depth_normal_bwd<LOSS>        one launch, the same tiles, a gather.  Phase 1 stages z and alpha of the tile with a halo of two.
//                       Phase 2, over the tile with a halo of one: the pixel's normal recomputed, its upstream gradient (read, or
//                       under LOSS formed from N and alpha), and what it takes from each of its four neighbours' depths, staged in
//                       LDS; LOSS also writes dL/dN for the tile's own pixels.  Phase 3, per pixel of the tile: the four takes that
//                       name it, added in the order left, right, up, down, and the chain through z = depth / alpha.
#include "gsr_internal.h"
#include "gsr_normals_math.h"
#include "../../include/gsrast_normals.h"

namespace gsr {

constexpr int kNrmBlock = 256;
constexpr int kNrmTileW = 64, kNrmTileH = 16, kNrmTilePx = kNrmTileW * kNrmTileH;
constexpr float kNrmInvalid = -1.f;            // staged z of a pixel that is invalid or outside the image (a valid z is >= 0)
constexpr int kNrmMaxBlocks = 1024;            // blocks of the loss forward: each walks ceil(tiles / 1024) tiles
constexpr size_t kNrmTicketBytes = 256;        // the workspace: the ticket word, then one float per block

struct Row3 { float v[3]; };                     // a [P,3] row: 4-byte aligned, moved as one 12-byte access

__global__ __launch_bounds__(kNrmBlock) void k_gaussian_normals_fwd(int64_t P, const Row3 *__restrict__ scales, const float4 *__restrict__ rot,
                                                                    const Row3 *__restrict__ means, const float *__restrict__ V,
                                                                    const float *__restrict__ cam, Row3 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kNrmBlock + threadIdx.x;
    if (i >= P) return;
    const Row3 s = scales[i], m = means[i];
    const float4 q4 = rot[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    Row3 o;
    nrm_gaussian_forward_one(s.v, q, m.v, V, cam, o.v);
    out[i] = o;
}

__global__ __launch_bounds__(kNrmBlock) void k_gaussian_normals_bwd(int64_t P, const Row3 *__restrict__ scales, const float4 *__restrict__ rot,
                                                                    const Row3 *__restrict__ means, const float *__restrict__ V,
                                                                    const float *__restrict__ cam, const Row3 *__restrict__ gout,
                                                                    float4 *__restrict__ drot)
{
    const int64_t i = (int64_t)blockIdx.x * kNrmBlock + threadIdx.x;
    if (i >= P) return;
    const Row3 s = scales[i], m = means[i], g = gout[i];
    const float4 q4 = rot[i];
    const float q[4] = {q4.x, q4.y, q4.z, q4.w};
    float dq[4];
    nrm_gaussian_backward_one(s.v, q, m.v, V, cam, g.v, dq);
    drot[i] = make_float4(dq[0], dq[1], dq[2], dq[3]);
}

// A tile with a halo of HALO pixels, staged: z (kNrmInvalid where the pixel is invalid or outside) and, where wanted, alpha
template <int HALO>
struct NrmTile {
    static constexpr int SW = kNrmTileW + 2 * HALO, SH = kNrmTileH + 2 * HALO, N = SW * SH;
    int x0, y0;                                   // the image coordinates of the stage's first element
    __device__ __forceinline__ int at(int x, int y) const { return (y - y0) * SW + (x - x0); }
};

template <int HALO, bool WITH_ALPHA>
__device__ __forceinline__ void nrm_stage(const NrmDims &d, const NrmTile<HALO> &t, const float *__restrict__ depth,
                                          const float *__restrict__ alpha, float *sz, float *sa)
{
    for (int e = threadIdx.x; e < NrmTile<HALO>::N; e += kNrmBlock) {
        const int x = t.x0 + e % NrmTile<HALO>::SW, y = t.y0 + e / NrmTile<HALO>::SW;
        float z = kNrmInvalid, a = 0.f;
        if (x >= 0 && x < d.W && y >= 0 && y < d.H) {
            const size_t i = (size_t)y * d.W + x;
            const float dp = depth[i];
            a = alpha[i];
            if (nrm_valid(d, dp, a)) z = dp / a;
        }
        sz[e] = z;
        if (WITH_ALPHA) sa[e] = a;
    }
}

template <int HALO>
struct NrmStagedZ {                               // the accessor of gsr_normals_math.h over a staged tile
    const float *sz; NrmTile<HALO> t;
    __device__ __forceinline__ bool operator()(int x, int y, float &z) const { z = sz[t.at(x, y)]; return z >= 0.f; }
};

// LOSS: at most kNrmMaxBlocks blocks walk the tiles with the grid's stride, so that the last block has few sums to add
template <bool LOSS>
__global__ __launch_bounds__(kNrmBlock) void k_depth_normal_fwd(NrmDims d, int nbx, int ntiles, const float *__restrict__ depth,
                                                                const float *__restrict__ alpha, const float *__restrict__ Nmap, float *__restrict__ out,
                                                                unsigned int *ticket, float *sums, double inv_hw)
{
    __shared__ float sz[NrmTile<1>::N];
    __shared__ float sh_wave[kNrmBlock / kWave];
    __shared__ double sh_total[kNrmBlock / kWave];
    __shared__ int sh_last;
    const size_t n = (size_t)d.H * d.W;
    float acc = 0.f;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int bx = tile % nbx, by = tile / nbx;
        if (tile != (int)blockIdx.x) __syncthreads();              // (uniform) the previous tile's pixels have read the stage
        NrmTile<1> t;
        t.x0 = bx * kNrmTileW - 1; t.y0 = by * kNrmTileH - 1;
        nrm_stage<1, false>(d, t, depth, alpha, sz, nullptr);
        __syncthreads();
        const NrmStagedZ<1> zat{sz, t};
        for (int q = threadIdx.x; q < kNrmTilePx; q += kNrmBlock) {
            const int x = bx * kNrmTileW + (q & (kNrmTileW - 1)), y = by * kNrmTileH + q / kNrmTileW;
            if (x >= d.W || y >= d.H) continue;
            const size_t i = (size_t)y * d.W + x;
            NrmStencil s;
            float nv[3] = {0.f, 0.f, 0.f};
            const bool has = nrm_stencil(d, x, y, zat, s);
            if (has) nrm_normal_one(d, nrm_px(d, x), nrm_py(d, y), s, nv);
            if constexpr (LOSS) {
                float Nv[3] = {0.f, 0.f, 0.f}, a = 0.f;
                if (has) { Nv[0] = Nmap[i]; Nv[1] = Nmap[n + i]; Nv[2] = Nmap[2 * n + i]; a = alpha[i]; }
                acc += nrm_loss_term(has, a, Nv, nv);
            } else {
                out[i] = nv[0]; out[n + i] = nv[1]; out[2 * n + i] = nv[2];
            }
        }
    }
    if constexpr (LOSS) {
        acc = wave_sum(acc);
        const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
        if (lane == 0) sh_wave[wave] = acc;
        __syncthreads();
        // thread 0: the block's sum in wave order, published; the ticket (release: the sum is visible to whoever reads it; acquire:
        // the last block sees every other block's)
        if (threadIdx.x == 0) {
            float b = 0.f;
            for (int w = 0; w < kNrmBlock / kWave; ++w) b += sh_wave[w];
            sums[blockIdx.x] = b;
            const unsigned int drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            sh_last = drawn == gridDim.x - 1;
        }
        __syncthreads();
        if (!sh_last) return;                                       // (uniform over the block)
        // the last block: the blocks' sums in binary64, thread t those of blocks t, t + 256, ...; then lanes, then waves, in order
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        double tot = 0.0;
        for (int b = threadIdx.x; b < (int)gridDim.x; b += kNrmBlock) tot += (double)__hip_atomic_load(&sums[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tot = wave_sum(tot);
        if (lane == 0) sh_total[wave] = tot;
        __syncthreads();
        if (threadIdx.x == 0) {
            double all = 0.0;
            for (int w = 0; w < kNrmBlock / kWave; ++w) all += sh_total[w];
            out[0] = (float)(all * inv_hw);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// gin: dL/dn [3,H,W] (LOSS = false) or the rendered normal map N (LOSS = true, with scale = -dL/dloss / (H W) read from gloss)
template <bool LOSS>
__global__ __launch_bounds__(kNrmBlock) void k_depth_normal_bwd(NrmDims d, int nbx, const float *__restrict__ depth, const float *__restrict__ alpha,
                                                                const float *__restrict__ gin, const float *__restrict__ gloss, float inv_hw,
                                                                float *__restrict__ dN, float *__restrict__ ddepth, float *__restrict__ dalpha)
{
    using Outer = NrmTile<2>;
    using Inner = NrmTile<1>;
    __shared__ float sz[Outer::N], sa[Outer::N];
    __shared__ float take[4][Inner::N];
    const int bx = blockIdx.x % nbx, by = blockIdx.x / nbx;
    Outer to;
    to.x0 = bx * kNrmTileW - 2; to.y0 = by * kNrmTileH - 2;
    Inner ti;
    ti.x0 = bx * kNrmTileW - 1; ti.y0 = by * kNrmTileH - 1;
    nrm_stage<2, true>(d, to, depth, alpha, sz, sa);
    __syncthreads();
    const NrmStagedZ<2> zat{sz, to};
    const size_t n = (size_t)d.H * d.W;
    float scale = 0.f;
    if constexpr (LOSS) scale = -(gloss[0] * inv_hw);
    const bool want_z = ddepth || dalpha;                       // (uniform over the grid: kernel arguments)
    // ---- phase 2: the takes of every pixel of the tile and its halo of one
    for (int e = threadIdx.x; e < Inner::N; e += kNrmBlock) {
        const int x = ti.x0 + e % Inner::SW, y = ti.y0 + e / Inner::SW;
        float gz[4] = {0.f, 0.f, 0.f, 0.f}, nv[3] = {0.f, 0.f, 0.f};
        const bool inside = x >= 0 && x < d.W && y >= 0 && y < d.H;
        NrmStencil s;
        const bool has = inside && nrm_stencil(d, x, y, zat, s);
        float a = 0.f;
        if (has) {
            const size_t i = (size_t)y * d.W + x;
            const float px = nrm_px(d, x), py = nrm_py(d, y);
            const float inv = nrm_normal_one(d, px, py, s, nv);
            float g[3] = {gin[i], gin[n + i], gin[2 * n + i]};
            if constexpr (LOSS) {
                a = sa[to.at(x, y)] * scale;
                g[0] *= a; g[1] *= a; g[2] *= a;
            }
            if (want_z) nrm_normal_backward_one(d, px, py, s, nv, inv, g, gz);
        }
        take[0][e] = gz[0]; take[1][e] = gz[1]; take[2][e] = gz[2]; take[3][e] = gz[3];
        if constexpr (LOSS) {
            const int tx = x - bx * kNrmTileW, ty = y - by * kNrmTileH;
            if (dN && inside && tx >= 0 && tx < kNrmTileW && ty >= 0 && ty < kNrmTileH) {
                const size_t i = (size_t)y * d.W + x;
                dN[i] = has ? a * nv[0] : 0.f; dN[n + i] = has ? a * nv[1] : 0.f; dN[2 * n + i] = has ? a * nv[2] : 0.f;
            }
        }
    }
    if (!want_z) return;
    __syncthreads();
    // ---- phase 3: the gather
    const auto taken = [&](int x, int y, int slot) { return take[slot][ti.at(x, y)]; };
    for (int q = threadIdx.x; q < kNrmTilePx; q += kNrmBlock) {
        const int x = bx * kNrmTileW + (q & (kNrmTileW - 1)), y = by * kNrmTileH + q / kNrmTileW;
        if (x >= d.W || y >= d.H) continue;
        const size_t i = (size_t)y * d.W + x;
        const float z = sz[to.at(x, y)];
        float gd = 0.f, ga = 0.f;
        if (z >= 0.f) nrm_chain(nrm_gather(d, x, y, taken), z, sa[to.at(x, y)], gd, ga);
        if (ddepth) ddepth[i] = gd;
        if (dalpha) dalpha[i] = ga;
    }
}

}  // namespace gsr

using namespace gsr;

static bool nrm_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int nrm_check_ptr(const char *who, const char *name, const void *p, uintptr_t align)
{
    if (!p) { set_error("%s: %s is NULL", who, name); return GSR_ERR_INVALID_ARGUMENT; }
    if (!nrm_aligned(p, align)) { set_error("%s: %s must be %d-byte aligned", who, name, (int)align); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int nrm_check_image(const char *who, int H, int W, float tanfovx, float tanfovy, float alpha_min)
{
    if (H < 0 || W < 0 || H > 32768 || W > 32768) {
        set_error("%s: image height = %d, width = %d (0 .. 32768 each)", who, H, W);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(tanfovx > 0.f) || !(tanfovy > 0.f) || isinf(tanfovx) || isinf(tanfovy)) {
        set_error("%s: tanfovx = %g, tanfovy = %g (positive and finite)", who, tanfovx, tanfovy);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(alpha_min > 0.f) || isinf(alpha_min)) {
        set_error("%s: alpha_min = %g (positive and finite: z = depth / alpha is taken where alpha >= alpha_min)", who, alpha_min);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int nrm_tiles(int H, int W, int &nbx) { nbx = (W + kNrmTileW - 1) / kNrmTileW; return nbx * ((H + kNrmTileH - 1) / kNrmTileH); }

static int nrm_check_gaussians(const char *who, int64_t P)
{
    if (P < 0 || P > (int64_t)kNrmBlock * 0x7fffffffLL) { set_error("%s: P=%lld", who, (long long)P); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

extern "C" int gsr_gaussian_normals_forward(int64_t P, const float *scales, const float *rotations, const float *means3D, const float *viewmatrix,
                                            const float *campos, float *normals_out, void *stream)
{
    const char *who = "gsr_gaussian_normals_forward";
    if (int rc = nrm_check_gaussians(who, P)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = nrm_check_ptr(who, "scales", scales, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "rotations", rotations, 16)) return rc;
    if (int rc = nrm_check_ptr(who, "means3D", means3D, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "viewmatrix", viewmatrix, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "campos", campos, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "normals_out", normals_out, 4)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("gaussian_normals_fwd", s);
    hipLaunchKernelGGL(k_gaussian_normals_fwd, dim3((unsigned)((P + kNrmBlock - 1) / kNrmBlock)), dim3(kNrmBlock), 0, s, P,
                       reinterpret_cast<const Row3 *>(scales), reinterpret_cast<const float4 *>(rotations), reinterpret_cast<const Row3 *>(means3D),
                       viewmatrix, campos, reinterpret_cast<Row3 *>(normals_out));
    GSR_LAUNCH_CHECK("gaussian_normals_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_gaussian_normals_backward(int64_t P, const float *scales, const float *rotations, const float *means3D, const float *viewmatrix,
                                             const float *campos, const float *grad_normals, float *grad_rotations, void *stream)
{
    const char *who = "gsr_gaussian_normals_backward";
    if (int rc = nrm_check_gaussians(who, P)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = nrm_check_ptr(who, "scales", scales, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "rotations", rotations, 16)) return rc;
    if (int rc = nrm_check_ptr(who, "means3D", means3D, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "viewmatrix", viewmatrix, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "campos", campos, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "grad_normals", grad_normals, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "grad_rotations", grad_rotations, 16)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("gaussian_normals_bwd", s);
    hipLaunchKernelGGL(k_gaussian_normals_bwd, dim3((unsigned)((P + kNrmBlock - 1) / kNrmBlock)), dim3(kNrmBlock), 0, s, P,
                       reinterpret_cast<const Row3 *>(scales), reinterpret_cast<const float4 *>(rotations), reinterpret_cast<const Row3 *>(means3D),
                       viewmatrix, campos, reinterpret_cast<const Row3 *>(grad_normals), reinterpret_cast<float4 *>(grad_rotations));
    GSR_LAUNCH_CHECK("gaussian_normals_bwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_depth_normal_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth, const float *alpha,
                                        float *normal_out, void *stream)
{
    const char *who = "gsr_depth_normal_forward";
    if (int rc = nrm_check_image(who, H, W, tanfovx, tanfovy, alpha_min)) return rc;
    if (H == 0 || W == 0) return GSR_OK;
    if (int rc = nrm_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "normal_out", normal_out, 4)) return rc;
    const NrmDims d = nrm_dims(H, W, tanfovx, tanfovy, alpha_min);
    int nbx;
    const int blocks = nrm_tiles(H, W, nbx);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("depth_normal_fwd", s);
    hipLaunchKernelGGL(k_depth_normal_fwd<false>, dim3((unsigned)blocks), dim3(kNrmBlock), 0, s, d, nbx, blocks, depth, alpha, (const float *)nullptr,
                       normal_out, (unsigned int *)nullptr, (float *)nullptr, 0.0);
    GSR_LAUNCH_CHECK("depth_normal_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_depth_normal_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *depth, const float *alpha,
                                         const float *grad_normal, float *grad_depth, float *grad_alpha, void *stream)
{
    const char *who = "gsr_depth_normal_backward";
    if (int rc = nrm_check_image(who, H, W, tanfovx, tanfovy, alpha_min)) return rc;
    if (H == 0 || W == 0 || (!grad_depth && !grad_alpha)) return GSR_OK;
    if (int rc = nrm_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "grad_normal", grad_normal, 4)) return rc;
    if (!nrm_aligned(grad_depth, 4) || !nrm_aligned(grad_alpha, 4)) { set_error("%s: grad_depth and grad_alpha must be 4-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    const NrmDims d = nrm_dims(H, W, tanfovx, tanfovy, alpha_min);
    int nbx;
    const int blocks = nrm_tiles(H, W, nbx);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("depth_normal_bwd", s);
    hipLaunchKernelGGL(k_depth_normal_bwd<false>, dim3((unsigned)blocks), dim3(kNrmBlock), 0, s, d, nbx, depth, alpha, grad_normal,
                       (const float *)nullptr, 0.f, (float *)nullptr, grad_depth, grad_alpha);
    GSR_LAUNCH_CHECK("depth_normal_bwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_normal_consistency_workspace_size(int32_t H, int32_t W, size_t *bytes)
{
    const char *who = "gsr_normal_consistency_workspace_size";
    if (int rc = nrm_check_image(who, H, W, 1.f, 1.f, 1.f)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    int nbx;
    *bytes = kNrmTicketBytes + align_up((size_t)nrm_tiles(H, W, nbx) * sizeof(float));
    return GSR_OK;
}

extern "C" int gsr_normal_consistency_forward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *normal_map,
                                              const float *depth, const float *alpha, void *workspace, size_t workspace_bytes, float *loss_out,
                                              void *stream)
{
    const char *who = "gsr_normal_consistency_forward";
    if (int rc = nrm_check_image(who, H, W, tanfovx, tanfovy, alpha_min)) return rc;
    if (H == 0 || W == 0) { set_error("%s: an image of %d x %d pixels has no mean", who, H, W); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = nrm_check_ptr(who, "normal_map", normal_map, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "workspace", workspace, 256)) return rc;
    if (int rc = nrm_check_ptr(who, "loss_out", loss_out, 4)) return rc;
    int nbx;
    const int blocks = nrm_tiles(H, W, nbx);
    const size_t need = kNrmTicketBytes + align_up((size_t)blocks * sizeof(float));
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    const NrmDims d = nrm_dims(H, W, tanfovx, tanfovy, alpha_min);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("normal_consistency_fwd", s);
    hipLaunchKernelGGL(k_depth_normal_fwd<true>, dim3((unsigned)(blocks < kNrmMaxBlocks ? blocks : kNrmMaxBlocks)), dim3(kNrmBlock), 0, s, d, nbx, blocks,
                       depth, alpha, normal_map, loss_out,
                       static_cast<unsigned int *>(workspace), reinterpret_cast<float *>(static_cast<char *>(workspace) + kNrmTicketBytes),
                       1.0 / ((double)H * (double)W));
    GSR_LAUNCH_CHECK("normal_consistency_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_normal_consistency_backward(int32_t H, int32_t W, float tanfovx, float tanfovy, float alpha_min, const float *normal_map,
                                               const float *depth, const float *alpha, const float *grad_loss, float *grad_normal_map,
                                               float *grad_depth, float *grad_alpha, void *stream)
{
    const char *who = "gsr_normal_consistency_backward";
    if (int rc = nrm_check_image(who, H, W, tanfovx, tanfovy, alpha_min)) return rc;
    if (H == 0 || W == 0 || (!grad_normal_map && !grad_depth && !grad_alpha)) return GSR_OK;
    if (int rc = nrm_check_ptr(who, "normal_map", normal_map, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "depth", depth, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "alpha", alpha, 4)) return rc;
    if (int rc = nrm_check_ptr(who, "grad_loss", grad_loss, 4)) return rc;
    if (!nrm_aligned(grad_normal_map, 4) || !nrm_aligned(grad_depth, 4) || !nrm_aligned(grad_alpha, 4)) {
        set_error("%s: grad_normal_map, grad_depth and grad_alpha must be 4-byte aligned", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const NrmDims d = nrm_dims(H, W, tanfovx, tanfovy, alpha_min);
    int nbx;
    const int blocks = nrm_tiles(H, W, nbx);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("normal_consistency_bwd", s);
    hipLaunchKernelGGL(k_depth_normal_bwd<true>, dim3((unsigned)blocks), dim3(kNrmBlock), 0, s, d, nbx, depth, alpha, normal_map, grad_loss,
                       (float)(1.0 / ((double)H * (double)W)), grad_normal_map, grad_depth, grad_alpha);
    GSR_LAUNCH_CHECK("normal_consistency_bwd", false, s);
    return GSR_OK;
}
