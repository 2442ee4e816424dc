// gsr_distortion.hip — the depth-distortion loss (Mip-NeRF 360's, in the squared form of 2DGS; include/gsrast_distortion.h; DESIGN
// section 29).  The arithmetic of one Gaussian and of one pixel lives in gsr_distortion_math.h; the kernels here load, call, store and
// sum.  No atomic anywhere: every sum has an order the program fixes, so the same inputs give the same bits.
//
//   k_depth_moments_fwd / _bwd   one launch each, a thread per Gaussian: 12 B read and 12 B written forward; the backward reads the
//                       same 12 B and dL/dmoments (12 B), recomputes z and m, and writes dL/dmeans3D (12 B).
//   k_distortion_fwd<kLoss>      one launch, a block per 1 024 consecutive pixels, four consecutive pixels per thread (one 16-byte
//                       load per plane where the planes are 16-byte aligned, four 4-byte loads of the same pixels where not: the
//                       pixels a thread owns, and with them every sum's order, do not depend on the alignment).  kLoss = false
//                       writes D [H W]; kLoss = true writes no map: a thread adds its four D in pixel order, a wave its lanes'
//                       sums (butterfly), thread 0 the four waves' in wave order, and the block's sum goes to partials[block].
//   k_distortion_sum             one block, behind k_distortion_fwd<true> on the same stream: thread t adds partials[t], [t + 256],
//                       ... in ascending order in binary64, then lanes, then waves in order; the loss is (float)(total / (H W)).
//   k_distortion_bwd<kLoss>      one launch, the same pixels per thread: dL/dmoments [3,H W] (plane 2: zeros) and dL/dalpha [H W],
//                       either NULL (not wanted).  kLoss = false reads dL/dD [H W]; kLoss = true reads dL/dloss [1].
#include "gsr_internal.h"
#include "gsr_distortion_math.h"
#include "gsr_wave.h"
#include "../../include/gsrast_distortion.h"

namespace gsr {

constexpr int kDstBlock = 256;
constexpr int kDstVec = 4;                              // consecutive pixels of a thread
constexpr int kDstBlockPx = kDstBlock * kDstVec;        // pixels of a block: one partial sum of the loss each
constexpr int kDstSumBlock = 256;                       // threads of the second stage: that many partials per trip

struct DstRow3 { float v[3]; };                         // a [P,3] row: 4-byte aligned, moved as one 12-byte access
struct DstPx { float v[kDstVec]; };

__global__ __launch_bounds__(kDstBlock) void k_depth_moments_fwd(int64_t P, DstMapping map, const DstRow3 *__restrict__ means,
                                                                 const float *__restrict__ V, DstRow3 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * kDstBlock + threadIdx.x;
    if (i >= P) return;
    const DstRow3 m = means[i];
    DstRow3 o;
    dst_moments_one(map, m.v, V, o.v);
    out[i] = o;
}

__global__ __launch_bounds__(kDstBlock) void k_depth_moments_bwd(int64_t P, DstMapping map, const DstRow3 *__restrict__ means,
                                                                 const float *__restrict__ V, const DstRow3 *__restrict__ gout,
                                                                 DstRow3 *__restrict__ dmeans)
{
    const int64_t i = (int64_t)blockIdx.x * kDstBlock + threadIdx.x;
    if (i >= P) return;
    const DstRow3 m = means[i], g = gout[i];
    DstRow3 d;
    dst_moments_backward_one(map, m.v, V, g.v, d.v);
    dmeans[i] = d;
}

// p[i0 .. i0 + 3], a pixel at or behind n as 0.  vec (uniform over the grid): p + i0 is 16-byte aligned and n is a multiple of 4
__device__ __forceinline__ DstPx dst_load(const float *__restrict__ p, int64_t i0, int64_t n, bool vec)
{
    DstPx r;
    if (vec) {
        const float4 t = *reinterpret_cast<const float4 *>(p + i0);
        r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w;
    } else {
#pragma unroll
        for (int k = 0; k < kDstVec; ++k) r.v[k] = i0 + k < n ? p[i0 + k] : 0.f;
    }
    return r;
}

__device__ __forceinline__ void dst_store(float *__restrict__ p, int64_t i0, int64_t n, bool vec, const DstPx &r)
{
    if (vec) {
        *reinterpret_cast<float4 *>(p + i0) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kDstVec; ++k) if (i0 + k < n) p[i0 + k] = r.v[k];
    }
}

// moments: [3, n], planes 0 (M1) and 1 (M2) are read.  out: D [n] (kLoss = false) or the blocks' sums [gridDim.x] (kLoss = true)
template <bool kLoss>
__global__ __launch_bounds__(kDstBlock) void k_distortion_fwd(int64_t n, int vec, const float *__restrict__ moments, const float *__restrict__ alpha,
                                                              float *__restrict__ out)
{
    const int64_t i0 = ((int64_t)blockIdx.x * kDstBlock + threadIdx.x) * kDstVec;
    DstPx D = {{0.f, 0.f, 0.f, 0.f}};
    if (i0 < n) {
        const DstPx M1 = dst_load(moments, i0, n, vec), M2 = dst_load(moments + n, i0, n, vec), A = dst_load(alpha, i0, n, vec);
#pragma unroll
        for (int k = 0; k < kDstVec; ++k) D.v[k] = dst_pixel(A.v[k], M1.v[k], M2.v[k]);        // (a pixel behind n: fma(0, 0, -0) = +0)
        if constexpr (!kLoss) dst_store(out, i0, n, vec, D);
    }
    if constexpr (kLoss) {
        __shared__ float sh_wave[kDstBlock / kWave];
        float acc = ((D.v[0] + D.v[1]) + D.v[2]) + D.v[3];
        acc = wave_sum(acc);
        if ((threadIdx.x & (kWave - 1)) == 0) sh_wave[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            float b = sh_wave[0];
            for (int w = 1; w < kDstBlock / kWave; ++w) b += sh_wave[w];
            out[blockIdx.x] = b;
        }
    }
}

__global__ __launch_bounds__(kDstSumBlock) void k_distortion_sum(int nparts, const float *__restrict__ parts, double inv_n, float *__restrict__ loss_out)
{
    __shared__ double sh_wave[kDstSumBlock / kWave];
    double t = 0.0;
    for (int b = threadIdx.x; b < nparts; b += kDstSumBlock) t += (double)parts[b];
    t = wave_sum(t);
    if ((threadIdx.x & (kWave - 1)) == 0) sh_wave[threadIdx.x >> 6] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        double all = sh_wave[0];
        for (int w = 1; w < kDstSumBlock / kWave; ++w) all += sh_wave[w];
        loss_out[0] = (float)(all * inv_n);
    }
}

// gin: dL/dD [n] (kLoss = false) or dL/dloss [1] (kLoss = true).  dmom [3, n] and dalpha [n]: either may be NULL
template <bool kLoss>
__global__ __launch_bounds__(kDstBlock) void k_distortion_bwd(int64_t n, int vec, const float *__restrict__ moments, const float *__restrict__ alpha,
                                                              const float *__restrict__ gin, float *__restrict__ dmom, float *__restrict__ dalpha)
{
    const int64_t i0 = ((int64_t)blockIdx.x * kDstBlock + threadIdx.x) * kDstVec;
    if (i0 >= n) return;
    const DstPx M1 = dst_load(moments, i0, n, vec), M2 = dst_load(moments + n, i0, n, vec), A = dst_load(alpha, i0, n, vec);
    DstPx g;
    if constexpr (kLoss) {
        const float s = dst_loss_scale(gin[0], n);
        g = {{s, s, s, s}};
    } else {
        g = dst_load(gin, i0, n, vec);
    }
    DstPx dA, dM1, dM2;
#pragma unroll
    for (int k = 0; k < kDstVec; ++k) dst_pixel_backward(g.v[k], A.v[k], M1.v[k], M2.v[k], dA.v[k], dM1.v[k], dM2.v[k]);
    if (dmom) {
        const DstPx zero = {{0.f, 0.f, 0.f, 0.f}};
        dst_store(dmom, i0, n, vec, dM1);
        dst_store(dmom + n, i0, n, vec, dM2);
        dst_store(dmom + 2 * n, i0, n, vec, zero);
    }
    if (dalpha) dst_store(dalpha, i0, n, vec, dA);
}

}  // namespace gsr

using namespace gsr;

static bool dst_aligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

static int dst_check_ptr(const char *who, const char *name, const void *p)
{
    if (!p) { set_error("%s: %s is NULL", who, name); return GSR_ERR_INVALID_ARGUMENT; }
    if (!dst_aligned(p, 4)) { set_error("%s: %s must be 4-byte aligned", who, name); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int dst_check_image(const char *who, int H, int W)
{
    if (H < 0 || W < 0 || H > 32768 || W > 32768) {
        set_error("%s: image height = %d, width = %d (0 .. 32768 each)", who, H, W);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int dst_check_gaussians(const char *who, int64_t P, int mapping, float near_plane, float far_plane)
{
    if (P < 0 || P > (int64_t)kDstBlock * 0x7fffffffLL) { set_error("%s: P=%lld", who, (long long)P); return GSR_ERR_INVALID_ARGUMENT; }
    if (mapping != GSR_DISTORTION_NDC && mapping != GSR_DISTORTION_LINEAR) {
        set_error("%s: mapping = %d (GSR_DISTORTION_NDC = 0 or GSR_DISTORTION_LINEAR = 1)", who, mapping);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(near_plane > 0.f) || !(far_plane > near_plane) || isinf(far_plane)) {
        set_error("%s: near = %g, far = %g (0 < near < far, finite)", who, near_plane, far_plane);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int dst_blocks(int H, int W) { return (int)(((int64_t)H * W + kDstBlockPx - 1) / kDstBlockPx); }

// the 16-byte path: every plane the kernel touches starts on a 16-byte boundary (NULL: not touched)
static int dst_vec(int64_t n, const void *a, const void *b, const void *c, const void *d, const void *e)
{
    return n % kDstVec == 0 && dst_aligned(a, 16) && dst_aligned(b, 16) && dst_aligned(c, 16) && dst_aligned(d, 16) && dst_aligned(e, 16);
}

extern "C" int gsr_depth_moments_forward(int64_t P, const float *means3D, const float *viewmatrix, int32_t mapping, float near_plane,
                                         float far_plane, float *moments_out, void *stream)
{
    const char *who = "gsr_depth_moments_forward";
    if (int rc = dst_check_gaussians(who, P, mapping, near_plane, far_plane)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = dst_check_ptr(who, "means3D", means3D)) return rc;
    if (int rc = dst_check_ptr(who, "viewmatrix", viewmatrix)) return rc;
    if (int rc = dst_check_ptr(who, "moments_out", moments_out)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("depth_moments_fwd", s);
    hipLaunchKernelGGL(k_depth_moments_fwd, dim3((unsigned)((P + kDstBlock - 1) / kDstBlock)), dim3(kDstBlock), 0, s, P,
                       dst_mapping(mapping, near_plane, far_plane), reinterpret_cast<const DstRow3 *>(means3D), viewmatrix,
                       reinterpret_cast<DstRow3 *>(moments_out));
    GSR_LAUNCH_CHECK("depth_moments_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_depth_moments_backward(int64_t P, const float *means3D, const float *viewmatrix, int32_t mapping, float near_plane,
                                          float far_plane, const float *grad_moments, float *grad_means3D, void *stream)
{
    const char *who = "gsr_depth_moments_backward";
    if (int rc = dst_check_gaussians(who, P, mapping, near_plane, far_plane)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = dst_check_ptr(who, "means3D", means3D)) return rc;
    if (int rc = dst_check_ptr(who, "viewmatrix", viewmatrix)) return rc;
    if (int rc = dst_check_ptr(who, "grad_moments", grad_moments)) return rc;
    if (int rc = dst_check_ptr(who, "grad_means3D", grad_means3D)) return rc;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("depth_moments_bwd", s);
    hipLaunchKernelGGL(k_depth_moments_bwd, dim3((unsigned)((P + kDstBlock - 1) / kDstBlock)), dim3(kDstBlock), 0, s, P,
                       dst_mapping(mapping, near_plane, far_plane), reinterpret_cast<const DstRow3 *>(means3D), viewmatrix,
                       reinterpret_cast<const DstRow3 *>(grad_moments), reinterpret_cast<DstRow3 *>(grad_means3D));
    GSR_LAUNCH_CHECK("depth_moments_bwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_distortion_map_forward(int32_t H, int32_t W, const float *moments_map, const float *alpha, float *distortion_out, void *stream)
{
    const char *who = "gsr_distortion_map_forward";
    if (int rc = dst_check_image(who, H, W)) return rc;
    if (H == 0 || W == 0) return GSR_OK;
    if (int rc = dst_check_ptr(who, "moments_map", moments_map)) return rc;
    if (int rc = dst_check_ptr(who, "alpha", alpha)) return rc;
    if (int rc = dst_check_ptr(who, "distortion_out", distortion_out)) return rc;
    const int64_t n = (int64_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("distortion_map_fwd", s);
    hipLaunchKernelGGL(k_distortion_fwd<false>, dim3((unsigned)dst_blocks(H, W)), dim3(kDstBlock), 0, s, n,
                       dst_vec(n, moments_map, alpha, distortion_out, nullptr, nullptr), moments_map, alpha, distortion_out);
    GSR_LAUNCH_CHECK("distortion_map_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_distortion_map_backward(int32_t H, int32_t W, const float *moments_map, const float *alpha, const float *grad_distortion,
                                           float *grad_moments_map, float *grad_alpha, void *stream)
{
    const char *who = "gsr_distortion_map_backward";
    if (int rc = dst_check_image(who, H, W)) return rc;
    if (H == 0 || W == 0 || (!grad_moments_map && !grad_alpha)) return GSR_OK;
    if (int rc = dst_check_ptr(who, "moments_map", moments_map)) return rc;
    if (int rc = dst_check_ptr(who, "alpha", alpha)) return rc;
    if (int rc = dst_check_ptr(who, "grad_distortion", grad_distortion)) return rc;
    if (!dst_aligned(grad_moments_map, 4) || !dst_aligned(grad_alpha, 4)) {
        set_error("%s: grad_moments_map and grad_alpha must be 4-byte aligned", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t n = (int64_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("distortion_map_bwd", s);
    hipLaunchKernelGGL(k_distortion_bwd<false>, dim3((unsigned)dst_blocks(H, W)), dim3(kDstBlock), 0, s, n,
                       dst_vec(n, moments_map, alpha, grad_distortion, grad_moments_map, grad_alpha), moments_map, alpha, grad_distortion,
                       grad_moments_map, grad_alpha);
    GSR_LAUNCH_CHECK("distortion_map_bwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_distortion_loss_workspace_size(int32_t H, int32_t W, size_t *bytes)
{
    const char *who = "gsr_distortion_loss_workspace_size";
    if (int rc = dst_check_image(who, H, W)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = align_up((size_t)dst_blocks(H, W) * sizeof(float));
    return GSR_OK;
}

extern "C" int gsr_distortion_loss_forward(int32_t H, int32_t W, const float *moments_map, const float *alpha, void *workspace,
                                           size_t workspace_bytes, float *loss_out, void *stream)
{
    const char *who = "gsr_distortion_loss_forward";
    if (int rc = dst_check_image(who, H, W)) return rc;
    if (H == 0 || W == 0) { set_error("%s: an image of %d x %d pixels has no mean", who, H, W); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = dst_check_ptr(who, "moments_map", moments_map)) return rc;
    if (int rc = dst_check_ptr(who, "alpha", alpha)) return rc;
    if (int rc = dst_check_ptr(who, "workspace", workspace)) return rc;
    if (int rc = dst_check_ptr(who, "loss_out", loss_out)) return rc;
    const int blocks = dst_blocks(H, W);
    const size_t need = align_up((size_t)blocks * sizeof(float));
    if (workspace_bytes < need) { set_error("%s: workspace_bytes = %zu, %zu needed", who, workspace_bytes, need); return GSR_ERR_WORKSPACE; }
    const int64_t n = (int64_t)H * W;
    float *parts = static_cast<float *>(workspace);
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("distortion_loss_fwd", s);
    hipLaunchKernelGGL(k_distortion_fwd<true>, dim3((unsigned)blocks), dim3(kDstBlock), 0, s, n, dst_vec(n, moments_map, alpha, nullptr, nullptr, nullptr),
                       moments_map, alpha, parts);
    GSR_LAUNCH_CHECK("distortion_loss_fwd", false, s);
    hipLaunchKernelGGL(k_distortion_sum, dim3(1), dim3(kDstSumBlock), 0, s, blocks, parts, 1.0 / (double)n, loss_out);
    GSR_LAUNCH_CHECK("distortion_loss_sum", false, s);
    return GSR_OK;
}

extern "C" int gsr_distortion_loss_backward(int32_t H, int32_t W, const float *moments_map, const float *alpha, const float *grad_loss,
                                            float *grad_moments_map, float *grad_alpha, void *stream)
{
    const char *who = "gsr_distortion_loss_backward";
    if (int rc = dst_check_image(who, H, W)) return rc;
    if (H == 0 || W == 0 || (!grad_moments_map && !grad_alpha)) return GSR_OK;
    if (int rc = dst_check_ptr(who, "moments_map", moments_map)) return rc;
    if (int rc = dst_check_ptr(who, "alpha", alpha)) return rc;
    if (int rc = dst_check_ptr(who, "grad_loss", grad_loss)) return rc;
    if (!dst_aligned(grad_moments_map, 4) || !dst_aligned(grad_alpha, 4)) {
        set_error("%s: grad_moments_map and grad_alpha must be 4-byte aligned", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const int64_t n = (int64_t)H * W;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("distortion_loss_bwd", s);
    hipLaunchKernelGGL(k_distortion_bwd<true>, dim3((unsigned)dst_blocks(H, W)), dim3(kDstBlock), 0, s, n,
                       dst_vec(n, moments_map, alpha, nullptr, grad_moments_map, grad_alpha), moments_map, alpha, grad_loss, grad_moments_map,
                       grad_alpha);
    GSR_LAUNCH_CHECK("distortion_loss_bwd", false, s);
    return GSR_OK;
}
