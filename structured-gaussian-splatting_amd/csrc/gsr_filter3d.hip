// gsr_filter3d.hip — Mip-Splatting's 3D smoothing filter (include/gsrast.h gsr_filter3d_*; the per-Gaussian rule is written once in
// gsr_filter3d_math.h).
//
// Filter size: k_filter3d_min_depth keeps one Gaussian's centre in registers and walks the whole camera table, staged in LDS
// kF3dCamChunk cameras at a time (every lane reads the same LDS address: one broadcast read, not 64 vector loads); it writes the
// minimum depth over the cameras that see the Gaussian and, per block, the maximum of those minima.  k_filter3d_finish reduces the
// blocks' maxima, gives it to the Gaussians no camera saw and scales by sqrt(0.2) / F.  Two launches whatever the number of
// cameras; min and max are exact, so the same inputs give the same bits and so does any order of the cameras.
//
// Application: k_filter3d_apply_fwd / _bwd, one thread per Gaussian, every row from its own inputs only.  HBM traffic per Gaussian:
// forward 20 B in (scales 12, opacity 4, filter 4), 16 B out; backward 36 B in, 16 B out.  Rows of three floats are read and written
// as 12-byte vectors.
#include "gsr_internal.h"
#include "gsr_filter3d_math.h"

namespace gsr {

constexpr int kF3dBlock = 256;
constexpr int kF3dWaves = kF3dBlock / kWave;
constexpr int kF3dCamChunk = 64;                 // cameras in LDS at once: 4 KB
constexpr int kF3dFinishBlocks = 1024;           // at most: every block of the finish re-reduces the partial maxima (L2 hits)
constexpr int64_t kF3dMaxP = (int64_t)1 << 30;

struct Row3 { float v[3]; };                     // a [P,3] row: 4-byte aligned, moved as one 12-byte access

__device__ __forceinline__ float block_max(float v, float *sh_wave)
{
    v = wave_max(v);
    if ((threadIdx.x & (kWave - 1)) == 0) sh_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = sh_wave[0];
#pragma unroll
    for (int w = 1; w < kF3dWaves; ++w) m = fmaxf(m, sh_wave[w]);
    return m;
}

__global__ __launch_bounds__(kF3dBlock) void k_filter3d_min_depth(int P, int C, const float *__restrict__ cams,
                                                                  const float *__restrict__ xyz, float *__restrict__ depth,
                                                                  float *__restrict__ block_maxima)
{
    __shared__ __align__(16) float sh_cam[kF3dCamChunk * kF3dCamFloats];
    __shared__ float sh_wave[kF3dWaves];
    const int i = blockIdx.x * kF3dBlock + threadIdx.x;
    const bool live = i < P;
    float p[3] = {0.f, 0.f, 0.f};
    if (live) {
        const Row3 r = reinterpret_cast<const Row3 *>(xyz)[i];
        p[0] = r.v[0]; p[1] = r.v[1]; p[2] = r.v[2];
    }
    float d = kF3dUnseen;
    for (int c0 = 0; c0 < C; c0 += kF3dCamChunk) {
        const int n = min(kF3dCamChunk, C - c0);
        if (c0) __syncthreads();                                     // the previous chunk has been read by every wave
        const float4 *src = reinterpret_cast<const float4 *>(cams) + (size_t)c0 * (kF3dCamFloats / 4);
        for (int k = threadIdx.x; k < n * (kF3dCamFloats / 4); k += kF3dBlock) reinterpret_cast<float4 *>(sh_cam)[k] = src[k];
        __syncthreads();
        for (int c = 0; c < n; ++c) d = filter3d_depth_step(p, sh_cam + c * kF3dCamFloats, d);
    }
    if (live) depth[i] = d;
    const float m = block_max(live && d < kF3dUnseen ? d : -1.f, sh_wave);          // depths are > 0.2: -1 = nobody in this block
    if (threadIdx.x == 0) block_maxima[blockIdx.x] = m;
}

// filter[i] = (depth[i], or the maximum over the seen Gaussians where nobody saw i) * scale; in place on `filter` (depth == filter).
// max_out[0] = that maximum, -1 if no Gaussian was seen (every filter is then 0: the caller's error).
__global__ __launch_bounds__(kF3dBlock) void k_filter3d_finish(int P, int n_partials, const float *__restrict__ block_maxima,
                                                               float scale, float *filter, float *__restrict__ max_out)
{
    __shared__ float sh_wave[kF3dWaves];
    float m = -1.f;
    for (int k = threadIdx.x; k < n_partials; k += kF3dBlock) m = fmaxf(m, block_maxima[k]);
    m = block_max(m, sh_wave);
    if (blockIdx.x == 0 && threadIdx.x == 0) max_out[0] = m;
    const float fill = m > 0.f ? m : 0.f;
    for (int i = blockIdx.x * kF3dBlock + threadIdx.x; i < P; i += gridDim.x * kF3dBlock) filter[i] = filter3d_finish_one(filter[i], fill, scale);
}

template <bool RAW>
__global__ __launch_bounds__(kF3dBlock) void k_filter3d_apply_fwd(int P, const float *__restrict__ opac, const float *__restrict__ scales,
                                                                  const float *__restrict__ filter, float *__restrict__ opac_out,
                                                                  float *__restrict__ scales_out)
{
    const int i = blockIdx.x * kF3dBlock + threadIdx.x;
    if (i >= P) return;
    const Row3 s = reinterpret_cast<const Row3 *>(scales)[i];
    Row3 so;
    float oo;
    filter3d_apply_one<RAW>(s.v, opac[i], filter[i], so.v, oo);
    opac_out[i] = oo;
    reinterpret_cast<Row3 *>(scales_out)[i] = so;
}

// g_opac / g_scales: the incoming gradients, NULL = zero; d_opac / d_scales: NULL = not wanted
template <bool RAW>
__global__ __launch_bounds__(kF3dBlock) void k_filter3d_apply_bwd(int P, const float *__restrict__ opac, const float *__restrict__ scales,
                                                                  const float *__restrict__ filter, const float *__restrict__ g_opac,
                                                                  const float *__restrict__ g_scales, float *__restrict__ d_opac,
                                                                  float *__restrict__ d_scales)
{
    const int i = blockIdx.x * kF3dBlock + threadIdx.x;
    if (i >= P) return;
    const Row3 s = reinterpret_cast<const Row3 *>(scales)[i];
    Row3 gs = {{0.f, 0.f, 0.f}}, ds;
    if (g_scales) gs = reinterpret_cast<const Row3 *>(g_scales)[i];
    const float go = g_opac ? g_opac[i] : 0.f;
    float dop;
    filter3d_apply_backward_one<RAW>(s.v, opac[i], filter[i], gs.v, go, ds.v, dop);
    if (d_opac) d_opac[i] = dop;
    if (d_scales) reinterpret_cast<Row3 *>(d_scales)[i] = ds;
}

}  // namespace gsr

using namespace gsr;

static bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
static int f3d_blocks(int64_t P) { return (int)((P + kF3dBlock - 1) / kF3dBlock); }
static size_t f3d_workspace_bytes(int64_t P) { return align_up(sizeof(float) * (size_t)(1 + f3d_blocks(P))); }

// 0 = go on; every check comes before any device work and names its argument
static int f3d_check_P(const char *who, int64_t P)
{
    if (P < 0 || P > kF3dMaxP) { set_error("%s: P=%lld (0 .. 2^30)", who, (long long)P); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int f3d_check_ptr(const char *who, const char *name, const void *p, uintptr_t align, bool required)
{
    if (!p) {
        if (!required) return GSR_OK;
        set_error("%s: %s is NULL", who, name);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned_to(p, align)) { set_error("%s: %s must be %d-byte aligned", who, name, (int)align); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

extern "C" int gsr_filter3d_workspace_size(int64_t P, size_t *bytes)
{
    const char *who = "gsr_filter3d_workspace_size";
    if (int rc = f3d_check_P(who, P)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = f3d_workspace_bytes(P);
    return GSR_OK;
}

extern "C" int gsr_filter3d_compute(int64_t P, int32_t C, const float *cameras, float focal_max, const float *xyz, float *filter_out,
                                    void *workspace, size_t workspace_bytes, int32_t *any_seen, void *stream)
{
    const char *who = "gsr_filter3d_compute";
    if (int rc = f3d_check_P(who, P)) return rc;
    if (C <= 0) { set_error("%s: C=%d (at least one camera)", who, C); return GSR_ERR_INVALID_ARGUMENT; }
    if (!(focal_max > 0.f) || !(focal_max < INFINITY)) { set_error("%s: focal_max=%g (positive and finite)", who, (double)focal_max); return GSR_ERR_INVALID_ARGUMENT; }
    if (P == 0) { if (any_seen) *any_seen = 0; return GSR_OK; }
    if (int rc = f3d_check_ptr(who, "cameras", cameras, 16, true)) return rc;
    if (int rc = f3d_check_ptr(who, "xyz", xyz, 4, true)) return rc;
    if (int rc = f3d_check_ptr(who, "filter_out", filter_out, 4, true)) return rc;
    if (int rc = f3d_check_ptr(who, "workspace", workspace, 4, true)) return rc;
    if (workspace_bytes < f3d_workspace_bytes(P)) {
        set_error("%s: workspace_bytes=%zu, gsr_filter3d_workspace_size says %zu", who, workspace_bytes, f3d_workspace_bytes(P));
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    float *max_out = static_cast<float *>(workspace), *partials = max_out + 1;
    const int blocks = f3d_blocks(P);
    {
        ProfileScope prof("filter3d_min_depth", s);
        hipLaunchKernelGGL(k_filter3d_min_depth, dim3(blocks), dim3(kF3dBlock), 0, s, (int)P, (int)C, cameras, xyz, filter_out, partials);
        GSR_LAUNCH_CHECK("filter3d_min_depth", false, s);
    }
    {
        ProfileScope prof("filter3d_finish", s);
        hipLaunchKernelGGL(k_filter3d_finish, dim3(blocks < kF3dFinishBlocks ? blocks : kF3dFinishBlocks), dim3(kF3dBlock), 0, s, (int)P, blocks,
                           partials, filter3d_scale(focal_max), filter_out, max_out);
        GSR_LAUNCH_CHECK("filter3d_finish", false, s);
    }
    if (any_seen) {                              // the one host synchronisation: was any Gaussian seen at all
        float m = -1.f;
        GSR_HIP_CHECK(hipMemcpyAsync(&m, max_out, sizeof(float), hipMemcpyDeviceToHost, s));
        GSR_HIP_CHECK(hipStreamSynchronize(s));
        *any_seen = m > 0.f ? 1 : 0;
    }
    return GSR_OK;
}

static int f3d_check_apply(const char *who, int64_t P, const float *opacities, const float *scales, const float *filter)
{
    if (int rc = f3d_check_ptr(who, "opacities", opacities, 4, true)) return rc;
    if (int rc = f3d_check_ptr(who, "scales", scales, 4, true)) return rc;
    return f3d_check_ptr(who, "filter", filter, 4, true);
}

extern "C" int gsr_filter3d_apply_forward(int64_t P, int32_t raw, const float *opacities, const float *scales, const float *filter,
                                          float *opacities_out, float *scales_out, void *stream)
{
    const char *who = "gsr_filter3d_apply_forward";
    if (int rc = f3d_check_P(who, P)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = f3d_check_apply(who, P, opacities, scales, filter)) return rc;
    if (int rc = f3d_check_ptr(who, "opacities_out", opacities_out, 4, true)) return rc;
    if (int rc = f3d_check_ptr(who, "scales_out", scales_out, 4, true)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const dim3 blocks(f3d_blocks(P)), threads(kF3dBlock);
    ProfileScope prof("filter3d_apply_fwd", s);
    if (raw) hipLaunchKernelGGL(k_filter3d_apply_fwd<true>, blocks, threads, 0, s, (int)P, opacities, scales, filter, opacities_out, scales_out);
    else hipLaunchKernelGGL(k_filter3d_apply_fwd<false>, blocks, threads, 0, s, (int)P, opacities, scales, filter, opacities_out, scales_out);
    GSR_LAUNCH_CHECK("filter3d_apply_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_filter3d_apply_backward(int64_t P, int32_t raw, const float *opacities, const float *scales, const float *filter,
                                           const float *grad_opacities_out, const float *grad_scales_out, float *grad_opacities,
                                           float *grad_scales, void *stream)
{
    const char *who = "gsr_filter3d_apply_backward";
    if (int rc = f3d_check_P(who, P)) return rc;
    if (P == 0) return GSR_OK;
    if (int rc = f3d_check_apply(who, P, opacities, scales, filter)) return rc;
    if (int rc = f3d_check_ptr(who, "grad_opacities_out", grad_opacities_out, 4, false)) return rc;
    if (int rc = f3d_check_ptr(who, "grad_scales_out", grad_scales_out, 4, false)) return rc;
    if (int rc = f3d_check_ptr(who, "grad_opacities", grad_opacities, 4, false)) return rc;
    if (int rc = f3d_check_ptr(who, "grad_scales", grad_scales, 4, false)) return rc;
    if (!grad_opacities && !grad_scales) return GSR_OK;              // nothing wanted
    hipStream_t s = (hipStream_t)stream;
    const dim3 blocks(f3d_blocks(P)), threads(kF3dBlock);
    ProfileScope prof("filter3d_apply_bwd", s);
    if (raw) hipLaunchKernelGGL(k_filter3d_apply_bwd<true>, blocks, threads, 0, s, (int)P, opacities, scales, filter, grad_opacities_out, grad_scales_out, grad_opacities, grad_scales);
    else hipLaunchKernelGGL(k_filter3d_apply_bwd<false>, blocks, threads, 0, s, (int)P, opacities, scales, filter, grad_opacities_out, grad_scales_out, grad_opacities, grad_scales);
    GSR_LAUNCH_CHECK("filter3d_apply_bwd", false, s);
    return GSR_OK;
}
