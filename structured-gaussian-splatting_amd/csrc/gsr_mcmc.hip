// gsr_mcmc.hip — the MCMC densification strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo"; gsplat's MCMCStrategy):
// the relocation rule, the row edit that applies it, the per-iteration position noise and the regulariser gradient.  The
// arithmetic of one Gaussian lives in gsr_math.h (mcmc_relocation_one, mcmc_noise_one, mcmc_reg_*); the kernels here load, call and
// store.  DESIGN section 16.
//
//   gsr_mcmc_relocation    three launches over the n sampled sources, none over P: clear the sources' counters, count them (integer
//                          atomics: any order gives the same counts), then the binary64 rule from the OLD opacity and scale of
//                          every source into the two output arrays.  Nothing of the model is written.
//   gsr_mcmc_relocate_rows one launch over n x (sum of the tensors' widths) elements: new values into the source rows, source rows
//                          into the dead rows, zeros into the sources' moments.  It reads nothing it writes: the new opacity and
//                          scale come from the arrays of the call above, the copied tensors (means, SH, rotation) are never written
//                          at a source row, and dead rows and source rows are disjoint.  A source sampled k times is written k
//                          times with one value.
//   gsr_mcmc_inject_noise  one launch, a thread per FOUR Gaussians: 4 rows of a [P,3] tensor are three aligned float4, so the means,
//                          log-scales and noise are read (and the means written) as whole float4 with no row straddling a thread;
//                          the P % 4 last Gaussians take scalar loads.  56 B read, 12 B written per Gaussian, no atomics, no LDS.
//   gsr_mcmc_reg_grads     one launch, the two gradients as flat float4 streams (the walk of k_act_fwd), added in place.
#include "gsr_internal.h"

namespace gsr {

constexpr int kMcmcBlock = 256;

__global__ __launch_bounds__(kMcmcBlock) void k_mcmc_count(int64_t n, const int64_t *__restrict__ sampled, uint32_t *__restrict__ counts,
                                                           int add)
{
    const int64_t j = (int64_t)blockIdx.x * kMcmcBlock + threadIdx.x;
    if (j >= n) return;
    if (add) atomicAdd(&counts[sampled[j]], 1u);
    else counts[sampled[j]] = 0u;
}

__global__ __launch_bounds__(kMcmcBlock) void k_mcmc_rule(int64_t n, const float *__restrict__ opacity_raw, const float *__restrict__ scaling_raw,
                                                          const int64_t *__restrict__ sampled, const uint32_t *__restrict__ counts,
                                                          float min_opacity, float *__restrict__ new_opacity_raw,
                                                          float *__restrict__ new_scaling_raw)
{
    const int64_t j = (int64_t)blockIdx.x * kMcmcBlock + threadIdx.x;
    if (j >= n) return;
    const int64_t src = sampled[j];
    const uint32_t cnt = counts[src];
    const int N = cnt >= (uint32_t)GSR_MCMC_MAX_RATIO ? GSR_MCMC_MAX_RATIO : 1 + (int)cnt;
    const float sc[3] = {scaling_raw[3 * src], scaling_raw[3 * src + 1], scaling_raw[3 * src + 2]};
    float o, s[3];
    mcmc_relocation_one(opacity_raw[src], sc, N, min_opacity, o, s);
    new_opacity_raw[j] = o;
    new_scaling_raw[3 * j] = s[0]; new_scaling_raw[3 * j + 1] = s[1]; new_scaling_raw[3 * j + 2] = s[2];
}

struct McmcRows {
    float *p[GSR_MCMC_MAX_TENSORS], *m[GSR_MCMC_MAX_TENSORS], *v[GSR_MCMC_MAX_TENSORS];
    uint32_t width[GSR_MCMC_MAX_TENSORS], col_end[GSR_MCMC_MAX_TENSORS];      // col_end: running sum of the widths
    int32_t role[GSR_MCMC_MAX_TENSORS];
    int count;
};

// element e of the launch = (sampled entry j = e / W, column e % W of the tensors laid side by side, W = col_end[count - 1]):
// neighbouring threads walk one row of one tensor
__global__ __launch_bounds__(kMcmcBlock) void k_mcmc_rows(McmcRows a, unsigned long long total, const int64_t *__restrict__ sampled,
                                                          const int64_t *__restrict__ dead, const float *__restrict__ new_opacity_raw,
                                                          const float *__restrict__ new_scaling_raw)
{
    const uint32_t W = a.col_end[a.count - 1];
    const unsigned long long stride = (unsigned long long)gridDim.x * kMcmcBlock;
    for (unsigned long long e = (unsigned long long)blockIdx.x * kMcmcBlock + threadIdx.x; e < total; e += stride) {
        const unsigned long long j = e / W;
        const uint32_t c = (uint32_t)(e - j * W);
        // the tensor of column c, picked by selects over constant indices (a per-thread index into the argument struct would
        // move it to scratch); the host sets col_end[count ..] = W, so c never lands past tensor count - 1
        float *p = a.p[0], *m = a.m[0], *v = a.v[0];
        uint32_t w = a.width[0], begin = 0;
        int32_t role = a.role[0];
#pragma unroll
        for (int k = 1; k < GSR_MCMC_MAX_TENSORS; ++k)
            if (c >= a.col_end[k - 1]) { p = a.p[k]; m = a.m[k]; v = a.v[k]; w = a.width[k]; begin = a.col_end[k - 1]; role = a.role[k]; }
        const uint32_t col = c - begin;
        const size_t src = (size_t)sampled[j] * w + col;
        float val;
        if (role == GSR_MCMC_ROLE_COPY) val = p[src];
        else {
            val = role == GSR_MCMC_ROLE_OPACITY ? new_opacity_raw[j] : new_scaling_raw[3 * j + col];
            p[src] = val;
        }
        if (dead) {
            p[(size_t)dead[j] * w + col] = val;
            if (m) { m[src] = 0.f; v[src] = 0.f; }
        }
    }
}

__device__ __forceinline__ void noise_rows4(const float4 ls[3], const float4 q[4], const float4 op, const float4 xi[3], float c, float4 x[3])
{
    const float *lsf = reinterpret_cast<const float *>(ls), *xif = reinterpret_cast<const float *>(xi), *qf = reinterpret_cast<const float *>(q);
    const float *opf = reinterpret_cast<const float *>(&op);
    float *xf = reinterpret_cast<float *>(x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float d[3];
        mcmc_noise_one(lsf + 3 * r, qf + 4 * r, opf[r], xif + 3 * r, c, d);
        xf[3 * r] += d[0]; xf[3 * r + 1] += d[1]; xf[3 * r + 2] += d[2];
    }
}

__global__ __launch_bounds__(kMcmcBlock) void k_mcmc_noise(int64_t P, float *__restrict__ xyz, const float *__restrict__ scaling_raw,
                                                           const float *__restrict__ rotation_raw, const float *__restrict__ opacity_raw,
                                                           const float *__restrict__ noise, float c)
{
    const int64_t P4 = P / 4;
    const int64_t i = (int64_t)blockIdx.x * kMcmcBlock + threadIdx.x;
    if (i < P4) {
        float4 x[3], ls[3], xi[3], q[4];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            x[k] = reinterpret_cast<const float4 *>(xyz)[3 * i + k];
            ls[k] = reinterpret_cast<const float4 *>(scaling_raw)[3 * i + k];
            xi[k] = reinterpret_cast<const float4 *>(noise)[3 * i + k];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = reinterpret_cast<const float4 *>(rotation_raw)[4 * i + k];
        const float4 op = reinterpret_cast<const float4 *>(opacity_raw)[i];
        noise_rows4(ls, q, op, xi, c, x);
#pragma unroll
        for (int k = 0; k < 3; ++k) reinterpret_cast<float4 *>(xyz)[3 * i + k] = x[k];
    }
    // the P % 4 last Gaussians: the first threads of block 0
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < P - P4 * 4) {
        const int64_t r = P4 * 4 + threadIdx.x;
        float d[3];
        mcmc_noise_one(scaling_raw + 3 * r, rotation_raw + 4 * r, opacity_raw[r], noise + 3 * r, c, d);
        xyz[3 * r] += d[0]; xyz[3 * r + 1] += d[1]; xyz[3 * r + 2] += d[2];
    }
}

struct RegGrid { unsigned nb_s, nb_o; };

__global__ __launch_bounds__(kMcmcBlock) void k_mcmc_reg(int64_t P, RegGrid grid, const float *__restrict__ opacity_raw,
                                                         const float *__restrict__ scaling_raw, float k_o, float k_s,
                                                         float *__restrict__ grad_opacity, float *__restrict__ grad_scaling)
{
    unsigned b = blockIdx.x;
    if (b < grid.nb_s) {
        const int64_t n = 3 * P, n4 = n / 4, stride = (int64_t)grid.nb_s * kMcmcBlock;
        for (int64_t i = (int64_t)b * kMcmcBlock + threadIdx.x; i < n4; i += stride) {
            const float4 v = reinterpret_cast<const float4 *>(scaling_raw)[i];
            float4 g = reinterpret_cast<float4 *>(grad_scaling)[i];
            g.x += mcmc_reg_scale_one(v.x, k_s); g.y += mcmc_reg_scale_one(v.y, k_s);
            g.z += mcmc_reg_scale_one(v.z, k_s); g.w += mcmc_reg_scale_one(v.w, k_s);
            reinterpret_cast<float4 *>(grad_scaling)[i] = g;
        }
        if (b == 0 && (int64_t)threadIdx.x < n - n4 * 4) {
            const int64_t i = n4 * 4 + threadIdx.x;
            grad_scaling[i] += mcmc_reg_scale_one(scaling_raw[i], k_s);
        }
        return;
    }
    b -= grid.nb_s;
    const int64_t n = P, n4 = n / 4, stride = (int64_t)grid.nb_o * kMcmcBlock;
    for (int64_t i = (int64_t)b * kMcmcBlock + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4 *>(opacity_raw)[i];
        float4 g = reinterpret_cast<float4 *>(grad_opacity)[i];
        g.x += mcmc_reg_opacity_one(v.x, k_o); g.y += mcmc_reg_opacity_one(v.y, k_o);
        g.z += mcmc_reg_opacity_one(v.z, k_o); g.w += mcmc_reg_opacity_one(v.w, k_o);
        reinterpret_cast<float4 *>(grad_opacity)[i] = g;
    }
    if (b == 0 && (int64_t)threadIdx.x < n - n4 * 4) {
        const int64_t i = n4 * 4 + threadIdx.x;
        grad_opacity[i] += mcmc_reg_opacity_one(opacity_raw[i], k_o);
    }
}

}  // namespace gsr

using namespace gsr;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static unsigned blocks_for(int64_t n) { return (unsigned)((n + kMcmcBlock - 1) / kMcmcBlock); }
constexpr int64_t kMcmcMaxRows = (int64_t)1 << 31;        // rows a launch of one thread per row (or per four) addresses

extern "C" int gsr_mcmc_relocation_workspace_size(int64_t P, size_t *bytes)
{
    if (P < 0 || P > kMcmcMaxRows || !bytes) {
        set_error("gsr_mcmc_relocation_workspace_size: P = %lld (0 .. 2^31), bytes = %p", (long long)P, (void *)bytes);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    *bytes = align_up((size_t)P * sizeof(uint32_t));
    return GSR_OK;
}

extern "C" int gsr_mcmc_relocation(int64_t P, int64_t n, const float *opacity_raw, const float *scaling_raw, const int64_t *sampled,
                                   float min_opacity, void *workspace, float *new_opacity_raw, float *new_scaling_raw, void *stream)
{
    if (P < 0 || P > kMcmcMaxRows || n < 0 || n > kMcmcMaxRows) {
        set_error("gsr_mcmc_relocation: P = %lld, n = %lld (0 .. 2^31 each)", (long long)P, (long long)n);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!(min_opacity > 0.f && min_opacity < 1.f)) {
        set_error("gsr_mcmc_relocation: min_opacity = %g is outside (0, 1)", (double)min_opacity);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0 || n == 0) return GSR_OK;
    if (!opacity_raw || !scaling_raw || !sampled || !workspace || !new_opacity_raw || !new_scaling_raw) {
        set_error("gsr_mcmc_relocation: NULL pointer (opacity_raw, scaling_raw, sampled, workspace and both outputs are required)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t *counts = static_cast<uint32_t *>(workspace);
    ProfileScope prof("mcmc_relocation", s);
    hipLaunchKernelGGL(k_mcmc_count, dim3(blocks_for(n)), dim3(kMcmcBlock), 0, s, n, sampled, counts, 0);
    GSR_LAUNCH_CHECK("mcmc_count_clear", false, s);
    hipLaunchKernelGGL(k_mcmc_count, dim3(blocks_for(n)), dim3(kMcmcBlock), 0, s, n, sampled, counts, 1);
    GSR_LAUNCH_CHECK("mcmc_count", false, s);
    hipLaunchKernelGGL(k_mcmc_rule, dim3(blocks_for(n)), dim3(kMcmcBlock), 0, s, n, opacity_raw, scaling_raw, sampled, counts, min_opacity,
                       new_opacity_raw, new_scaling_raw);
    GSR_LAUNCH_CHECK("mcmc_rule", false, s);
    return GSR_OK;
}

extern "C" int gsr_mcmc_relocate_rows(int32_t count, const gsr_mcmc_tensor *tensors, int64_t P, int64_t n, const int64_t *sampled,
                                      const int64_t *dead, const float *new_opacity_raw, const float *new_scaling_raw, void *stream)
{
    if (count < 0 || count > GSR_MCMC_MAX_TENSORS || (count > 0 && !tensors)) {
        set_error("gsr_mcmc_relocate_rows: 0 .. %d tensors", GSR_MCMC_MAX_TENSORS);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P < 0 || P > kMcmcMaxRows || n < 0 || n > kMcmcMaxRows) {
        set_error("gsr_mcmc_relocate_rows: P = %lld, n = %lld (0 .. 2^31 each)", (long long)P, (long long)n);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    McmcRows a;
    a.count = count;
    uint32_t W = 0;
    for (int i = 0; i < count; ++i) {
        const gsr_mcmc_tensor &t = tensors[i];
        if (t.width < 1) {
            set_error("gsr_mcmc_relocate_rows: tensor %d: width = %d (width >= 1)", i, t.width);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (t.role != GSR_MCMC_ROLE_COPY && t.role != GSR_MCMC_ROLE_OPACITY && t.role != GSR_MCMC_ROLE_SCALING) {
            set_error("gsr_mcmc_relocate_rows: tensor %d: role = %d (GSR_MCMC_ROLE_COPY, _OPACITY or _SCALING)", i, t.role);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if ((t.role == GSR_MCMC_ROLE_OPACITY && t.width != 1) || (t.role == GSR_MCMC_ROLE_SCALING && t.width != 3)) {
            set_error("gsr_mcmc_relocate_rows: tensor %d: width = %d does not fit its role (opacity: 1, scaling: 3)", i, t.width);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if ((!t.exp_avg) != (!t.exp_avg_sq)) {
            set_error("gsr_mcmc_relocate_rows: tensor %d: exp_avg and exp_avg_sq are both given or both NULL", i);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (P > 0 && n > 0 && !t.param) {
            set_error("gsr_mcmc_relocate_rows: tensor %d: param is NULL", i);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if ((int64_t)W + t.width > (int64_t)1 << 20) {
            set_error("gsr_mcmc_relocate_rows: the widths sum to more than 2^20");
            return GSR_ERR_INVALID_ARGUMENT;
        }
        W += (uint32_t)t.width;
        a.p[i] = t.param; a.m[i] = t.exp_avg; a.v[i] = t.exp_avg_sq;
        a.width[i] = (uint32_t)t.width; a.col_end[i] = W; a.role[i] = t.role;
    }
    if (P == 0 || n == 0 || count == 0) return GSR_OK;
    if (!sampled || !new_opacity_raw || !new_scaling_raw) {
        set_error("gsr_mcmc_relocate_rows: NULL pointer (sampled and both new-value arrays are required)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    for (int i = count; i < GSR_MCMC_MAX_TENSORS; ++i) { a.p[i] = a.m[i] = a.v[i] = nullptr; a.width[i] = 1; a.col_end[i] = W; a.role[i] = GSR_MCMC_ROLE_COPY; }
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long total = (unsigned long long)n * W;
    const unsigned long long want = (total + kMcmcBlock - 1) / kMcmcBlock;
    ProfileScope prof("mcmc_rows", s);
    hipLaunchKernelGGL(k_mcmc_rows, dim3((unsigned)(want < 16384 ? want : 16384)), dim3(kMcmcBlock), 0, s, a, total, sampled, dead,
                       new_opacity_raw, new_scaling_raw);
    GSR_LAUNCH_CHECK("mcmc_rows", false, s);
    return GSR_OK;
}

extern "C" int gsr_mcmc_inject_noise(int64_t P, float *xyz, const float *scaling_raw, const float *rotation_raw, const float *opacity_raw,
                                     const float *noise, float c, void *stream)
{
    if (P < 0 || P > kMcmcMaxRows) {
        set_error("gsr_mcmc_inject_noise: P = %lld (0 .. 2^31)", (long long)P);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    if (!xyz || !scaling_raw || !rotation_raw || !opacity_raw || !noise) {
        set_error("gsr_mcmc_inject_noise: NULL pointer (xyz, scaling_raw, rotation_raw, opacity_raw and noise are required)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(xyz) || !aligned16(scaling_raw) || !aligned16(rotation_raw) || !aligned16(opacity_raw) || !aligned16(noise)) {
        set_error("gsr_mcmc_inject_noise: tensors must be 16-byte aligned");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    const int64_t threads = P / 4 > 0 ? P / 4 : 1;
    ProfileScope prof("mcmc_noise", s);
    hipLaunchKernelGGL(k_mcmc_noise, dim3(blocks_for(threads)), dim3(kMcmcBlock), 0, s, P, xyz, scaling_raw, rotation_raw, opacity_raw, noise, c);
    GSR_LAUNCH_CHECK("mcmc_noise", false, s);
    return GSR_OK;
}

extern "C" int gsr_mcmc_reg_grads(int64_t P, const float *opacity_raw, const float *scaling_raw, float lambda_opacity, float lambda_scale,
                                  float *grad_opacity, float *grad_scaling, void *stream)
{
    if (P < 0 || P > kMcmcMaxRows) {
        set_error("gsr_mcmc_reg_grads: P = %lld (0 .. 2^31)", (long long)P);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0 || (!grad_opacity && !grad_scaling)) return GSR_OK;
    if ((grad_opacity && !opacity_raw) || (grad_scaling && !scaling_raw)) {
        set_error("gsr_mcmc_reg_grads: a wanted gradient needs its raw tensor (opacity_raw / scaling_raw is NULL)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((grad_opacity && (!aligned16(opacity_raw) || !aligned16(grad_opacity))) || (grad_scaling && (!aligned16(scaling_raw) || !aligned16(grad_scaling)))) {
        set_error("gsr_mcmc_reg_grads: tensors must be 16-byte aligned");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    auto blocks = [](int64_t n4) { int64_t b = (n4 + kMcmcBlock - 1) / kMcmcBlock; return (unsigned)(b < 1 ? 1 : (b > 2048 ? 2048 : b)); };
    RegGrid g;
    g.nb_s = grad_scaling ? blocks((3 * P + 3) / 4) : 0u;
    g.nb_o = grad_opacity ? blocks((P + 3) / 4) : 0u;
    const float k_o = (float)((double)lambda_opacity / (double)P), k_s = (float)((double)lambda_scale / (3.0 * (double)P));
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("mcmc_reg", s);
    hipLaunchKernelGGL(k_mcmc_reg, dim3(g.nb_s + g.nb_o), dim3(kMcmcBlock), 0, s, P, g, opacity_raw, scaling_raw, k_o, k_s, grad_opacity, grad_scaling);
    GSR_LAUNCH_CHECK("mcmc_reg", false, s);
    return GSR_OK;
}
