// gsr_antialias.hip — anti-aliasing as an opacity compensation in front of the unchanged rasterizer (include/gsrast.h
// gsr_opacity_compensation_*; the rule is written once in gsr_math.h opacity_compensation_one / _backward_one).
// The rasterizer low-passes every splat by GSR_COV2D_DILATE on the diagonal of its 2D covariance and keeps that covariance for the
// radius, the binning rectangle and the conic; these two kernels scale the opacity by rho = sqrt(det cov2D / det(cov2D + dilation))
// and take rho's gradient back to means3D, scales and rotations.  One thread per Gaussian, every row from its own inputs only: no
// atomics, no cross-lane sums, the same inputs give the same bits.
//
// HBM traffic per Gaussian: the forward reads 44 B (mean 12, scale 12, quaternion 16, opacity 4) and writes 4; the backward reads
// 48 (those and the incoming gradient) and writes up to 44.  A row whose incoming gradient is exactly zero (most rows of a frame
// were never binned) reads 4 B and writes zeros.  The view matrix is a wave-uniform load.
#include "gsr_internal.h"

namespace gsr {

constexpr int kAaBlock = 256;

// One Gaussian's geometry and opacity in registers, activated (the idiom of gsr_geom.hip load_gaussian, without SH or a
// precomputed covariance).  RAW: the tensors are log-scales, raw quaternions and logits; in.act keeps what activate_raw made of them.
struct AaIn {
    float p[3], sc[3], q[4], opacity, logit;
    RawAct act;
};

template <bool RAW>
__device__ __forceinline__ void load_aa(int i, const float *__restrict__ means, const float *__restrict__ scales,
                                        const float *__restrict__ rots, const float *__restrict__ opac, AaIn &in)
{
    in.p[0] = means[3 * (size_t)i]; in.p[1] = means[3 * (size_t)i + 1]; in.p[2] = means[3 * (size_t)i + 2];
    in.sc[0] = scales[3 * (size_t)i]; in.sc[1] = scales[3 * (size_t)i + 1]; in.sc[2] = scales[3 * (size_t)i + 2];
    const float4 qq = reinterpret_cast<const float4 *>(rots)[i];
    in.q[0] = qq.x; in.q[1] = qq.y; in.q[2] = qq.z; in.q[3] = qq.w;
    in.opacity = in.logit = opac[i];
    if constexpr (RAW) {
        activate_raw(in.sc, in.q, in.logit, in.act);
#pragma unroll
        for (int k = 0; k < 3; ++k) in.sc[k] = in.act.scale[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) in.q[k] = in.act.q[k];
        in.opacity = in.act.opacity;
    }
}

template <bool RAW>
__global__ __launch_bounds__(kAaBlock) void k_aa_fwd(FrameK f, const float *__restrict__ view, const float *__restrict__ means,
                                                     const float *__restrict__ scales, const float *__restrict__ rots,
                                                     const float *__restrict__ opac, float *__restrict__ out)
{
    const int i = blockIdx.x * kAaBlock + threadIdx.x;
    if (i >= f.P) return;
    float V[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = view[k];
    AaIn in;
    load_aa<RAW>(i, means, scales, rots, opac, in);
    out[i] = opacity_compensation_one(f, V, in.p, in.sc, in.q, in.opacity, RAW ? &in.logit : nullptr);
}

template <bool RAW>
__global__ __launch_bounds__(kAaBlock) void k_aa_bwd(FrameK f, const float *__restrict__ view, const float *__restrict__ means,
                                                     const float *__restrict__ scales, const float *__restrict__ rots,
                                                     const float *__restrict__ opac, const float *__restrict__ gout,
                                                     float *__restrict__ dmeans, float *__restrict__ dopac,
                                                     float *__restrict__ dscales, float *__restrict__ drots)
{
    const int i = blockIdx.x * kAaBlock + threadIdx.x;
    if (i >= f.P) return;
    const float gin = gout[i];
    GeomGrad g;
#pragma unroll
    for (int k = 0; k < 3; ++k) { g.dmean[k] = 0.f; g.dscale[k] = 0.f; }
#pragma unroll
    for (int k = 0; k < 4; ++k) g.drot[k] = 0.f;
    g.dopacity = 0.f;
    if (gin != 0.f) {                          // (a NaN gradient runs the chain and spreads, as it would through torch ops)
        float V[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) V[k] = view[k];
        AaIn in;
        load_aa<RAW>(i, means, scales, rots, opac, in);
        opacity_compensation_backward_one(f, V, in.p, in.sc, in.q, in.opacity, RAW ? &in.act : nullptr, gin, g);
    }
    if (dopac) dopac[i] = g.dopacity;
    if (dmeans) { dmeans[3 * (size_t)i] = g.dmean[0]; dmeans[3 * (size_t)i + 1] = g.dmean[1]; dmeans[3 * (size_t)i + 2] = g.dmean[2]; }
    if (dscales) { dscales[3 * (size_t)i] = g.dscale[0]; dscales[3 * (size_t)i + 1] = g.dscale[1]; dscales[3 * (size_t)i + 2] = g.dscale[2]; }
    if (drots) reinterpret_cast<float4 *>(drots)[i] = make_float4(g.drot[0], g.drot[1], g.drot[2], g.drot[3]);
}

}  // namespace gsr

using namespace gsr;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Only what these two kernels read is asked for: P, the image size and field of view (the focal lengths), scale_modifier, the view
// matrix and the four per-Gaussian tensors.  SH, colours, bg, projmatrix and campos are ignored.
static int validate_aa(const char *who, const gsr_frame_desc *d, const gsr_camera *cam, const gsr_gaussians *g)
{
    if (!d || !cam || !g) { set_error("%s: desc, camera and gaussians are required", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->P < 0 || d->P >= (1 << kQuadMaskShift) || d->width <= 0 || d->height <= 0 || !(d->tanfovx > 0.f) || !(d->tanfovy > 0.f)) {
        set_error("%s: bad frame: P=%d (0 .. 2^%d - 1) width=%d height=%d tanfov=(%g, %g)", who, d->P, kQuadMaskShift, d->width, d->height,
                  (double)d->tanfovx, (double)d->tanfovy);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (g->cov3D_precomp) {
        set_error("%s: cov3D_precomp is not supported: the compensation's gradient goes to scales and rotations", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (g->raw < 0 || g->raw > 2) { set_error("%s: raw must be 0, 1 or 2", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->P == 0) return GSR_OK;
    if (!cam->viewmatrix) { set_error("%s: viewmatrix missing", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!g->means3D || !g->opacities || !g->scales || !g->rotations) {
        set_error("%s: means3D, opacities, scales and rotations are required", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(g->rotations)) { set_error("%s: rotations must be 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

extern "C" int gsr_opacity_compensation_forward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                                                float *opacities_out, void *stream)
{
    const char *who = "gsr_opacity_compensation_forward";
    if (int rc = validate_aa(who, desc, cam, g)) return rc;
    if (desc->P == 0) return GSR_OK;
    if (!opacities_out) { set_error("%s: opacities_out is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    const FrameK f = make_frame(*desc);
    const dim3 blocks((f.P + kAaBlock - 1) / kAaBlock), threads(kAaBlock);
    ProfileScope prof("aa_fwd", s);
    if (g->raw) hipLaunchKernelGGL(k_aa_fwd<true>, blocks, threads, 0, s, f, cam->viewmatrix, g->means3D, g->scales, g->rotations, g->opacities, opacities_out);
    else hipLaunchKernelGGL(k_aa_fwd<false>, blocks, threads, 0, s, f, cam->viewmatrix, g->means3D, g->scales, g->rotations, g->opacities, opacities_out);
    GSR_LAUNCH_CHECK("aa_fwd", desc->debug != 0, s);
    return GSR_OK;
}

extern "C" int gsr_opacity_compensation_backward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g,
                                                 const float *grad_opacities_out, const gsr_grads *grads, void *stream)
{
    const char *who = "gsr_opacity_compensation_backward";
    if (int rc = validate_aa(who, desc, cam, g)) return rc;
    if (!grads) { set_error("%s: grads is NULL (its fields may be)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->P == 0) return GSR_OK;
    if (!grad_opacities_out) { set_error("%s: grad_opacities_out is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!aligned16(grads->rotations)) { set_error("%s: grads->rotations must be 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!grads->means3D && !grads->opacities && !grads->scales && !grads->rotations) return GSR_OK;      // nothing wanted
    hipStream_t s = (hipStream_t)stream;
    const FrameK f = make_frame(*desc);
    const dim3 blocks((f.P + kAaBlock - 1) / kAaBlock), threads(kAaBlock);
    ProfileScope prof("aa_bwd", s);
    if (g->raw) hipLaunchKernelGGL(k_aa_bwd<true>, blocks, threads, 0, s, f, cam->viewmatrix, g->means3D, g->scales, g->rotations, g->opacities, grad_opacities_out, grads->means3D, grads->opacities, grads->scales, grads->rotations);
    else hipLaunchKernelGGL(k_aa_bwd<false>, blocks, threads, 0, s, f, cam->viewmatrix, g->means3D, g->scales, g->rotations, g->opacities, grad_opacities_out, grads->means3D, grads->opacities, grads->scales, grads->rotations);
    GSR_LAUNCH_CHECK("aa_bwd", desc->debug != 0, s);
    return GSR_OK;
}
