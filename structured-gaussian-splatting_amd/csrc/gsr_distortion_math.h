// gsr_distortion_math.h — the depth-distortion loss, per element, written once as GSR_HD inline functions: the
// kernels of gsr_distortion.hip call them on the device, tests/distortion_host.cpp compiles the same text with g++.
//
// Per pixel, over the splats the colour composites, w_i = alpha_i T_i and a per-splat depth value m_i (Mip-NeRF 360's distortion
// term in the squared form 2DGS uses):
//     D = sum_{i<j} w_i w_j (m_i - m_j)^2 = A M2 - M1^2,   A = sum w_i,  M1 = sum w_i m_i,  M2 = sum w_i m_i^2
// A is the alpha map; M1 and M2 are two linear channels, blended as extra colours (m, m^2, 0) of the colour frame.
//
// Per Gaussian: z = the view depth of the mean (row-vector convention, z = x V02 + y V12 + z V22 + V32, three fmaf as the other
// per-Gaussian ops of this library take it), and
//     ndc     m = far (z - near) / ((far - near) z)       in [0, 1) for z in (near, inf): the depth of the projection matrix,
//                                                         d m / d z = far near / ((far - near) z^2)
//     linear  m = z,                                      d m / d z = 1
// Where z <= near (ndc) or z <= 0 (linear) m = +0.0 and the gradient is +0.0 (the frame culls such a Gaussian anyway).
//
// Every product-sum below is written out: one fmaf in dst_pixel, three in dst_view_depth, and no other multiply stands beside an
// add that a compiler could contract with it except in dst_moments_backward_one's g0 + 2 m g1, which the file is compiled
// without contraction for (csrc/Makefile).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#ifndef GSR_HD
#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD static inline
#endif
#endif

namespace gsr {

constexpr int kDstMappingNdc = 0, kDstMappingLinear = 1;       // GSR_DISTORTION_NDC, GSR_DISTORTION_LINEAR of include/gsrast_distortion.h

// ---- per Gaussian ---------------------------------------------------------------------------------------------------------------

struct DstMapping { int kind; float near, far, span, far_near; };      // span = far - near, far_near = far * near

GSR_HD DstMapping dst_mapping(int kind, float near, float far)
{
    DstMapping d;
    d.kind = kind; d.near = near; d.far = far;
    d.span = far - near; d.far_near = far * near;
    return d;
}

// V: the view matrix [4,4] row-major (column 2 is read)
GSR_HD float dst_view_depth(const float p[3], const float *V) { return fmaf(p[0], V[2], fmaf(p[1], V[6], fmaf(p[2], V[10], V[14]))); }

GSR_HD bool dst_in_front(const DstMapping &d, float z) { return d.kind == kDstMappingNdc ? z > d.near : z > 0.f; }

// m of one Gaussian; the denominator of the ndc form is returned for the backward
GSR_HD float dst_depth_value(const DstMapping &d, float z, float &den)
{
    den = 1.f;
    if (!dst_in_front(d, z)) return 0.f;
    if (d.kind != kDstMappingNdc) return z;
    den = d.span * z;
    return (d.far * (z - d.near)) / den;
}

GSR_HD void dst_moments_one(const DstMapping &d, const float mean[3], const float *V, float out[3])
{
    float den;
    const float m = dst_depth_value(d, dst_view_depth(mean, V), den);
    out[0] = m; out[1] = m * m; out[2] = 0.f;
}

// dL/dmean from g = dL/d(m, m^2, .): gz = (g0 + 2 m g1) dm/dz, then the view depth's three coefficients
GSR_HD void dst_moments_backward_one(const DstMapping &d, const float mean[3], const float *V, const float g[3], float dmean[3])
{
    const float z = dst_view_depth(mean, V);
    float den;
    const float m = dst_depth_value(d, z, den);
    if (!dst_in_front(d, z)) { dmean[0] = 0.f; dmean[1] = 0.f; dmean[2] = 0.f; return; }
    float gz = g[0] + (2.f * m) * g[1];
    if (d.kind == kDstMappingNdc) gz = gz * (d.far_near / (den * z));
    dmean[0] = gz * V[2]; dmean[1] = gz * V[6]; dmean[2] = gz * V[10];
}

// ---- per pixel ------------------------------------------------------------------------------------------------------------------

// D = A M2 - M1^2: the square rounded, then one fused multiply-add; not clamped
GSR_HD float dst_pixel(float A, float M1, float M2) { return fmaf(A, M2, -(M1 * M1)); }

// from g = dL/dD: dA = g M2, dM1 = -2 g M1, dM2 = g A
GSR_HD void dst_pixel_backward(float g, float A, float M1, float M2, float &dA, float &dM1, float &dM2)
{
    dA = g * M2;
    dM1 = 0.f - 2.f * (g * M1);               // (0 - x: a zero gradient is +0.0)
    dM2 = g * A;
}

// the loss is mean(D): every pixel's g is grad_loss / N, with 1 / N rounded to binary32 from binary64 first
GSR_HD float dst_loss_scale(float grad_loss, int64_t n) { return grad_loss * (float)(1.0 / (double)n); }

}  // namespace gsr
