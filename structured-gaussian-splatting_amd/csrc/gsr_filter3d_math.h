// gsr_filter3d_math.h — Mip-Splatting's 3D smoothing filter, per Gaussian, written once as GSR_HD inline
// functions: the kernels of gsr_filter3d.hip call them on the device, tests/filter3d_host.cpp compiles the same text with g++.
//
// Filter size: one camera is 16 floats, the 12 view entries the rule reads (the row-vector view matrix V, coordinate by coordinate:
// V00 V10 V20 V30, V01 V11 V21 V31, V02 V12 V22 V32) and then fx, fy, W, H.  filter3d_depth_step folds one camera into the running
// minimum depth of one Gaussian; min is exact, so the cameras' order does not matter.
//
// Application: s' = sqrt(s^2 + f^2) per axis, o' = o sqrt(prod s^2 / prod s'^2).  RAW = log-scales and logits in and out.  Every form
// below is a sum of terms of one sign or a product of factors in [0, 1]: the forward neither overflows nor cancels for finite inputs.
// (A gradient can: dl'/du_i = (1 - r_i) (1 + e^l) / (1 + e^l (1 - c)) is itself beyond binary32 for a logit over 88 beside a filter
// that barely registers.)
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/gsr_constants.h"

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

constexpr int kF3dCamFloats = 16;
constexpr float kF3dNear = (float)GSR_NEAR_CUT;
constexpr float kF3dHalfExtent = (float)(0.5 + GSR_F3D_MARGIN);     // -0.15 W <= u + W/2 <= 1.15 W  <=>  |u| <= 0.65 W
constexpr float kF3dUnseen = INFINITY;                               // d of a Gaussian no camera saw, until the fill

// d = min(d, z) when this camera sees p: z > 0.2 and the pixel within the image grown by 15 % on every side.  The screen test is
// multiplied through by z (> 0): |x fx| <= 0.65 W z.  Three fmaf per coordinate, in this order, on the device and on the host.
GSR_HD float filter3d_depth_step(const float p[3], const float *cam, float d)
{
    const float x = fmaf(p[0], cam[0], fmaf(p[1], cam[1], fmaf(p[2], cam[2], cam[3])));
    const float y = fmaf(p[0], cam[4], fmaf(p[1], cam[5], fmaf(p[2], cam[6], cam[7])));
    const float z = fmaf(p[0], cam[8], fmaf(p[1], cam[9], fmaf(p[2], cam[10], cam[11])));
    const float limx = (kF3dHalfExtent * cam[14]) * z, limy = (kF3dHalfExtent * cam[15]) * z;
    const bool valid = z > kF3dNear && fabsf(x * cam[12]) <= limx && fabsf(y * cam[13]) <= limy;
    return valid && z < d ? z : d;
}

// sqrt(GSR_F3D_VARIANCE) / F, the factor between a depth and its filter size
GSR_HD float filter3d_scale(float focal_max) { return sqrtf((float)GSR_F3D_VARIANCE) / focal_max; }

// The filter of one Gaussian from its minimum depth: `fill` (the maximum over the seen Gaussians) where no camera saw it
GSR_HD float filter3d_finish_one(float d, float fill, float scale) { return (d < kF3dUnseen ? d : fill) * scale; }

// One axis in the log domain: with w = f / s, g = -0.5 log1p(w^2) = log(s / s') <= 0 and r = s^2 / s'^2 = 1 / (1 + w^2).
// w comes from the inputs themselves (f exp(-u): no rounded log f in front of a difference); beyond e^40 the 1 under the log is
// below half an ulp of w^2 and g = -(log f - u).
constexpr float kF3dAxisSwitch = 40.f;            // log f - u beyond which 1 + w^2 is w^2 in binary32
constexpr float kF3dExpSwitch = -87.f;            // the log-scale under which exp(-u) is taken in two halves: alone it overflows at -88.7

struct F3dAxis { float g, r, one_minus_r, u_out; };              // u_out = u - g = log s'

GSR_HD F3dAxis filter3d_axis_raw(float u, float f, float lf)
{
    F3dAxis a;
    const float t = lf - u;
    if (t > kF3dAxisSwitch) { a.g = -t; a.r = expf(-2.f * t); a.one_minus_r = 1.f; a.u_out = lf; return a; }
    float w;
    if (u < kF3dExpSwitch) {                          // s is under binary32's normal range; t <= 40, so f E <= w <= e^40
        const float E = expf(-0.5f * u);              // (finite down to u = -177; under that, t <= 40 would need an f of zero)
        w = (f * E) * E;
    } else {
        w = f * expf(-u);
    }
    const float w2 = w * w;
    a.g = -0.5f * log1pf(w2);
    a.r = 1.f / (1.f + w2);
    a.one_minus_r = w2 / (1.f + w2);
    a.u_out = u - a.g;
    return a;
}

// One axis in the linear domain: rho = s / s' and s' = m sqrt(1 + (n / m)^2), m the larger of s and f
struct F3dAxisLin { float s_out, rho, r, one_minus_r; };

GSR_HD F3dAxisLin filter3d_axis_lin(float s, float f)
{
    F3dAxisLin a;
    const bool big = s >= f;
    const float m = big ? s : f, n = big ? f : s;
    const float q = n / m, root = sqrtf(1.f + q * q);
    a.s_out = m * root;
    a.rho = (big ? 1.f : q) / root;
    const float q2 = q * q, den = 1.f + q2;                          // r = s^2 / (s^2 + f^2)
    a.r = (big ? 1.f : q2) / den;
    a.one_minus_r = (big ? q2 : 1.f) / den;
    return a;
}

// logit(sigmoid(l) c) for log c = lc <= 0, and its two factors: dl = d l'/d l = (1 - p) / (1 - p'), a = 1 / (1 - p').
// qc = 1 - c = -expm1(lc).  l <= 0: l' = l + lc - log1p(e^l qc); l > 0, mirrored: l' = lc - log(e^-l + qc).
// qc == 0 (the filter is negligible on every axis): 1 / (1 - p') = 1 + e^l, held at FLT_MAX beyond l = 88.7 so that its product
// with a 1 - r_i of zero is zero and not a NaN.
struct F3dLogit { float l_out, dl, a; };

GSR_HD F3dLogit filter3d_logit(float l, float lc)
{
    F3dLogit o;
    const float qc = -expm1f(lc);
    if (qc == 0.f) { o.l_out = l; o.dl = 1.f; o.a = fminf(1.f + expf(l), 3.402823466e+38f); return o; }
    if (l <= 0.f) {
        const float e = expf(l), den = 1.f + e * qc;
        o.l_out = l + lc - log1pf(e * qc);
        o.dl = 1.f / den;
        o.a = (1.f + e) / den;
    } else {
        const float e = expf(-l), den = e + qc;
        o.l_out = lc - logf(den);
        // beyond l = 87 e^-l is subnormal, a few bits wide: nothing to den, but dl is e / den.  e^(40 - l) e^-40 keeps its digits
        // (40 - l is exact there)
        o.dl = l > 80.f ? expf(40.f - l) / den * 4.2483543e-18f : e / den;
        o.a = (e + 1.f) / den;
    }
    return o;
}

// Forward of one Gaussian.  sc[3], op: log-scales and the logit (RAW) or scales and the opacity.  f <= 0 (no filter): the row passes
// through bit for bit.
template <bool RAW>
GSR_HD void filter3d_apply_one(const float sc[3], float op, float f, float sc_out[3], float &op_out)
{
    if (!(f > 0.f)) {
        sc_out[0] = sc[0]; sc_out[1] = sc[1]; sc_out[2] = sc[2]; op_out = op;
        return;
    }
    if (RAW) {
        const float lf = logf(f);
        float lc = 0.f;
        for (int k = 0; k < 3; ++k) {
            const F3dAxis a = filter3d_axis_raw(sc[k], f, lf);
            sc_out[k] = a.u_out;
            lc += a.g;
        }
        op_out = filter3d_logit(op, lc).l_out;
    } else {
        float coef = 1.f;
        for (int k = 0; k < 3; ++k) {
            const F3dAxisLin a = filter3d_axis_lin(sc[k], f);
            sc_out[k] = a.s_out;
            coef *= a.rho;
        }
        op_out = op * coef;
    }
}

// Backward of one Gaussian, recomputed from the inputs: gsc[3], gop are dL/d(sc_out), dL/d(op_out); dsc[3], dop the gradients on
// the inputs.  No gradient goes to f.
template <bool RAW>
GSR_HD void filter3d_apply_backward_one(const float sc[3], float op, float f, const float gsc[3], float gop, float dsc[3], float &dop)
{
    if (!(f > 0.f)) {
        dsc[0] = gsc[0]; dsc[1] = gsc[1]; dsc[2] = gsc[2]; dop = gop;
        return;
    }
    if (RAW) {
        const float lf = logf(f);
        F3dAxis a[3];
        float lc = 0.f;
        for (int k = 0; k < 3; ++k) { a[k] = filter3d_axis_raw(sc[k], f, lf); lc += a[k].g; }
        const F3dLogit o = filter3d_logit(op, lc);
        dop = gop * o.dl;
        const float ga = gop * o.a;
        for (int k = 0; k < 3; ++k) dsc[k] = gsc[k] * a[k].r + ga * a[k].one_minus_r;
    } else {
        F3dAxisLin a[3];
        for (int k = 0; k < 3; ++k) a[k] = filter3d_axis_lin(sc[k], f);
        dop = gop * (a[0].rho * a[1].rho * a[2].rho);
        const float go = gop * op;
        // d coef / d s_k = (prod of the other rho) (1 - r_k) / s'_k: no division by s_k
        dsc[0] = gsc[0] * a[0].rho + go * (a[1].rho * a[2].rho) * a[0].one_minus_r / a[0].s_out;
        dsc[1] = gsc[1] * a[1].rho + go * (a[0].rho * a[2].rho) * a[1].one_minus_r / a[1].s_out;
        dsc[2] = gsc[2] * a[2].rho + go * (a[0].rho * a[1].rho) * a[2].one_minus_r / a[2].s_out;
    }
}

}  // namespace gsr
