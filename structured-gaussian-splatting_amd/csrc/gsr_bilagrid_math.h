// gsr_bilagrid_math.h — the bilateral grid's per-pixel rule, written once as GSR_HD inline functions: the
// kernels of gsr_bilagrid.hip load, call and store; tests/bilagrid_host.cpp compiles the same functions with g++.
//
// A grid is [12, L, Gy, Gx] floats: 12 coefficients of a 3x4 affine colour transform at every node (z = luma, y, x).  A pixel
// reads the 8 nodes around (fx, fy, fz), trilinearly, and applies the interpolated transform to (r, g, b, 1).  The rule is torch's
// grid_sample(mode="bilinear", padding_mode="border", align_corners=True) on a 5-D input followed by the affine product.
#pragma once

#include <math.h>
#include <stdint.h>

#ifndef GSR_HD
#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD static inline
#endif
#endif

#if defined(__HIPCC__)
#define GSR_HD_MEMBER __host__ __device__ __forceinline__
#else
#define GSR_HD_MEMBER inline
#endif

namespace gsr {

struct BilaDims { int L, Gy, Gx, H, W; };

// One axis of a tap: the two nodes and the weight t of the upper one (the lower one weighs 1 - t).  Both indices are inside
// [0, G - 1] whatever f is (a NaN lands on node 0): the out-of-range corner is this op's characteristic bug.
struct BilaAxis { int i0, i1; float t; };

GSR_HD BilaAxis bila_axis(float f, int G)
{
    BilaAxis a;
    if (G <= 1) { a.i0 = a.i1 = 0; a.t = 0.f; return a; }
    const float fl = fminf(fmaxf(floorf(f), 0.f), (float)(G - 1));      // clamped as a float: the cast below is always defined
    a.i0 = (int)fl;
    a.i1 = a.i0 + 1 < G ? a.i0 + 1 : G - 1;
    a.t = f - fl;
    return a;
}

// the weight of node n on that axis: (1 - t | t), both where the two nodes coincide (t is 0 there)
GSR_HD float bila_axis_weight(const BilaAxis &a, int n) { return (n == a.i0 ? 1.f - a.t : 0.f) + (n == a.i1 ? a.t : 0.f); }

GSR_HD float bila_coord(int p, int n, int G) { return ((float)p + 0.5f) / (float)n * (float)(G - 1); }
GSR_HD float bila_gray(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

struct BilaTap { BilaAxis x, y, z; float gray; };

GSR_HD BilaTap bila_tap(const BilaDims &d, int py, int px, float r, float g, float b)
{
    BilaTap t;
    t.x = bila_axis(bila_coord(px, d.W, d.Gx), d.Gx);
    t.y = bila_axis(bila_coord(py, d.H, d.Gy), d.Gy);
    t.gray = bila_gray(r, g, b);
    t.z = bila_axis(fminf(fmaxf(t.gray, 0.f), 1.f) * (float)(d.L - 1), d.L);
    return t;
}

// The grid nodes the pixels [p_first, p_last] of one axis read: coordinates grow with the pixel, so these are the lower node of
// the first and the upper node of the last.
GSR_HD void bila_span(int p_first, int p_last, int n, int G, int &lo, int &hi)
{
    lo = bila_axis(bila_coord(p_first, n, G), G).i0;
    hi = bila_axis(bila_coord(p_last, n, G), G).i1;
}

// Where the coefficients of a tap are read from: the grid as it lies in memory, [12, L, Gy, Gx] ...
struct BilaGridView {
    const float *g; int L, Gy, Gx;
    GSR_HD_MEMBER float at(int k, int z, int y, int x) const { return g[(((size_t)k * L + z) * Gy + y) * Gx + x]; }
};
// ... or a copy of the nodes [ylo, ylo + ny) x [xlo, xlo + nx) laid out [ny, nx, L, 12], the 12 coefficients of a node side by side
// (the kernels stage a tile's footprint in LDS this way)
struct BilaTileView {
    const float *s; int L, xlo, ylo, nx;
    GSR_HD_MEMBER float at(int k, int z, int y, int x) const { return s[(((y - ylo) * nx + (x - xlo)) * L + z) * 12 + k]; }
};

// xy-bilinear interpolation of all 12 coefficients at the tap's two luma levels
template <class View>
GSR_HD void bila_levels(const View &v, const BilaTap &t, float lo[12], float hi[12])
{
    const float w[4] = {(1.f - t.y.t) * (1.f - t.x.t), (1.f - t.y.t) * t.x.t, t.y.t * (1.f - t.x.t), t.y.t * t.x.t};
    const int ys[4] = {t.y.i0, t.y.i0, t.y.i1, t.y.i1}, xs[4] = {t.x.i0, t.x.i1, t.x.i0, t.x.i1};
#pragma unroll
    for (int k = 0; k < 12; ++k) lo[k] = hi[k] = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c)
#pragma unroll
        for (int k = 0; k < 12; ++k) {
            lo[k] += w[c] * v.at(k, t.z.i0, ys[c], xs[c]);
            hi[k] += w[c] * v.at(k, t.z.i1, ys[c], xs[c]);
        }
}

// out_c = A[4c] r + A[4c+1] g + A[4c+2] b + A[4c+3],  A_k = (1 - tz) lo_k + tz hi_k
template <class View>
GSR_HD void bila_forward_one(const View &v, const BilaTap &t, const float in[3], float out[3])
{
    float lo[12], hi[12];
    bila_levels(v, t, lo, hi);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float A[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) A[j] = (1.f - t.z.t) * lo[4 * c + j] + t.z.t * hi[4 * c + j];
        out[c] = A[0] * in[0] + A[1] * in[1] + A[2] * in[2] + A[3];
    }
}

// dimage_j = sum_c A[4c+j] go_c + gw_j (L - 1) [0 < gray < 1] sum_k (hi_k - lo_k) go_c in_j
template <class View>
GSR_HD void bila_backward_image_one(int L, const View &v, const BilaTap &t, const float in[3], const float go[3], float dimage[3])
{
    const float in4[4] = {in[0], in[1], in[2], 1.f};
    float lo[12], hi[12], s = 0.f;
    bila_levels(v, t, lo, hi);
    dimage[0] = dimage[1] = dimage[2] = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = 4 * c + j;
            if (j < 3) dimage[j] += ((1.f - t.z.t) * lo[k] + t.z.t * hi[k]) * go[c];
            s += (hi[k] - lo[k]) * (go[c] * in4[j]);
        }
    if (t.gray > 0.f && t.gray < 1.f) {
        s *= (float)(L - 1);
        dimage[0] += 0.299f * s; dimage[1] += 0.587f * s; dimage[2] += 0.114f * s;
    }
}

// d tv / d grids[e] for unit upstream: the three-axis stencil around element e = (.., z, y, x) with value v; kx, ky, kz = 2 / (the
// number of differences along the axis), 0 for an axis of size 1
GSR_HD float bila_tv_backward_one(const float *g, int64_t e, int z, int y, int x, int L, int Gy, int Gx, float kx, float ky, float kz)
{
    const float v = g[e];
    float r = 0.f;
    if (x > 0) r += kx * (v - g[e - 1]);
    if (x + 1 < Gx) r -= kx * (g[e + 1] - v);
    if (y > 0) r += ky * (v - g[e - Gx]);
    if (y + 1 < Gy) r -= ky * (g[e + Gx] - v);
    if (z > 0) r += kz * (v - g[e - (int64_t)Gy * Gx]);
    if (z + 1 < L) r -= kz * (g[e + (int64_t)Gy * Gx] - v);
    return r;
}

}  // namespace gsr
