// gsr_normals_math.h — normal maps, per element, written once as GSR_HD inline functions: the kernels of
// gsr_normals.hip call them on the device, tests/normals_host.cpp compiles the same text with g++.
//
// Per Gaussian: the shortest axis of the ellipsoid, column k = argmin scales of R(q / |q|), turned to the camera and rotated into
// the view space (row-vector convention: n_view = n_world V[:3,:3]).
//
// Per pixel: with the view depths z of the four axis neighbours, Dx = z(x+1) - z(x-1), Sx = z(x+1) + z(x-1), Dy, Sy likewise,
//     m = (fx Sy Dx, fy Sx Dy, -(Sx Sy + px Sy Dx + py Sx Dy)),   n = m / |m|
// which is normalize(dP/dy x dP/dx) of the back-projected points P = (px z / fx, py z / fy, z) with every product pair that the
// cross product subtracts already cancelled on paper.  z > 0 at a valid pixel, so Sx Sy > 0 and |m| > 0.
//
// Where a pixel's view depth is read, an accessor `zat(x, y, z)` answers whether (x, y) is a valid pixel and, if so, its z; it is
// never asked about a pixel outside the image.  The kernels answer from a staged tile, the host program from the whole arrays.
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

// ---- per Gaussian ---------------------------------------------------------------------------------------------------------------

// argmin with ties to the lowest index (NaN never wins)
GSR_HD int nrm_shortest_axis(const float s[3])
{
    int k = 0;
    if (s[1] < s[k]) k = 1;
    if (s[2] < s[k]) k = 2;
    return k;
}

// column k of upstream's build_rotation for the unit quaternion u = (r, x, y, z)
GSR_HD void nrm_rotation_column(const float u[4], int k, float c[3])
{
    const float r = u[0], x = u[1], y = u[2], z = u[3];
    if (k == 0) { c[0] = 1.f - 2.f * (y * y + z * z); c[1] = 2.f * (x * y + r * z); c[2] = 2.f * (x * z - r * y); }
    else if (k == 1) { c[0] = 2.f * (x * y - r * z); c[1] = 1.f - 2.f * (x * x + z * z); c[2] = 2.f * (y * z + r * x); }
    else { c[0] = 2.f * (x * z + r * y); c[1] = 2.f * (y * z - r * x); c[2] = 1.f - 2.f * (x * x + y * y); }
}

// gu = (d column k / d u)^T gc
GSR_HD void nrm_rotation_column_backward(const float u[4], int k, const float gc[3], float gu[4])
{
    const float r = u[0], x = u[1], y = u[2], z = u[3];
    if (k == 0) {
        gu[0] = 2.f * (z * gc[1] - y * gc[2]);
        gu[1] = 2.f * (y * gc[1] + z * gc[2]);
        gu[2] = 2.f * (x * gc[1] - r * gc[2]) - 4.f * y * gc[0];
        gu[3] = 2.f * (r * gc[1] + x * gc[2]) - 4.f * z * gc[0];
    } else if (k == 1) {
        gu[0] = 2.f * (x * gc[2] - z * gc[0]);
        gu[1] = 2.f * (y * gc[0] + r * gc[2]) - 4.f * x * gc[1];
        gu[2] = 2.f * (x * gc[0] + z * gc[2]);
        gu[3] = 2.f * (y * gc[2] - r * gc[0]) - 4.f * z * gc[1];
    } else {
        gu[0] = 2.f * (y * gc[0] - x * gc[1]);
        gu[1] = 2.f * (z * gc[0] - r * gc[1]) - 4.f * x * gc[2];
        gu[2] = 2.f * (r * gc[0] + z * gc[1]) - 4.f * y * gc[2];
        gu[3] = 2.f * (x * gc[0] + y * gc[1]);
    }
}

struct NrmGaussian { float u[4], inv_len, nw[3], sign; int k; };      // nw: the world normal, already turned to the camera (by sign)

// V: the view matrix [4,4] row-major (rows 0..2 are read); cam: the camera centre
GSR_HD NrmGaussian nrm_gaussian(const float s[3], const float q[4], const float mean[3], const float *cam)
{
    NrmGaussian g;
    g.k = nrm_shortest_axis(s);
    g.inv_len = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (int i = 0; i < 4; ++i) g.u[i] = q[i] * g.inv_len;
    nrm_rotation_column(g.u, g.k, g.nw);
    const float dot = g.nw[0] * (mean[0] - cam[0]) + g.nw[1] * (mean[1] - cam[1]) + g.nw[2] * (mean[2] - cam[2]);
    g.sign = dot > 0.f ? -1.f : 1.f;                                                    // (exactly 0 does not flip)
    for (int i = 0; i < 3; ++i) g.nw[i] *= g.sign;
    return g;
}

GSR_HD void nrm_gaussian_forward_one(const float s[3], const float q[4], const float mean[3], const float *V, const float *cam, float out[3])
{
    const NrmGaussian g = nrm_gaussian(s, q, mean, cam);
    for (int j = 0; j < 3; ++j) out[j] = g.nw[0] * V[j] + g.nw[1] * V[4 + j] + g.nw[2] * V[8 + j];
}

// dq from dL/d(out): k and the sign recomputed from the inputs
GSR_HD void nrm_gaussian_backward_one(const float s[3], const float q[4], const float mean[3], const float *V, const float *cam,
                                      const float gout[3], float dq[4])
{
    const NrmGaussian g = nrm_gaussian(s, q, mean, cam);
    float gc[3], gu[4];
    for (int i = 0; i < 3; ++i) gc[i] = g.sign * (gout[0] * V[4 * i] + gout[1] * V[4 * i + 1] + gout[2] * V[4 * i + 2]);
    nrm_rotation_column_backward(g.u, g.k, gc, gu);
    const float dot = g.u[0] * gu[0] + g.u[1] * gu[1] + g.u[2] * gu[2] + g.u[3] * gu[3];
    for (int i = 0; i < 4; ++i) dq[i] = (gu[i] - g.u[i] * dot) * g.inv_len;
}

// ---- per pixel ------------------------------------------------------------------------------------------------------------------

struct NrmDims { int H, W; float fx, fy, alpha_min; };

GSR_HD NrmDims nrm_dims(int H, int W, float tanfovx, float tanfovy, float alpha_min)
{
    NrmDims d;
    d.H = H; d.W = W;
    d.fx = (float)W / (2.f * tanfovx); d.fy = (float)H / (2.f * tanfovy);
    d.alpha_min = alpha_min;
    return d;
}

GSR_HD bool nrm_valid(const NrmDims &d, float depth, float alpha) { return alpha >= d.alpha_min && depth > 0.f; }
GSR_HD float nrm_px(const NrmDims &d, int x) { return ((float)x + 0.5f) - 0.5f * (float)d.W; }      // exact for W < 2^23
GSR_HD float nrm_py(const NrmDims &d, int y) { return ((float)y + 0.5f) - 0.5f * (float)d.H; }
GSR_HD bool nrm_interior(const NrmDims &d, int x, int y) { return x >= 1 && y >= 1 && x <= d.W - 2 && y <= d.H - 2; }

struct NrmStencil { float Dx, Sx, Dy, Sy; };

// the stencil of the normal at (x, y): false when the pixel is on the border or a neighbour is not valid
template <class ZAt>
GSR_HD bool nrm_stencil(const NrmDims &d, int x, int y, const ZAt &zat, NrmStencil &s)
{
    if (!nrm_interior(d, x, y)) return false;
    float zl, zr, zu, zd;
    if (!zat(x - 1, y, zl) || !zat(x + 1, y, zr) || !zat(x, y - 1, zu) || !zat(x, y + 1, zd)) return false;
    s.Dx = zr - zl; s.Sx = zr + zl; s.Dy = zd - zu; s.Sy = zd + zu;
    return true;
}

// n = m / |m| and 1 / |m|
GSR_HD float nrm_normal_one(const NrmDims &d, float px, float py, const NrmStencil &s, float n[3])
{
    const float a = s.Sy * s.Dx, b = s.Sx * s.Dy;
    const float m0 = d.fx * a, m1 = d.fy * b, m2 = -(s.Sx * s.Sy + px * a + py * b);
    const float inv = 1.f / sqrtf(m0 * m0 + m1 * m1 + m2 * m2);
    n[0] = m0 * inv; n[1] = m1 * inv; n[2] = m2 * inv;
    return inv;
}

// What the normal of one pixel takes from its neighbours' depths: gz = dL/dz of (left, right, up, down) from g = dL/dn
GSR_HD void nrm_normal_backward_one(const NrmDims &d, float px, float py, const NrmStencil &s, const float n[3], float inv, const float g[3],
                                    float gz[4])
{
    const float dot = n[0] * g[0] + n[1] * g[1] + n[2] * g[2];
    const float gm0 = (g[0] - n[0] * dot) * inv, gm1 = (g[1] - n[1] * dot) * inv, gm2 = (g[2] - n[2] * dot) * inv;
    const float gDx = s.Sy * (gm0 * d.fx - gm2 * px), gDy = s.Sx * (gm1 * d.fy - gm2 * py);
    const float gSx = gm1 * d.fy * s.Dy - gm2 * (s.Sy + py * s.Dy), gSy = gm0 * d.fx * s.Dx - gm2 * (s.Sx + px * s.Dx);
    gz[0] = gSx - gDx; gz[1] = gSx + gDx; gz[2] = gSy - gDy; gz[3] = gSy + gDy;
}

// The term of the consistency loss at one pixel, 1 - alpha <N, n>; has_n: the pixel has a depth normal
GSR_HD float nrm_loss_term(bool has_n, float alpha, const float N[3], const float n[3])
{
    return has_n ? 1.f - alpha * (N[0] * n[0] + N[1] * n[1] + N[2] * n[2]) : 1.f;
}

// dL/dz of one pixel from what its four neighbours' normals take from it, in the order left, right, up, down: the left neighbour
// takes it as its right depth, and so on.  take(x, y, slot): gz[slot] of the normal at (x, y), 0 where that pixel has none; only
// asked about pixels inside the image.
template <class Take>
GSR_HD float nrm_gather(const NrmDims &d, int x, int y, const Take &take)
{
    float s = 0.f;
    if (x >= 1) s += take(x - 1, y, 1);
    if (x <= d.W - 2) s += take(x + 1, y, 0);
    if (y >= 1) s += take(x, y - 1, 3);
    if (y <= d.H - 2) s += take(x, y + 1, 2);
    return s;
}

// z = depth / alpha: d z / d depth = 1 / alpha, d z / d alpha = -z / alpha
GSR_HD void nrm_chain(float gz, float z, float alpha, float &gdepth, float &galpha)
{
    gdepth = gz / alpha;
    galpha = 0.f - (gz * z) / alpha;          // (0 - x: a zero gradient is +0.0)
}

}  // namespace gsr
