// gsr_math.h — per-Gaussian fp32 maths of the rasterizer (forward preprocess and its backward),
// written once as GSR_HD inline functions.  The HIP kernels (gsr_geom.hip) are thin load/store
// wrappers around these; tests/host_harness.cpp compiles the same functions with g++ so the
// formulas can be checked against the oracle without a GPU (test infrastructure, not a CPU path:
// nothing in the product loads that harness).
//
// Spec: SURVEY.md Appendix A.1-A.6 (forward), A.10 (backward).  Reference twins are cited inline
// (paths relative to /root/reference).
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/gsr_constants.h"

#if defined(__HIPCC__)
#define GSR_HD __host__ __device__ __forceinline__
#else
#define GSR_HD static inline
#endif

namespace gsr {

struct FrameK {            // kernel-side scalars derived from gsr_frame_desc
    int P, D, M, W, H, Gx, Gy, ty0, ty1;
    float tanfovx, tanfovy, focal_x, focal_y, scale_modifier;
};

// 48-byte record consumed by the binning and blend kernels (3 x float4).  The conic and the opacity are stored
// PRE-SCALED so that a pixel's alpha is ONE exp2 of a two-FMA quadratic:
//   qA = -0.5 log2(e) A,  qB = -log2(e) B,  qC = -0.5 log2(e) C,  lop = log2(opacity)
//   p(d) = qA dx^2 + qB dx dy + qC dy^2 + lop  =  log2(opacity * exp(power(d)))      =>  alpha = min(0.99, 2^p)
//   power(d) > 0  <=>  p > lop.
constexpr float kLog2e = 1.4426950408889634f;
struct Splat {
    float x, y, cA, cB;    // pixel-space mean, qA, qB
    float cC, op, r, g;    // qC, lop, colour r g
    float b, depth, rect_x, rect_y; // rect_x / rect_y: bit patterns of (x0 | x1 << 16), (y0 | y1 << 16): the tile
                                    // rectangle the binning walks (tight_rect below), slab-clipped
};

struct TileRect { int x0, y0, x1, y1; };

// ---- A.5: tile rectangle of a splat (slab-clipped in y).  int() truncates toward zero.
GSR_HD TileRect tile_rect(float px, float py, float radius, const FrameK &f)
{
    TileRect r;
    r.x0 = (int)((px - radius) / (float)GSR_TILE);
    r.y0 = (int)((py - radius) / (float)GSR_TILE);
    r.x1 = (int)((px + radius + (float)(GSR_TILE - 1)) / (float)GSR_TILE);
    r.y1 = (int)((py + radius + (float)(GSR_TILE - 1)) / (float)GSR_TILE);
    r.x0 = r.x0 < 0 ? 0 : (r.x0 > f.Gx ? f.Gx : r.x0);
    r.x1 = r.x1 < 0 ? 0 : (r.x1 > f.Gx ? f.Gx : r.x1);
    r.y0 = r.y0 < 0 ? 0 : (r.y0 > f.Gy ? f.Gy : r.y0);
    r.y1 = r.y1 < 0 ? 0 : (r.y1 > f.Gy ? f.Gy : r.y1);
    return r;
}

// ---- exact tile culling.  Returns false only when NO pixel of tile (tile_x, tile_y) can pass the blend's
// acceptance test (power <= 0 and alpha = min(0.99, op * exp(power)) >= 1/255, A.8) for this splat, so dropping
// the (tile, splat) instance changes no pixel and no gradient.  The maximum of the concave quadratic
// power(d) = -1/2 (A dx^2 + C dy^2) - B dx dy over the tile's pixel-centre rectangle (a superset of its 256
// pixels) is compared with the power at which alpha reaches 1/255, minus a margin that covers the blend
// kernels' fp32 evaluation error (few 1e-7 of the term magnitudes) and their exp2-based exponential (1e-6).
// A, B, C, opacity back from the pre-scaled record fields.
GSR_HD void unscale_conic(float qA, float qB, float qC, float lop, float &A, float &B, float &C, float &op)
{
    A = qA * (-2.f / kLog2e); B = qB * (-1.f / kLog2e); C = qC * (-2.f / kLog2e); op = exp2f(lop);
}

GSR_HD bool tile_may_contribute(float sx, float sy, float A, float B, float C, float op, int tile_x, int tile_y)
{
    if (op < (float)GSR_ALPHA_MIN) return false;             // op * G <= op < 1/255 for every G <= 1
    if (!(A > 0.f) || !(C > 0.f) || !(A * C - B * B > 0.f)) return true;     // not a proper ellipse: keep
    // d = splat - pixel, pixel in [16 t, 16 t + 15]
    const float dx0 = sx - (float)(tile_x * GSR_TILE + GSR_TILE - 1), dx1 = sx - (float)(tile_x * GSR_TILE);
    const float dy0 = sy - (float)(tile_y * GSR_TILE + GSR_TILE - 1), dy1 = sy - (float)(tile_y * GSR_TILE);
    if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) return true;   // centre inside the rectangle
    float qmax = -3.0e38f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 2; ++e) {
        const float ex = e ? dx1 : dx0;                         // edge dx = ex, dy free
        float dy = fminf(dy1, fmaxf(dy0, -B * ex / C));
        qmax = fmaxf(qmax, -0.5f * (A * ex * ex + C * dy * dy) - B * ex * dy);
        const float ey = e ? dy1 : dy0;                         // edge dy = ey, dx free
        float dx = fminf(dx1, fmaxf(dx0, -B * ey / A));
        qmax = fmaxf(qmax, -0.5f * (A * dx * dx + C * ey * ey) - B * dx * ey);
    }
    const float mx = fmaxf(fabsf(dx0), fabsf(dx1)), my = fmaxf(fabsf(dy0), fabsf(dy1));
    const float S = 0.5f * A * mx * mx + 0.5f * C * my * my + fabsf(B) * mx * my;
    const float need = -logf(255.f * op);                       // power at which op * exp(power) = 1/255
    return qmax >= need - (0.01f + 1e-5f * S);
}

// ---- sub-tile culling, same bound as tile_may_contribute on an arbitrary pixel rectangle [x0, x1] x [y0, y1] (pixel
// centres, inclusive), written on the PRE-SCALED record fields (Splat): p(d) = qA dx^2 + qB dx dy + qC dy^2 + lop is
// log2(opacity * exp(power(d))), a pixel accepts the splat iff log2(1/255) <= p and p <= lop.  Returns false only when
// no pixel of the rectangle can accept it (margins as in tile_may_contribute, in log2 units).
GSR_HD bool rect_may_contribute_q(float sx, float sy, float qA, float qB, float qC, float lop, float x0, float x1, float y0,
                                  float y1)
{
    const float kLog2AlphaMin = -7.994353437f;                  // log2(1/255)
    if (lop < kLog2AlphaMin) return false;
    if (!(qA < 0.f) || !(qC < 0.f) || !(4.f * qA * qC - qB * qB > 0.f)) return true;     // not a proper ellipse: keep
    const float dx0 = sx - x1, dx1 = sx - x0, dy0 = sy - y1, dy1 = sy - y0;         // d = splat - pixel
    if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) return true;          // centre inside the rectangle
    const float hC = -0.5f * qB / qC, hA = -0.5f * qB / qA;     // vertex of the 1-D quadratic along an edge
    float qmax = -3.0e38f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int e = 0; e < 2; ++e) {
        const float ex = e ? dx1 : dx0;                             // edge dx = ex, dy free
        const float dy = fminf(dy1, fmaxf(dy0, hC * ex));
        qmax = fmaxf(qmax, (qA * ex + qB * dy) * ex + qC * dy * dy);
        const float ey = e ? dy1 : dy0;                             // edge dy = ey, dx free
        const float dx = fminf(dx1, fmaxf(dx0, hA * ey));
        qmax = fmaxf(qmax, (qC * ey + qB * dx) * ey + qA * dx * dx);
    }
    const float mx = fmaxf(fabsf(dx0), fabsf(dx1)), my = fmaxf(fabsf(dy0), fabsf(dy1));
    const float S = -qA * mx * mx - qC * my * my + fabsf(qB) * mx * my;
    return qmax >= (kLog2AlphaMin - lop) - (0.0145f + 1e-5f * S);
}

// Bit k (k = qx + 2 qy) set <=> the 8x8 quadrant (qx, qy) of the 16x16 tile whose first pixel is (px0, py0) may hold a
// pixel that accepts the splat.  The blend kernels map one quadrant to one pixel per lane and skip clear quadrants.
GSR_HD unsigned quadrant_mask_q(float sx, float sy, float qA, float qB, float qC, float lop, float px0, float py0)
{
    unsigned m = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        const float x0 = px0 + (float)((k & 1) * (GSR_TILE / 2)), y0 = py0 + (float)((k >> 1) * (GSR_TILE / 2));
        if (rect_may_contribute_q(sx, sy, qA, qB, qC, lop, x0, x0 + (float)(GSR_TILE / 2 - 1), y0, y0 + (float)(GSR_TILE / 2 - 1)))
            m |= 1u << k;
    }
    return m;
}

// Cheaper, looser form of quadrant_mask_q for the emit kernels: the axis-aligned bounding box of the region where the
// splat's alpha can reach 1/255 (half-widths xe, ye: two square roots per SPLAT, see splat_extent_q) against each
// quadrant's pixel range: a handful of compares per tile.  Conservative (a superset of quadrant_mask_q's bits).
GSR_HD void splat_extent_q(float qA, float qB, float qC, float lop, float &xe, float &ye)
{
    const float kLog2AlphaMin = -7.994353437f;
    const float L = (lop - kLog2AlphaMin) * 1.001f + 0.02f;    // log2 units; covers rect_may_contribute_q's margins
    const float det = 4.f * qA * qC - qB * qB;
    if (!(qA < 0.f) || !(qC < 0.f) || !(det > 0.f) || !(L > 0.f)) { xe = L > 0.f ? 3.0e38f : -1.f; ye = xe; return; }
    // p(d) - lop = qA dx^2 + qB dx dy + qC dy^2 >= -L  <=>  a dx^2 + 2 b dx dy + c dy^2 <= L with a = -qA, b = -qB/2, c = -qC;
    // extents of that ellipse: |dx| <= sqrt(L c / (a c - b^2)), |dy| <= sqrt(L a / (a c - b^2)); a c - b^2 = det / 4
    const float k = 4.f * L / det;
    xe = sqrtf(k * -qC) * 1.001f + 0.01f;
    ye = sqrtf(k * -qA) * 1.001f + 0.01f;
}

GSR_HD unsigned quadrant_mask_bbox(float sx, float sy, float xe, float ye, float px0, float py0)
{
    if (xe < 0.f) return 0u;
    const float h = (float)(GSR_TILE / 2);
    // quadrant columns [px0, px0 + 7] and [px0 + 8, px0 + 15] against [sx - xe, sx + xe]; rows likewise
    const unsigned mx = ((sx - xe <= px0 + h - 1.f && sx + xe >= px0) ? 1u : 0u) | ((sx - xe <= px0 + 2.f * h - 1.f && sx + xe >= px0 + h) ? 2u : 0u);
    const unsigned my = ((sy - ye <= py0 + h - 1.f && sy + ye >= py0) ? 1u : 0u) | ((sy - ye <= py0 + 2.f * h - 1.f && sy + ye >= py0 + h) ? 2u : 0u);
    // bit k = qx + 2 qy
    return ((my & 1u) ? mx : 0u) | ((my & 2u) ? (mx << 2) : 0u);
}

GSR_HD void slab_clip(TileRect &r, const FrameK &f)
{
    if (r.y0 < f.ty0) r.y0 = f.ty0;
    if (r.y1 > f.ty1) r.y1 = f.ty1;
    if (r.y1 < r.y0) r.y1 = r.y0;
}

// ---- the rectangle the binning actually walks: the reference's A.5 rectangle (a pixel outside it never sees
// the splat, whatever its alpha) INTERSECTED with the bounding box of the region where alpha can reach 1/255:
// |dx| <= sqrt(2 L cov_xx), |dy| <= sqrt(2 L cov_yy), L = ln(255 opacity), cov = 2D covariance incl. dilation.
// Outside that box op * exp(power) < 1/255 for every pixel, so no tile there can take the splat: exact.
// 2 % + 0.5 px of margin covers the blend kernels' fp32 arithmetic.  L <= 0: the splat is never accepted.
GSR_HD TileRect tight_rect(const TileRect &ref, float px, float py, float cov_xx, float cov_yy, float opacity)
{
    TileRect r = ref;
    const float L = logf(255.f * opacity);
    if (!(L > 0.f)) { r.x1 = r.x0; r.y1 = r.y0; return r; }
    const float xe = 1.02f * sqrtf(2.f * L * cov_xx) + 0.5f, ye = 1.02f * sqrtf(2.f * L * cov_yy) + 0.5f;
    const float inv = 1.f / (float)GSR_TILE;
    const int x0 = (int)floorf((px - xe) * inv), x1 = (int)floorf((px + xe) * inv) + 1;
    const int y0 = (int)floorf((py - ye) * inv), y1 = (int)floorf((py + ye) * inv) + 1;
    if (x0 > r.x0) r.x0 = x0;
    if (x1 < r.x1) r.x1 = x1;
    if (y0 > r.y0) r.y0 = y0;
    if (y1 < r.y1) r.y1 = y1;
    if (r.x1 < r.x0) r.x1 = r.x0;
    if (r.y1 < r.y0) r.y1 = r.y0;
    return r;
}

GSR_HD float pack_u16x2(int lo, int hi)
{
    const uint32_t u = ((uint32_t)lo & 0xFFFFu) | (((uint32_t)hi & 0xFFFFu) << 16);
    float f;
    memcpy(&f, &u, 4);
    return f;
}

GSR_HD TileRect unpack_rect(float rx, float ry)
{
    uint32_t ux, uy;
    memcpy(&ux, &rx, 4);
    memcpy(&uy, &ry, 4);
    TileRect r;
    r.x0 = (int)(ux & 0xFFFFu); r.x1 = (int)(ux >> 16);
    r.y0 = (int)(uy & 0xFFFFu); r.y1 = (int)(uy >> 16);
    return r;
}

// ---- A.3: rotation from quaternion (r,x,y,z) used as given; utils/general_utils.py:90-98.
GSR_HD void quat_to_rot(const float q[4], float R[9])
{
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - r * z);       R[2] = 2.f * (x * z + r * y);
    R[3] = 2.f * (x * y + r * z);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - r * x);
    R[6] = 2.f * (x * z - r * y);       R[7] = 2.f * (y * z + r * x);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// ---- A.3: Sigma = R diag(mod*s)^2 R^T packed [xx,xy,xz,yy,yz,zz]; scene/gaussian_model.py:25-29.
GSR_HD void cov3d_from_scale_rot(const float s[3], float mod, const float q[4], float cov[6])
{
    float R[9];
    quat_to_rot(q, R);
    const float s0 = mod * s[0], s1 = mod * s[1], s2 = mod * s[2];
    const float v0 = s0 * s0, v1 = s1 * s1, v2 = s2 * s2;
    cov[0] = R[0] * R[0] * v0 + R[1] * R[1] * v1 + R[2] * R[2] * v2;
    cov[1] = R[0] * R[3] * v0 + R[1] * R[4] * v1 + R[2] * R[5] * v2;
    cov[2] = R[0] * R[6] * v0 + R[1] * R[7] * v1 + R[2] * R[8] * v2;
    cov[3] = R[3] * R[3] * v0 + R[4] * R[4] * v1 + R[5] * R[5] * v2;
    cov[4] = R[3] * R[6] * v0 + R[4] * R[7] * v1 + R[5] * R[8] * v2;
    cov[5] = R[6] * R[6] * v0 + R[7] * R[7] * v1 + R[8] * R[8] * v2;
}

// p_view component k of a world point (transformPoint4x3 with the transposed view matrix V): evaluated as ONE fixed binary32
// expression, fma(p2, V[8+k], fma(p1, V[4+k], p0 * V[k])) + V[12+k] -- the reference compiler's contraction of the left-to-right
// sum, and one of the evaluations the oracle's depth band holds (oracle/gsr_oracle_impl.h "dB").  Left to the compiler, the device
// contracted the first multiply instead (fma(p2, ., fma(p0, ., p1 * .))): at a posed camera the terms cancel (|p_view.z| ~ 0.2 from
// terms ~ 0.5) and that evaluation is a few ulps away, so two splats an ulp apart swapped depth order outside the oracle's band.
// z is the depth sort key and the near cut (A.1), so preprocess, geometry backward and markVisible all use this one function.
GSR_HD float view_coord(const float p[3], const float *V, int k)
{
    return fmaf(p[2], V[8 + k], fmaf(p[1], V[4 + k], p[0] * V[k])) + V[12 + k];
}

// Shared by forward and backward: everything the EWA projection (A.4) derives from p_view and Sigma.
struct Ewa {
    float tx, ty, tz;            // clamped view-space point
    float xmul, ymul;            // 0 where tx/tz (ty/tz) was clamped, else 1
    float T[6];                  // T = J * R_w2c (2x3, row-major)
    float S0[3], S1[3];          // rows of T * Sigma
    float a, b, c;               // 2D covariance entries incl. the 0.3 dilation
};

GSR_HD void ewa_project(const float pv[3], const float cov[6], const float *V, const FrameK &f, Ewa &e)
{
    const float limx = (float)GSR_FOV_CLAMP * f.tanfovx, limy = (float)GSR_FOV_CLAMP * f.tanfovy;
    const float txtz = pv[0] / pv[2], tytz = pv[1] / pv[2];
    e.xmul = (txtz < -limx || txtz > limx) ? 0.f : 1.f;
    e.ymul = (tytz < -limy || tytz > limy) ? 0.f : 1.f;
    e.tx = fminf(limx, fmaxf(-limx, txtz)) * pv[2];
    e.ty = fminf(limy, fmaxf(-limy, tytz)) * pv[2];
    e.tz = pv[2];
    const float J00 = f.focal_x / e.tz, J02 = -(f.focal_x * e.tx) / (e.tz * e.tz);
    const float J11 = f.focal_y / e.tz, J12 = -(f.focal_y * e.ty) / (e.tz * e.tz);
    // R_w2c[i][j] = V[j][i] with V the transposed (row-vector) view matrix, scene/cameras.py:54
    e.T[0] = J00 * V[0] + J02 * V[2];  e.T[1] = J00 * V[4] + J02 * V[6];  e.T[2] = J00 * V[8] + J02 * V[10];
    e.T[3] = J11 * V[1] + J12 * V[2];  e.T[4] = J11 * V[5] + J12 * V[6];  e.T[5] = J11 * V[9] + J12 * V[10];
    e.S0[0] = cov[0] * e.T[0] + cov[1] * e.T[1] + cov[2] * e.T[2];
    e.S0[1] = cov[1] * e.T[0] + cov[3] * e.T[1] + cov[4] * e.T[2];
    e.S0[2] = cov[2] * e.T[0] + cov[4] * e.T[1] + cov[5] * e.T[2];
    e.S1[0] = cov[0] * e.T[3] + cov[1] * e.T[4] + cov[2] * e.T[5];
    e.S1[1] = cov[1] * e.T[3] + cov[3] * e.T[4] + cov[4] * e.T[5];
    e.S1[2] = cov[2] * e.T[3] + cov[4] * e.T[4] + cov[5] * e.T[5];
    e.a = e.T[0] * e.S0[0] + e.T[1] * e.S0[1] + e.T[2] * e.S0[2] + (float)GSR_COV2D_DILATE;
    e.b = e.T[0] * e.S1[0] + e.T[1] * e.S1[1] + e.T[2] * e.S1[2];
    e.c = e.T[3] * e.S1[0] + e.T[4] * e.S1[1] + e.T[5] * e.S1[2] + (float)GSR_COV2D_DILATE;
}

// ---- A.6: SH basis (utils/sh_utils.py:74-100) and its derivatives wrt the unit direction.
template <bool WITH_GRAD>
GSR_HD void sh_basis(int D, float x, float y, float z, float *b, float *bx, float *by, float *bz)
{
    b[0] = (float)GSR_SH_C0;
    if (WITH_GRAD) { bx[0] = by[0] = bz[0] = 0.f; }
    if (D > 0) {
        b[1] = -(float)GSR_SH_C1 * y; b[2] = (float)GSR_SH_C1 * z; b[3] = -(float)GSR_SH_C1 * x;
        if (WITH_GRAD) {
            bx[1] = 0.f; by[1] = -(float)GSR_SH_C1; bz[1] = 0.f;
            bx[2] = 0.f; by[2] = 0.f; bz[2] = (float)GSR_SH_C1;
            bx[3] = -(float)GSR_SH_C1; by[3] = 0.f; bz[3] = 0.f;
        }
        if (D > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            b[4] = (float)GSR_SH_C2_0 * xy;
            b[5] = (float)GSR_SH_C2_1 * yz;
            b[6] = (float)GSR_SH_C2_2 * (2.f * zz - xx - yy);
            b[7] = (float)GSR_SH_C2_3 * xz;
            b[8] = (float)GSR_SH_C2_4 * (xx - yy);
            if (WITH_GRAD) {
                bx[4] = (float)GSR_SH_C2_0 * y; by[4] = (float)GSR_SH_C2_0 * x; bz[4] = 0.f;
                bx[5] = 0.f; by[5] = (float)GSR_SH_C2_1 * z; bz[5] = (float)GSR_SH_C2_1 * y;
                bx[6] = (float)GSR_SH_C2_2 * -2.f * x; by[6] = (float)GSR_SH_C2_2 * -2.f * y; bz[6] = (float)GSR_SH_C2_2 * 4.f * z;
                bx[7] = (float)GSR_SH_C2_3 * z; by[7] = 0.f; bz[7] = (float)GSR_SH_C2_3 * x;
                bx[8] = (float)GSR_SH_C2_4 * 2.f * x; by[8] = (float)GSR_SH_C2_4 * -2.f * y; bz[8] = 0.f;
            }
            if (D > 2) {
                b[9]  = (float)GSR_SH_C3_0 * y * (3.f * xx - yy);
                b[10] = (float)GSR_SH_C3_1 * xy * z;
                b[11] = (float)GSR_SH_C3_2 * y * (4.f * zz - xx - yy);
                b[12] = (float)GSR_SH_C3_3 * z * (2.f * zz - 3.f * xx - 3.f * yy);
                b[13] = (float)GSR_SH_C3_4 * x * (4.f * zz - xx - yy);
                b[14] = (float)GSR_SH_C3_5 * z * (xx - yy);
                b[15] = (float)GSR_SH_C3_6 * x * (xx - 3.f * yy);
                if (WITH_GRAD) {
                    bx[9]  = (float)GSR_SH_C3_0 * 6.f * xy;  by[9]  = (float)GSR_SH_C3_0 * (3.f * xx - 3.f * yy); bz[9] = 0.f;
                    bx[10] = (float)GSR_SH_C3_1 * yz;        by[10] = (float)GSR_SH_C3_1 * xz;  bz[10] = (float)GSR_SH_C3_1 * xy;
                    bx[11] = (float)GSR_SH_C3_2 * -2.f * xy; by[11] = (float)GSR_SH_C3_2 * (4.f * zz - xx - 3.f * yy); bz[11] = (float)GSR_SH_C3_2 * 8.f * yz;
                    bx[12] = (float)GSR_SH_C3_3 * -6.f * xz; by[12] = (float)GSR_SH_C3_3 * -6.f * yz; bz[12] = (float)GSR_SH_C3_3 * (6.f * zz - 3.f * xx - 3.f * yy);
                    bx[13] = (float)GSR_SH_C3_4 * (4.f * zz - 3.f * xx - yy); by[13] = (float)GSR_SH_C3_4 * -2.f * xy; bz[13] = (float)GSR_SH_C3_4 * 8.f * xz;
                    bx[14] = (float)GSR_SH_C3_5 * 2.f * xz;  by[14] = (float)GSR_SH_C3_5 * -2.f * yz; bz[14] = (float)GSR_SH_C3_5 * (xx - yy);
                    bx[15] = (float)GSR_SH_C3_6 * (3.f * xx - 3.f * yy); by[15] = (float)GSR_SH_C3_6 * -6.f * xy; bz[15] = 0.f;
                }
            }
        }
    }
}

struct PreOut {
    int radius;            // 0 = invisible
    unsigned tiles;        // tiles touched inside the slab
    unsigned clamped;      // bit c: channel c clamped at 0
    float mass;            // optical mass inside the slab, pixel x nepers (optical_mass below); 0 when no tile is touched
    Splat s;
};

// ---- optical mass of a splat: the integral over the image plane of its optical depth tau(x) = -ln(1 - alpha(x)),
// alpha(x) = opacity * exp(power(x)).  For a 2D Gaussian of covariance Sigma' that integral is
// 2 pi sqrt(det Sigma') * Li2(opacity) (dilogarithm; = opacity * 2 pi sqrt(det) for faint splats).  A pixel takes the
// blend's transmittance cut-off (T < 1e-4, A.8) once the optical depths in front of it sum to ln(1e4) = 9.21, so
// the running sum of masses in depth order, divided by the pixel count, is the frame's mean optical depth: the
// chunk plan (gsr_binning.hip) cuts the depth order where that mean reaches a fixed multiple of 9.21 instead of at
// a swept instance count.  Capped by what the splat's binning rectangle can hold, scaled to the slab's share of it.
GSR_HD float optical_mass(float det_cov2d, float opacity, int rect_tiles_full, int rect_tiles_slab)
{
    if (rect_tiles_full <= 0 || rect_tiles_slab <= 0) return 0.f;
    const float op = fminf(fmaxf(opacity, 0.f), (float)GSR_ALPHA_MAX);
    const float li2 = op * (1.f + op * (0.25f + 0.39f * op * op));             // Li2 on [0, 1] to 2 %
    float m = 6.2831853f * sqrtf(fmaxf(det_cov2d, 0.f)) * li2;
    const float cap = (float)rect_tiles_full * (float)(GSR_TILE * GSR_TILE) * -logf(1.f - op);
    m = fminf(m, cap);
    return m * ((float)rect_tiles_slab / (float)rect_tiles_full);
}

// ---- A.6: colour of one Gaussian from its [K,3] SH coefficients (+0.5, clamp at 0; bit c of `clamped` = channel c
// clamped).  Its own function because the forward evaluates it LAZILY: only for the depth chunks that are binned.
template <int DEG = -1>
GSR_HD void sh_color_one(const FrameK &f, const float *campos, const float p[3], const float *sh, float rgb[3], unsigned &clamped)
{
    float dx = p[0] - campos[0], dy = p[1] - campos[1], dz = p[2] - campos[2];
    const float inv = 1.f / sqrtf(dx * dx + dy * dy + dz * dz);
    dx *= inv; dy *= inv; dz *= inv;
    float bas[16];
    const int D = DEG >= 0 ? DEG : f.D;          // DEG >= 0: compile-time degree, loops unroll
    sh_basis<false>(D, dx, dy, dz, bas, nullptr, nullptr, nullptr);
    const int K = (D + 1) * (D + 1);
    clamped = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int ch = 0; ch < 3; ++ch) {
        float acc = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < K; ++k) acc += bas[k] * sh[3 * k + ch];
        acc += (float)GSR_SH_OFFSET;
        if (acc < 0.f) { clamped |= 1u << ch; acc = 0.f; }
        rgb[ch] = acc;
    }
}

// ---- A.1-A.6 for one Gaussian.  `sh` points at this Gaussian's [M,3] coefficients (or null: then, without a
// precomputed colour, the colour is left at 0 for a later sh_color_one), `colpre` at its precomputed colour (or
// null), `covpre` at its precomputed covariance (or null).
template <int DEG = -1>
GSR_HD void preprocess_one(const FrameK &f, const float *V, const float *PV, const float *campos,
                           const float p[3], const float *scale, const float *quat, const float *covpre,
                           float opacity, const float *sh, const float *colpre, PreOut &o)
{
    o.radius = 0; o.tiles = 0; o.clamped = 0; o.mass = 0.f;
    o.s = Splat{0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float pv[3];
    pv[0] = view_coord(p, V, 0);
    pv[1] = view_coord(p, V, 1);
    pv[2] = view_coord(p, V, 2);
    if (pv[2] <= (float)GSR_NEAR_CUT) return;                                   // A.1
    const float hx = p[0] * PV[0] + p[1] * PV[4] + p[2] * PV[8] + PV[12];
    const float hy = p[0] * PV[1] + p[1] * PV[5] + p[2] * PV[9] + PV[13];
    const float hw = p[0] * PV[3] + p[1] * PV[7] + p[2] * PV[11] + PV[15];
    const float pw = 1.f / (hw + (float)GSR_HOM_EPS);                           // A.2
    const float ndcx = hx * pw, ndcy = hy * pw;

    float cov[6];
    if (covpre) { for (int k = 0; k < 6; ++k) cov[k] = covpre[k]; }
    else cov3d_from_scale_rot(scale, f.scale_modifier, quat, cov);

    Ewa e;
    ewa_project(pv, cov, V, f, e);
    const float det = e.a * e.c - e.b * e.b;
    if (det == 0.f) return;
    const float det_inv = 1.f / det;
    const float mid = 0.5f * (e.a + e.c);
    const float disc = fmaxf((float)GSR_LAMBDA_FLOOR, mid * mid - det);
    const float sq = sqrtf(disc);
    const float lmax = fmaxf(mid + sq, mid - sq);
    const float my_radius = ceilf((float)GSR_RADIUS_SIGMAS * sqrtf(lmax));
    const float px = ((ndcx + 1.f) * (float)f.W - 1.f) * 0.5f;
    const float py = ((ndcy + 1.f) * (float)f.H - 1.f) * 0.5f;
    TileRect r = tile_rect(px, py, my_radius, f);
    if ((r.x1 - r.x0) * (r.y1 - r.y0) == 0) return;

    float rgb[3] = {0.f, 0.f, 0.f};
    if (colpre) { rgb[0] = colpre[0]; rgb[1] = colpre[1]; rgb[2] = colpre[2]; }
    else if (sh) sh_color_one<DEG>(f, campos, p, sh, rgb, o.clamped);
    o.radius = (int)my_radius;
    o.s.x = px; o.s.y = py;
    o.s.cA = (-0.5f * kLog2e) * (e.c * det_inv); o.s.cB = -kLog2e * (-e.b * det_inv); o.s.cC = (-0.5f * kLog2e) * (e.a * det_inv);
    o.s.op = log2f(opacity);
    o.s.r = rgb[0]; o.s.g = rgb[1]; o.s.b = rgb[2];
    o.s.depth = pv[2];
    TileRect t = tight_rect(r, px, py, e.a, e.c, opacity);
    const int full_tiles = (t.x1 - t.x0) * (t.y1 - t.y0);
    slab_clip(t, f);
    o.s.rect_x = pack_u16x2(t.x0, t.x1);
    o.s.rect_y = pack_u16x2(t.y0, t.y1);
    o.tiles = (unsigned)((t.x1 - t.x0) * (t.y1 - t.y0));
    o.mass = optical_mass(det, opacity, full_tiles, (int)o.tiles);
}

struct GeomGrad {
    float dmean[3], dmean2D[2], dopacity, dcolor[3], dscale[3], drot[4], dcov[6];
};

// ---- the pieces of A.10 that geom_backward_one and camera_backward_one are both built from.
// The forward's EWA projection of one Gaussian, recomputed.
GSR_HD void ewa_of_gaussian(const FrameK &f, const float *V, const float p[3], const float *scale, const float *quat,
                            const float *covpre, Ewa &e)
{
    float pv[3];
    pv[0] = view_coord(p, V, 0);
    pv[1] = view_coord(p, V, 1);
    pv[2] = view_coord(p, V, 2);
    float cov[6];
    if (covpre) { for (int k = 0; k < 6; ++k) cov[k] = covpre[k]; }
    else cov3d_from_scale_rot(scale, f.scale_modifier, quat, cov);
    ewa_project(pv, cov, V, f, e);
}

// The screen chain: conic -> 2D covariance -> T = J R_w2c -> J -> clamped view-space point, for sg = (dmean2D.x, dmean2D.y, gA, gB, gC, ...).
struct ScreenChain {
    float dL_da, dL_db, dL_dc;   // dL/d(2D covariance entries)
    float dT0[3], dT1[3];        // dL/dT rows = 2 G2 T Sigma
    float dtx, dty, dtz;         // dL/d(tx, ty, tz); dtx / dty carry the frustum clamp's xmul / ymul
};

// The chain behind dL/dT, shared with the opacity compensation (opacity_compensation_backward_one): s.dT0, s.dT1 -> J -> clamped
// view-space point (s.dtx, s.dty, s.dtz).
GSR_HD void jacobian_chain_backward(const FrameK &f, const float *V, const Ewa &e, ScreenChain &s)
{
    const float *dT0 = s.dT0, *dT1 = s.dT1;
    // dL/dJ (non-zeros of J) = dL/dT R_w2c^T
    const float dJ00 = V[0] * dT0[0] + V[4] * dT0[1] + V[8] * dT0[2];
    const float dJ02 = V[2] * dT0[0] + V[6] * dT0[1] + V[10] * dT0[2];
    const float dJ11 = V[1] * dT1[0] + V[5] * dT1[1] + V[9] * dT1[2];
    const float dJ12 = V[2] * dT1[0] + V[6] * dT1[1] + V[10] * dT1[2];
    const float tzi = 1.f / e.tz, tz2 = tzi * tzi, tz3 = tz2 * tzi;
    s.dtx = e.xmul * -f.focal_x * tz2 * dJ02;
    s.dty = e.ymul * -f.focal_y * tz2 * dJ12;
    s.dtz = -f.focal_x * tz2 * dJ00 - f.focal_y * tz2 * dJ11 + (2.f * f.focal_x * e.tx) * tz3 * dJ02 +
            (2.f * f.focal_y * e.ty) * tz3 * dJ12;
}

GSR_HD void screen_chain_backward(const FrameK &f, const float *V, const Ewa &e, const float sg[9], ScreenChain &s)
{
    // conic -> 2D covariance (stored gB is half the derivative wrt the scalar B, A.9 note)
    const float den = e.a * e.c - e.b * e.b;
    const float k2 = 1.f / (den * den + (float)GSR_CONIC_BWD_EPS);
    const float gA = sg[2], gB = sg[3], gC = sg[4];
    const float dL_da = k2 * (-e.c * e.c * gA + 2.f * e.b * e.c * gB + (den - e.a * e.c) * gC);
    const float dL_dc = k2 * (-e.a * e.a * gC + 2.f * e.a * e.b * gB + (den - e.a * e.c) * gA);
    const float dL_db = k2 * 2.f * (e.b * e.c * gA - (den + 2.f * e.b * e.b) * gB + e.a * e.b * gC);
    s.dL_da = dL_da; s.dL_db = dL_db; s.dL_dc = dL_dc;
    // dL/dT = 2 G2 T Sigma
    float *dT0 = s.dT0, *dT1 = s.dT1;
    dT0[0] = 2.f * e.S0[0] * dL_da + e.S1[0] * dL_db; dT0[1] = 2.f * e.S0[1] * dL_da + e.S1[1] * dL_db;
    dT0[2] = 2.f * e.S0[2] * dL_da + e.S1[2] * dL_db;
    dT1[0] = 2.f * e.S1[0] * dL_dc + e.S0[0] * dL_db; dT1[1] = 2.f * e.S1[1] * dL_dc + e.S0[1] * dL_db;
    dT1[2] = 2.f * e.S1[2] * dL_dc + e.S0[2] * dL_db;
    jacobian_chain_backward(f, V, e, s);
}

// Homogeneous divide (A.2): ndc = (hx, hy) mw, so d ndc.x / d(hx, hw) = (mw, -mul1) and d ndc.y / d(hy, hw) = (mw, -mul2).
GSR_HD void hom_divide_backward(const float p[3], const float *PV, float &mw, float &mul1, float &mul2)
{
    const float hx = p[0] * PV[0] + p[1] * PV[4] + p[2] * PV[8] + PV[12];
    const float hy = p[0] * PV[1] + p[1] * PV[5] + p[2] * PV[9] + PV[13];
    const float hw = p[0] * PV[3] + p[1] * PV[7] + p[2] * PV[11] + PV[15];
    mw = 1.f / (hw + (float)GSR_HOM_EPS);
    mul1 = hx * mw * mw; mul2 = hy * mw * mw;
}

// SH colour (A.6) back to the view direction d = (p - campos) / |p - campos|: dd[k] = dL/dp_k = -dL/dcampos_k, through normalize().
// DSH (compile time; the camera side passes false) and want_dsh: dsh (this Gaussian's [K,3] row) receives basis_k * dRGB for k < K;
// the caller zeroes k >= K.  It may point anywhere (registers, an LDS staging row, the output tensor itself) but never depends on a
// run-time select, so that a register array stays in registers.  clamped: bit c set <=> channel c was clamped.
template <int DEG, bool DSH>
GSR_HD void sh_direction_backward(const FrameK &f, const float *campos, const float p[3], const float *sh, unsigned clamped,
                                  const float sg[9], float dd[3], float *dsh, bool want_dsh, bool has_colpre)
{
    dd[0] = dd[1] = dd[2] = 0.f;
    if (has_colpre) return;
    const float ox = p[0] - campos[0], oy = p[1] - campos[1], oz = p[2] - campos[2];
    const float inv = 1.f / sqrtf(ox * ox + oy * oy + oz * oz);
    const float dxn = ox * inv, dyn = oy * inv, dzn = oz * inv;
    float bas[16], bx[16], by[16], bz[16];
    const int D = DEG >= 0 ? DEG : f.D;
    sh_basis<true>(D, dxn, dyn, dzn, bas, bx, by, bz);
    const int K = (D + 1) * (D + 1);
    float ddx = 0.f, ddy = 0.f, ddz = 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int ch = 0; ch < 3; ++ch) {
        const float dRGB = ((clamped >> ch) & 1u) ? 0.f : sg[6 + ch];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < K; ++k) {
            const float c = sh[3 * k + ch] * dRGB;
            if (DSH && want_dsh) dsh[3 * k + ch] = bas[k] * dRGB;
            ddx += bx[k] * c; ddy += by[k] * c; ddz += bz[k] * c;
        }
    }
    const float dot = dxn * ddx + dyn * ddy + dzn * ddz;           // through normalize()
    dd[0] = (ddx - dxn * dot) * inv;
    dd[1] = (ddy - dyn * dot) * inv;
    dd[2] = (ddz - dzn * dot) * inv;
}

// Two steps of A.10 that the opacity compensation takes too.  The view term of dL/dmeans3D from dL/d(tx, ty, tz):
GSR_HD void view_point_backward(const float *V, const ScreenChain &s, float dmean[3])
{
    dmean[0] = V[0] * s.dtx + V[1] * s.dty + V[2] * s.dtz;
    dmean[1] = V[4] * s.dtx + V[5] * s.dty + V[6] * s.dtz;
    dmean[2] = V[8] * s.dtx + V[9] * s.dty + V[10] * s.dtz;
}

// quat_to_rot back: gR = dL/dR (row-major, gR[3 i + j] = dL/dR[i][j]) -> dL/dq for the quaternion as given (not normalised here).
GSR_HD void quat_to_rot_backward(const float quat[4], const float gR[9], float drot[4])
{
    const float r = quat[0], x = quat[1], y = quat[2], z = quat[3];
    drot[0] = 2.f * (-z * gR[1] + y * gR[2] + z * gR[3] - x * gR[5] - y * gR[6] + x * gR[7]);
    drot[1] = 2.f * (y * gR[1] + z * gR[2] + y * gR[3] - 2.f * x * gR[4] - r * gR[5] + z * gR[6] + r * gR[7] - 2.f * x * gR[8]);
    drot[2] = 2.f * (-2.f * y * gR[0] + x * gR[1] + r * gR[2] + x * gR[3] + z * gR[5] - r * gR[6] + z * gR[7] - 2.f * y * gR[8]);
    drot[3] = 2.f * (-2.f * z * gR[0] - r * gR[1] + x * gR[2] + r * gR[3] - 2.f * z * gR[4] + y * gR[5] + x * gR[6] + y * gR[7]);
}

// ---- A.10 for one visible Gaussian.  sg = (dmean2D.x, dmean2D.y, gA, gB, gC, dopacity, drgb[3]).
// dsh, want_dsh, clamped: see sh_direction_backward.
template <int DEG = -1>
GSR_HD void geom_backward_one(const FrameK &f, const float *V, const float *PV, const float *campos,
                              const float p[3], const float *scale, const float *quat, const float *covpre,
                              const float *sh, bool has_colpre, unsigned clamped, const float sg[9],
                              GeomGrad &g, float *dsh, bool want_dsh = true)
{
    Ewa e;
    ewa_of_gaussian(f, V, p, scale, quat, covpre, e);

    g.dmean2D[0] = sg[0]; g.dmean2D[1] = sg[1];
    g.dopacity = sg[5];

    ScreenChain s;
    screen_chain_backward(f, V, e, sg, s);
    const float dL_da = s.dL_da, dL_db = s.dL_db, dL_dc = s.dL_dc;
    const float *T = e.T;
    g.dcov[0] = T[0] * T[0] * dL_da + T[0] * T[3] * dL_db + T[3] * T[3] * dL_dc;
    g.dcov[3] = T[1] * T[1] * dL_da + T[1] * T[4] * dL_db + T[4] * T[4] * dL_dc;
    g.dcov[5] = T[2] * T[2] * dL_da + T[2] * T[5] * dL_db + T[5] * T[5] * dL_dc;
    g.dcov[1] = 2.f * T[0] * T[1] * dL_da + (T[0] * T[4] + T[1] * T[3]) * dL_db + 2.f * T[3] * T[4] * dL_dc;
    g.dcov[2] = 2.f * T[0] * T[2] * dL_da + (T[0] * T[5] + T[2] * T[3]) * dL_db + 2.f * T[3] * T[5] * dL_dc;
    g.dcov[4] = 2.f * T[2] * T[1] * dL_da + (T[1] * T[5] + T[2] * T[4]) * dL_db + 2.f * T[4] * T[5] * dL_dc;
    view_point_backward(V, s, g.dmean);

    // projection path
    float mw, mul1, mul2;
    hom_divide_backward(p, PV, mw, mul1, mul2);
    g.dmean[0] += (PV[0] * mw - PV[3] * mul1) * sg[0] + (PV[1] * mw - PV[3] * mul2) * sg[1];
    g.dmean[1] += (PV[4] * mw - PV[7] * mul1) * sg[0] + (PV[5] * mw - PV[7] * mul2) * sg[1];
    g.dmean[2] += (PV[8] * mw - PV[11] * mul1) * sg[0] + (PV[9] * mw - PV[11] * mul2) * sg[1];

    // colour path
    g.dcolor[0] = sg[6]; g.dcolor[1] = sg[7]; g.dcolor[2] = sg[8];
    float dd[3];
    sh_direction_backward<DEG, true>(f, campos, p, sh, clamped, sg, dd, dsh, want_dsh, has_colpre);
    if (!has_colpre) { g.dmean[0] += dd[0]; g.dmean[1] += dd[1]; g.dmean[2] += dd[2]; }

    // 3D covariance path
    for (int k = 0; k < 3; ++k) g.dscale[k] = 0.f;
    for (int k = 0; k < 4; ++k) g.drot[k] = 0.f;
    if (!covpre) {
        float R[9];
        quat_to_rot(quat, R);
        const float s[3] = {f.scale_modifier * scale[0], f.scale_modifier * scale[1], f.scale_modifier * scale[2]};
        const float G3[9] = {g.dcov[0], 0.5f * g.dcov[1], 0.5f * g.dcov[2], 0.5f * g.dcov[1], g.dcov[3],
                             0.5f * g.dcov[4], 0.5f * g.dcov[2], 0.5f * g.dcov[4], g.dcov[5]};
        float gR[9];
        for (int k = 0; k < 3; ++k) {
            float ds = 0.f;
            for (int j = 0; j < 3; ++j) {
                // dM[k][j] = 2 * sum_l s_k R[l][k] G3[l][j]
                const float dM = 2.f * s[k] * (R[k] * G3[j] + R[3 + k] * G3[3 + j] + R[6 + k] * G3[6 + j]);
                ds += R[3 * j + k] * dM;
                gR[3 * j + k] = s[k] * dM;
            }
            g.dscale[k] = ds;                     // scale_modifier factor omitted (A.10)
        }
        quat_to_rot_backward(quat, gR, g.drot);
    }
}

// ---- camera gradients of one visible Gaussian: what A.10 computes on its way to dL/dmeans3D and drops,
// turned into this Gaussian's contribution to dL/dviewmatrix, dL/dprojmatrix and dL/dcampos.  Row-vector convention of the header
// (p_view_c = sum_r p_r V[4r+c] + V[12+c]); with ph = (p, 1):
//   c[3r + k]       dL/dV[4r+k], k = 0..2:  ph_r (dtx, dty, dtz)_k  (p_view; dtx / dty carry xmul / ymul as for means3D)
//                                           + for r < 3, through T = J R_w2c:  J00 dT0r | J11 dT1r | J02 dT0r + J12 dT1r
//   c[12 + 3r + k]  dL/dPV[4r + (0, 1, 3)[k]]:  ph_r (mw sg0, mw sg1, -(mul1 sg0 + mul2 sg1))_k
//   c[24 + k]       dL/dcampos_k = minus the SH view-direction term of dL/dmeans3D (zero with a precomputed colour)
// Column 3 of V and column 2 of PV are never read by the forward: their gradients are exact zeros and have no slot here.
// The 27 terms are ADDED to c (the caller zeroes it; a thread that visits several Gaussians keeps one set of accumulators).
// Built from the same pieces as geom_backward_one (ewa_of_gaussian ... sh_direction_backward above).
constexpr int kCamTerms = 27;

template <int DEG = -1>
GSR_HD void camera_backward_one(const FrameK &f, const float *V, const float *PV, const float *campos, const float p[3],
                                const float *scale, const float *quat, const float *covpre, const float *sh, bool has_colpre,
                                unsigned clamped, const float sg[9], float c[kCamTerms])
{
    Ewa e;
    ewa_of_gaussian(f, V, p, scale, quat, covpre, e);

    ScreenChain s;
    screen_chain_backward(f, V, e, sg, s);
    const float J00 = f.focal_x / e.tz, J02 = -(f.focal_x * e.tx) / (e.tz * e.tz);
    const float J11 = f.focal_y / e.tz, J12 = -(f.focal_y * e.ty) / (e.tz * e.tz);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 3; ++r) {
        c[3 * r + 0] += p[r] * s.dtx + J00 * s.dT0[r];
        c[3 * r + 1] += p[r] * s.dty + J11 * s.dT1[r];
        c[3 * r + 2] += p[r] * s.dtz + (J02 * s.dT0[r] + J12 * s.dT1[r]);
    }
    c[9] += s.dtx; c[10] += s.dty; c[11] += s.dtz;

    // projection path: ndc = (hx, hy) mw
    float mw, mul1, mul2;
    hom_divide_backward(p, PV, mw, mul1, mul2);
    const float dh0 = mw * sg[0], dh1 = mw * sg[1], dh3 = -(mul1 * sg[0] + mul2 * sg[1]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 3; ++r) { c[12 + 3 * r] += p[r] * dh0; c[13 + 3 * r] += p[r] * dh1; c[14 + 3 * r] += p[r] * dh3; }
    c[21] += dh0; c[22] += dh1; c[23] += dh3;

    // colour path: the view direction is (p - campos) / |p - campos|
    float dd[3];
    sh_direction_backward<DEG, false>(f, campos, p, sh, clamped, sg, dd, nullptr, false, has_colpre);
    if (!has_colpre) { c[24] -= dd[0]; c[25] -= dd[1]; c[26] -= dd[2]; }
}

// ---- the activations of the reference's parameter store, for the raw-parameter mode
// (scene/gaussian_model.py:47-60: scaling exp, opacity sigmoid, rotation torch.nn.functional.normalize with
// eps 1e-12; :108-127 getters).  activate_raw_backward turns the gradients w.r.t. the activated values into
// gradients w.r.t. the raw parameters, in place.
struct RawAct {
    float scale[3], q[4], opacity, inv_norm;
    bool clamped_norm;     // |raw quaternion| < eps: normalize() divided by eps, not by the norm
};

GSR_HD void activate_raw(const float log_scale[3], const float raw_q[4], float logit, RawAct &a)
{
    for (int k = 0; k < 3; ++k) a.scale[k] = expf(log_scale[k]);
    const float n = sqrtf(raw_q[0] * raw_q[0] + raw_q[1] * raw_q[1] + raw_q[2] * raw_q[2] + raw_q[3] * raw_q[3]);
    a.clamped_norm = n < 1e-12f;
    a.inv_norm = 1.f / fmaxf(n, 1e-12f);
    for (int k = 0; k < 4; ++k) a.q[k] = raw_q[k] * a.inv_norm;
    a.opacity = 1.f / (1.f + expf(-logit));
}

GSR_HD void activate_raw_backward(const RawAct &a, GeomGrad &g)
{
    for (int k = 0; k < 3; ++k) g.dscale[k] *= a.scale[k];
    const float dot = a.clamped_norm ? 0.f : a.q[0] * g.drot[0] + a.q[1] * g.drot[1] + a.q[2] * g.drot[2] + a.q[3] * g.drot[3];
    for (int k = 0; k < 4; ++k) g.drot[k] = (g.drot[k] - a.q[k] * dot) * a.inv_norm;
    g.dopacity *= a.opacity * (1.f - a.opacity);
}

// ---- Anti-aliasing as an opacity compensation (the 2D filter of Mip-Splatting, upstream's `antialiasing`).
// The forward low-passes every splat by h = GSR_COV2D_DILATE on the diagonal of its 2D covariance; this factor pays the energy back:
//   det0 = a0 c0 - b^2     det1 = (a0 + h)(c0 + h) - b^2 = det0 + h (a0 + c0) + h^2     (a0, b, c0: the entries BEFORE the dilation h)
//   x = det0 / det1        rho = sqrt(max(GSR_AA_MIN_RATIO, x))        opacity' = opacity rho
// The entries are formed from the 2x3 factor W = T R diag(scale_modifier s) of the 2D covariance W W^T (T of ewa_project: same
// frustum clamp), not as e.a - h and not from Sigma: a0 = |W0|^2, c0 = |W1|^2, b = W0 . W1 are sums without a subtraction, and
//   det0 = m01^2 + m02^2 + m12^2,   m_kl = W0_k W1_l - W0_l W1_k   (Cauchy-Binet)
// is a sum of squares where a0 c0 - b^2 cancels all but one part in (aspect ratio)^2 of its terms: for a needle a hundred times
// longer than wide that is every bit of binary32.  The gradient goes back the same way, through W: to the scales directly, to
// the rotation through dL/dR (quat_to_rot_backward), to means3D through dL/dT (jacobian_chain_backward, view_point_backward).
// A Gaussian the preprocess culls before it has a covariance (A.1), or one with det1 == 0, passes through (rho = 1 exactly).
struct AaFactor {
    float R[9], s[3];           // rotation matrix, scale_modifier * scale
    float u[3], v[3];           // T0 . R[:, k], T1 . R[:, k]:  W0_k = u_k s_k, W1_k = v_k s_k
    float w0[3], w1[3];         // rows of W
    float m01, m02, m12;        // 2x2 minors of W
    float tr, det0, det1, rho;  // tr = a0 + c0
    bool pass, clamped;         // pass: rho = 1, no geometry gradient; clamped: x <= GSR_AA_MIN_RATIO, rho is the constant
};

GSR_HD void aa_factor(const FrameK &f, const float *V, const float p[3], const float *scale, const float *quat, Ewa &e, AaFactor &a)
{
    a.pass = true; a.clamped = false; a.rho = 1.f;
    if (!(view_coord(p, V, 2) > (float)GSR_NEAR_CUT)) return;                   // A.1, as in_frustum below
    ewa_of_gaussian(f, V, p, scale, quat, nullptr, e);
    quat_to_rot(quat, a.R);
    for (int k = 0; k < 3; ++k) {
        a.s[k] = f.scale_modifier * scale[k];
        a.u[k] = e.T[0] * a.R[k] + e.T[1] * a.R[3 + k] + e.T[2] * a.R[6 + k];
        a.v[k] = e.T[3] * a.R[k] + e.T[4] * a.R[3 + k] + e.T[5] * a.R[6 + k];
        a.w0[k] = a.u[k] * a.s[k];
        a.w1[k] = a.v[k] * a.s[k];
    }
    a.m01 = a.w0[0] * a.w1[1] - a.w0[1] * a.w1[0];
    a.m02 = a.w0[0] * a.w1[2] - a.w0[2] * a.w1[0];
    a.m12 = a.w0[1] * a.w1[2] - a.w0[2] * a.w1[1];
    const float h = (float)GSR_COV2D_DILATE;
    a.tr = (a.w0[0] * a.w0[0] + a.w0[1] * a.w0[1] + a.w0[2] * a.w0[2]) + (a.w1[0] * a.w1[0] + a.w1[1] * a.w1[1] + a.w1[2] * a.w1[2]);
    a.det0 = a.m01 * a.m01 + a.m02 * a.m02 + a.m12 * a.m12;
    a.det1 = a.det0 + h * a.tr + h * h;
    if (a.det1 == 0.f) return;
    a.pass = false;
    const float x = a.det0 / a.det1;
    a.clamped = !(x > (float)GSR_AA_MIN_RATIO);
    a.rho = sqrtf(a.clamped ? (float)GSR_AA_MIN_RATIO : x);
}

// scale, quat, opacity: the ACTIVATED values.  logit (raw mode; else null): the opacity's logit; the result is then the logit of
// p' = opacity rho, written as log p' - log(1 - p').
GSR_HD float opacity_compensation_one(const FrameK &f, const float *V, const float p[3], const float *scale, const float *quat,
                                      float opacity, const float *logit)
{
    Ewa e;
    AaFactor a;
    aa_factor(f, V, p, scale, quat, e, a);
    if (a.pass) return logit ? *logit : opacity;
    const float pp = opacity * a.rho;
    return logit ? logf(pp) - log1pf(-pp) : pp;
}

// gin: dL/dopacity' (raw mode: dL/dlogit').  Writes g.dopacity, g.dmean, g.dscale, g.drot: with `act` (raw mode: what activate_raw
// made of this Gaussian) they are the gradients on the logit, the log-scales and the raw quaternion,
//   dlogit'/dlogit = (1 - p) / (1 - p')      dlogit'/drho = 1 / (rho (1 - p'))
// else on the activated values.  As in geom_backward_one, a clamped tx (ty) passes nothing (xmul / ymul) and g.dscale is the
// gradient on scale_modifier * scale (A.10 omits the factor): the two backwards add up on the same tensors.  No camera gradient.
GSR_HD void opacity_compensation_backward_one(const FrameK &f, const float *V, const float p[3], const float *scale, const float *quat,
                                              float opacity, const RawAct *act, float gin, GeomGrad &g)
{
    Ewa e;
    AaFactor a;
    aa_factor(f, V, p, scale, quat, e, a);
    for (int k = 0; k < 3; ++k) { g.dmean[k] = 0.f; g.dscale[k] = 0.f; }
    for (int k = 0; k < 4; ++k) g.drot[k] = 0.f;
    g.dopacity = gin;
    if (a.pass) return;
    float dL_drho;
    if (act) {
        const float inv = 1.f / (1.f - opacity * a.rho);
        g.dopacity = gin * ((1.f - opacity) * inv);
        dL_drho = gin * (inv / a.rho);
    } else {
        g.dopacity = gin * a.rho;
        dL_drho = gin * opacity;
    }
    if (a.clamped) return;
    // x = det0 / (det0 + h tr + h^2):  dx/ddet0 = (det1 - det0) / det1^2 = h (tr + h) / det1^2,  dx/dtr = -h det0 / det1^2
    const float h = (float)GSR_COV2D_DILATE;
    const float k = dL_drho * h / (2.f * a.rho * a.det1 * a.det1);       // dL/dx h / det1^2
    const float kd = 2.f * k * (a.tr + h), kt = -2.f * k * a.det0;       // twice dL/ddet0, dL/dtr: det0 and tr are quadratic in W
    const float dw0[3] = {kd * (a.m01 * a.w1[1] + a.m02 * a.w1[2]) + kt * a.w0[0], kd * (a.m12 * a.w1[2] - a.m01 * a.w1[0]) + kt * a.w0[1],
                          kt * a.w0[2] - kd * (a.m02 * a.w1[0] + a.m12 * a.w1[1])};
    const float dw1[3] = {kt * a.w1[0] - kd * (a.m01 * a.w0[1] + a.m02 * a.w0[2]), kd * (a.m01 * a.w0[0] - a.m12 * a.w0[2]) + kt * a.w1[1],
                          kd * (a.m02 * a.w0[0] + a.m12 * a.w0[1]) + kt * a.w1[2]};
    // W0_k = u_k s_k, u_k = sum_j T0_j R[j][k]
    ScreenChain s;
    float gR[9];
    for (int j = 0; j < 3; ++j) { s.dT0[j] = 0.f; s.dT1[j] = 0.f; }
    for (int c = 0; c < 3; ++c) {
        g.dscale[c] = dw0[c] * a.u[c] + dw1[c] * a.v[c];
        const float du = dw0[c] * a.s[c], dv = dw1[c] * a.s[c];
        for (int j = 0; j < 3; ++j) {
            s.dT0[j] += du * a.R[3 * j + c];
            s.dT1[j] += dv * a.R[3 * j + c];
            gR[3 * j + c] = e.T[j] * du + e.T[3 + j] * dv;
        }
    }
    quat_to_rot_backward(quat, gR, g.drot);
    jacobian_chain_backward(f, V, e, s);
    view_point_backward(V, s, g.dmean);
    if (act) {
        const float keep = g.dopacity;
        activate_raw_backward(*act, g);
        g.dopacity = keep;
    }
}

// ---- The latent structured model's composition (scene/latent_gaussian_model.py forward): child k of structure b is the
// decoder's 11 + 3M floats c added onto / rotated by the structure's own mean, opacity logit, log-scale and rotation.
//   xyz = c[0:3] + s_mean     opacity = c[3] + s_opacity     scaling = c[4:7] + s_scale        (one fp32 add each)
//   rotation = std(n(s_rot) (x) n(c[7:11]))      n(v) = v / max(|v|_2, 1e-12) (a division, as torch.nn.functional.normalize),
//   (x) the Hamilton product, real part first;  std(q) = -q where q_w < 0 (q_w == 0 is not flipped).
// The 3M SH floats behind them are copied, not computed: no function here.
constexpr int kChildGeom = 11;             // floats of a child in front of its SH block; also floats of a structure
constexpr float kQuatNormEps = 1e-12f;

struct QuatNorm { float v[4], n, inv; };   // v / max(n, eps); inv = 1 / max(n, eps)

GSR_HD void quat_normalize(const float q[4], QuatNorm &o)
{
    o.n = sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float nc = fmaxf(o.n, kQuatNormEps);
    o.inv = 1.f / nc;
    for (int k = 0; k < 4; ++k) o.v[k] = q[k] / nc;
}

// d normalize, the rule of k_act_bwd: g / n_c - v (v . g) / (n n_c^2) where n >= eps; below eps the clamp passes nothing and
// only g / eps remains
GSR_HD void quat_normalize_backward(const float q[4], const QuatNorm &o, const float g[4], float d[4])
{
    const float dot = q[0] * g[0] + q[1] * g[1] + q[2] * g[2] + q[3] * g[3];
    const float k = o.n >= kQuatNormEps ? dot * o.inv * o.inv / o.n : 0.f;
    for (int i = 0; i < 4; ++i) d[i] = g[i] * o.inv - q[i] * k;
}

// c: the child's first 11 decoder outputs; s: the structure's (mean[3], opacity, scale[3], rotation[4]) in the same column
// order; out: the child's (xyz[3], opacity, scaling[3], rotation[4])
GSR_HD void compose_child(const float c[kChildGeom], const float s[kChildGeom], float out[kChildGeom])
{
    for (int i = 0; i < 7; ++i) out[i] = c[i] + s[i];
    QuatNorm a, b;
    quat_normalize(s + 7, a);
    quat_normalize(c + 7, b);
    const float *A = a.v, *B = b.v;
    const float w = A[0] * B[0] - A[1] * B[1] - A[2] * B[2] - A[3] * B[3];
    const float x = A[0] * B[1] + A[1] * B[0] + A[2] * B[3] - A[3] * B[2];
    const float y = A[0] * B[2] - A[1] * B[3] + A[2] * B[0] + A[3] * B[1];
    const float z = A[0] * B[3] + A[1] * B[2] - A[2] * B[1] + A[3] * B[0];
    const bool flip = w < 0.f;
    out[7] = flip ? -w : w; out[8] = flip ? -x : x; out[9] = flip ? -y : y; out[10] = flip ? -z : z;
}

// g: dL/d out of compose_child.  d_c: dL/d c.  d_s: THIS child's term of dL/d s (the caller sums a structure's children).
// Recomputes the two normalisations and the product's sign from c and s: the forward keeps nothing.
GSR_HD void compose_child_backward(const float c[kChildGeom], const float s[kChildGeom], const float g[kChildGeom],
                                   float d_c[kChildGeom], float d_s[kChildGeom])
{
    for (int i = 0; i < 7; ++i) { d_c[i] = g[i]; d_s[i] = g[i]; }
    QuatNorm a, b;
    quat_normalize(s + 7, a);
    quat_normalize(c + 7, b);
    const float *A = a.v, *B = b.v;
    const float w = A[0] * B[0] - A[1] * B[1] - A[2] * B[2] - A[3] * B[3];
    const float sg = w < 0.f ? -1.f : 1.f;
    const float gw = sg * g[7], gx = sg * g[8], gy = sg * g[9], gz = sg * g[10];
    const float dA[4] = {gw * B[0] + gx * B[1] + gy * B[2] + gz * B[3], -gw * B[1] + gx * B[0] - gy * B[3] + gz * B[2],
                         -gw * B[2] + gx * B[3] + gy * B[0] - gz * B[1], -gw * B[3] - gx * B[2] + gy * B[1] + gz * B[0]};
    const float dB[4] = {gw * A[0] + gx * A[1] + gy * A[2] + gz * A[3], -gw * A[1] + gx * A[0] + gy * A[3] - gz * A[2],
                         -gw * A[2] - gx * A[3] + gy * A[0] + gz * A[1], -gw * A[3] + gx * A[2] - gy * A[1] + gz * A[0]};
    quat_normalize_backward(s + 7, a, dA, d_s + 7);
    quat_normalize_backward(c + 7, b, dB, d_c + 7);
}

// ---- The MCMC densification strategy ("3D Gaussian Splatting as Markov Chain Monte Carlo"): the arithmetic of
// one Gaussian for the relocation rule, the position noise and the regulariser gradient (kernels: gsr_mcmc.hip).
//
// Relocation: a source of opacity o and scale s that stands for N Gaussians afterwards (N = 1 + the times it was sampled, clamped to
// 1 .. GSR_MCMC_MAX_RATIO) becomes
//   o' = 1 - (1 - o)^(1/N)      D = sum_{i=1..N} sum_{k=0..i-1} C(i-1, k) (-1)^k (k+1)^(-1/2) o'^(k+1)      s' = (o / D) s
//   opacity_raw' = logit(clamp(o', min_opacity, 1 - 2^-23))        scaling_raw' = scaling_raw + log(o / D)
// The inner sums over i collapse (sum_{i=k+1..N} C(i-1, k) = C(N, k+1)): D = sum_{j=1..N} C(N, j) (-1)^(j-1) j^(-1/2) o'^j, with
// C(N, j) = C(N, j-1) (N-j+1) / j exact in binary64 (every product stays below 2^53 for N <= 51).  The sum alternates and cancels:
// everything here is binary64 (o and 1 - o as the two sigmoids, o' through expm1 of log(1 - o) / N, so that a small o loses
// nothing), rounded to binary32 once at the end.  N = 1 is the identity: the inputs are returned as they are.
GSR_HD void mcmc_relocation_one(float opacity_raw, const float scaling_raw[3], int N, float min_opacity, float &new_opacity_raw,
                                float new_scaling_raw[3])
{
    if (N <= 1) {
        new_opacity_raw = opacity_raw;
        for (int k = 0; k < 3; ++k) new_scaling_raw[k] = scaling_raw[k];
        return;
    }
    if (N > GSR_MCMC_MAX_RATIO) N = GSR_MCMC_MAX_RATIO;
    const double x = (double)opacity_raw;
    const double o = 1.0 / (1.0 + exp(-x)), om = 1.0 / (1.0 + exp(x));       // o, 1 - o
    const double log_om1 = log(om) / (double)N;                              // log(1 - o')
    const double o1 = -expm1(log_om1);                                       // o'
    double D = 0.0, c = 1.0, pw = 1.0;
    for (int j = 1; j <= N; ++j) {
        c = c * (double)(N - j + 1) / (double)j;                             // C(N, j)
        pw *= o1;
        const double term = c * pw / sqrt((double)j);
        D += (j & 1) ? term : -term;
    }
    const double lo = (double)min_opacity, hi = 1.0 - 1.1920928955078125e-07;
    const double logit = o1 < lo ? log(lo) - log1p(-lo) : (o1 > hi ? log(hi) - log1p(-hi) : log(o1) - log_om1);
    new_opacity_raw = (float)logit;
    const double shift = log(o / D);
    for (int k = 0; k < 3; ++k) new_scaling_raw[k] = (float)((double)scaling_raw[k] + shift);
}

// Position noise: delta = R(q^) diag(s^2) R(q^)^T (xi g(o) c),   g(o) = 1 / (1 + exp(100 o - 0.5)),   q^ = q / max(|q|, 1e-12),
// s = exp(log_scale), o = sigmoid(logit).  exp may overflow to +inf for o near 1: g is then 0 and the delta exactly zero (a zero g
// returns before anything is multiplied by it, so that no 0 * inf can form).
GSR_HD void mcmc_noise_one(const float log_scale[3], const float raw_q[4], float logit, const float xi[3], float c, float delta[3])
{
    const float o = 1.f / (1.f + expf(-logit));
    const float g = 1.f / (1.f + expf(100.f * o - 0.5f));
    delta[0] = delta[1] = delta[2] = 0.f;
    if (!(g > 0.f)) return;
    const float n = sqrtf(raw_q[0] * raw_q[0] + raw_q[1] * raw_q[1] + raw_q[2] * raw_q[2] + raw_q[3] * raw_q[3]);
    const float nc = fmaxf(n, 1e-12f);
    const float q[4] = {raw_q[0] / nc, raw_q[1] / nc, raw_q[2] / nc, raw_q[3] / nc};
    float R[9];
    quat_to_rot(q, R);
    const float gc = g * c;
    const float w[3] = {xi[0] * gc, xi[1] * gc, xi[2] * gc};
    float v[3];
    for (int k = 0; k < 3; ++k) {                                            // v = diag(s^2) R^T w
        const float s = expf(log_scale[k]);
        v[k] = (R[k] * w[0] + R[3 + k] * w[1] + R[6 + k] * w[2]) * (s * s);
    }
    for (int k = 0; k < 3; ++k) delta[k] = R[3 * k] * v[0] + R[3 * k + 1] * v[1] + R[3 * k + 2] * v[2];
}

// Regulariser gradient: d/d opacity_raw of k_o o = k_o o (1 - o), d/d scaling_raw of k_s s = k_s s (k_o = lambda_o / P,
// k_s = lambda_s / (3 P): the gradients of lambda_o mean(o) + lambda_s mean(s)).  o (1 - o) = e / (1 + e)^2 with e = exp(-|x|):
// no subtraction from 1 and no overflow for any logit.
GSR_HD float mcmc_reg_opacity_one(float logit, float k_o)
{
    const float e = expf(-fabsf(logit)), d = 1.f + e;
    return k_o * (e / (d * d));
}
GSR_HD float mcmc_reg_scale_one(float log_scale, float k_s) { return k_s * expf(log_scale); }
GSR_HD void mcmc_reg_one(float logit, const float log_scale[3], float k_o, float k_s, float &d_opacity, float d_scaling[3])
{
    d_opacity = mcmc_reg_opacity_one(logit, k_o);
    for (int k = 0; k < 3; ++k) d_scaling[k] = mcmc_reg_scale_one(log_scale[k], k_s);
}

// ---- the Adam update of one element (torch.optim.Adam without weight decay or amsgrad), the one statement of the rule:
// every path of the dense and the sparse step (gsr_optim.hip: float4 bodies and trailing elements) calls it.
//   m' = m + (g - m)(1 - b1);  v' = b2 v + (1 - b2) g^2;  p' = p - step (m' / (sqrt(v') inv_bc2_sqrt + eps))
// with step = lr / (1 - b1^t) and inv_bc2_sqrt = 1 / sqrt(1 - b2^t) from the host.  Every multiply-add is an explicit fmaf, so no
// contraction is left to a compiler and the bits are the same under any -ffp-contract and on the host.  v' rounds v b2 and fuses the
// other product; m' and p' have one product each.
struct AdamConsts { float one_minus_b1, b2, one_minus_b2, eps; };

GSR_HD void adam_update(float &p, float &m, float &v, float g, float step, float inv_bc2_sqrt, const AdamConsts &c)
{
    m = fmaf(g - m, c.one_minus_b1, m);
    v = fmaf(c.one_minus_b2 * g, g, v * c.b2);
    p = fmaf(-step, m / fmaf(sqrtf(v), inv_bc2_sqrt, c.eps), p);
}

// The step size of column c of a row of w floats whose first `split` step with `head` and the others with `tail`.  c may lie in a
// following row: in the next one at most if `wide` (the four columns under a float4 when w >= 3), in any otherwise.
GSR_HD float adam_step_size(uint32_t c, uint32_t w, uint32_t split, float head, float tail, bool wide)
{
    c = wide ? (c >= w ? c - w : c) : c % w;
    return c < split ? head : tail;
}

// ---- A.1 alone (markVisible).
GSR_HD bool in_frustum(const float p[3], const float *V)
{
    return view_coord(p, V, 2) > (float)GSR_NEAR_CUT;
}

}  // namespace gsr
