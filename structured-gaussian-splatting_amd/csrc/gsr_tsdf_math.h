// gsr_tsdf_math.h — TSDF fusion and surface nets, per element, written once as GSR_HD inline functions: the kernels
// of gsr_tsdf.hip call them on the device, tests/tsdf_host.cpp compiles the same text with g++.
//
// Fusion (KinectFusion's projective rule with free-space carving, restated from the literature): the centre of voxel (ix, iy, iz) is
// origin + voxel (ix, iy, iz); it is taken to the view space (row-vector convention, p_view = p V[:3,:3] + V[3,:3]), projected to the
// pixel that holds it, and - where that pixel has a depth d = depth / alpha with d - z > -trunc - the clamped signed distance
// t = min(1, (d - z) / trunc) enters the voxel's running mean.  Every multiply-add pair is an explicit fmaf, so the host and the
// device round alike whatever the compiler would contract.
//
// Surface nets: a voxel is observed when weight >= min_weight and inside when tsdf < 0.  An accessor `at(x, y, z, f)` answers whether
// the voxel is observed and hands out its tsdf; it is never asked about a voxel outside the volume.
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

struct TsdfGrid { int nx, ny, nz; float ox, oy, oz, voxel, trunc; };
struct TsdfFrame { int H, W; float fx, fy, cx, cy, alpha_min, depth_max; };

GSR_HD TsdfFrame tsdf_frame(int H, int W, float tanfovx, float tanfovy, float alpha_min, float depth_max)
{
    TsdfFrame f;
    f.H = H; f.W = W;
    f.fx = (float)W / (2.f * tanfovx); f.fy = (float)H / (2.f * tanfovy);
    f.cx = 0.5f * (float)W; f.cy = 0.5f * (float)H;
    f.alpha_min = alpha_min; f.depth_max = depth_max;
    return f;
}

// ---- fusion ---------------------------------------------------------------------------------------------------------------------

// Steps 1 and 2 of the rule: the voxel's view depth z and the pixel (px, py) that holds its projection; false: the voxel is skipped.
// V: the view matrix [4,4] row-major (columns 0..2 are read)
GSR_HD bool tsdf_project(const TsdfGrid &g, const TsdfFrame &f, const float *V, int ix, int iy, int iz, int &px, int &py, float &z)
{
    const float wx = fmaf(g.voxel, (float)ix, g.ox), wy = fmaf(g.voxel, (float)iy, g.oy), wz = fmaf(g.voxel, (float)iz, g.oz);
    z = fmaf(wx, V[2], fmaf(wy, V[6], fmaf(wz, V[10], V[14])));
    if (!(z > 0.f)) return false;
    const float x = fmaf(wx, V[0], fmaf(wy, V[4], fmaf(wz, V[8], V[12])));
    const float y = fmaf(wx, V[1], fmaf(wy, V[5], fmaf(wz, V[9], V[13])));
    const float u = (f.fx * x) / z + f.cx, v = (f.fy * y) / z + f.cy;
    if (!(u >= 0.f) || !(u < (float)f.W) || !(v >= 0.f) || !(v < (float)f.H)) return false;      // (a NaN fails the first of each pair)
    px = (int)floorf(u); py = (int)floorf(v);
    return true;
}

// Steps 3 to 5: the sample t of a voxel at view depth z from its pixel's depth and alpha; false: the voxel is skipped
GSR_HD bool tsdf_sample(const TsdfFrame &f, float trunc, float depth, float alpha, float z, float &t)
{
    if (!(alpha >= f.alpha_min && depth > 0.f)) return false;
    const float d = depth / alpha;
    if (d > f.depth_max) return false;
    const float s = d - z;
    if (!(s > -trunc)) return false;
    t = fminf(1.f, s / trunc);
    return true;
}

// the running mean of w old samples and a new one
GSR_HD float tsdf_mean(float old, float w, float sample) { return fmaf(old, w, sample) / (w + 1.f); }

// ---- surface nets ---------------------------------------------------------------------------------------------------------------

struct SnDims { int nx, ny, nz; };

constexpr unsigned kSnVertex = 8u;            // sn_classify: bit a (0..2) = the edge to the next voxel along axis a emits a quad

GSR_HD int sn_corner_x(int k) { return k & 1; }
GSR_HD int sn_corner_y(int k) { return (k >> 1) & 1; }
GSR_HD int sn_corner_z(int k) { return k >> 2; }

// What voxel (ix, iy, iz) owns.  kSnVertex: the cell whose lowest corner it is exists and is active (8 observed corners, both signs).
// Bit a: the edge from the voxel to its next neighbour along axis a joins two observed voxels of different sign and its four
// adjacent cells exist and are active - they hold the edge, so they have both signs, and are active when the 2 x 3 x 3 voxels around
// the edge are observed.
template <class At>
GSR_HD unsigned sn_classify(const SnDims &d, int ix, int iy, int iz, const At &at)
{
    float f0;
    if (!at(ix, iy, iz, f0)) return 0u;
    const bool in0 = f0 < 0.f;
    unsigned out = 0u;
    if (ix + 1 < d.nx && iy + 1 < d.ny && iz + 1 < d.nz) {
        bool all = true, any_in = in0, any_out = !in0;
        for (int k = 1; k < 8 && all; ++k) {
            float f;
            if (!at(ix + sn_corner_x(k), iy + sn_corner_y(k), iz + sn_corner_z(k), f)) all = false;
            else if (f < 0.f) any_in = true;
            else any_out = true;
        }
        if (all && any_in && any_out) out |= kSnVertex;
    }
    const int p[3] = {ix, iy, iz}, n[3] = {d.nx, d.ny, d.nz};
    for (int a = 0; a < 3; ++a) {
        const int b = (a + 1) % 3, c = (a + 2) % 3;
        if (p[a] + 1 >= n[a] || p[b] < 1 || p[b] + 1 >= n[b] || p[c] < 1 || p[c] + 1 >= n[c]) continue;
        int q[3] = {ix, iy, iz};
        q[a] += 1;
        float f1;
        if (!at(q[0], q[1], q[2], f1) || (f1 < 0.f) == in0) continue;
        bool all = true;
        for (int da = 0; da < 2 && all; ++da)
            for (int db = -1; db < 2 && all; ++db)
                for (int dc = -1; dc < 2 && all; ++dc) {
                    int r[3];
                    r[a] = p[a] + da; r[b] = p[b] + db; r[c] = p[c] + dc;
                    float f;
                    if (!at(r[0], r[1], r[2], f)) all = false;
                }
        if (all) out |= 1u << a;
    }
    return out;
}

// The four cells around the edge from voxel (ix, iy, iz) along axis a, by their lowest corners, counter-clockwise seen against the
// axis ((b, c) the two axes after a, cyclically: e_b x e_c = e_a): (-b -c), (-c), (the voxel's own), (-b)
GSR_HD void sn_quad_cells(int a, int ix, int iy, int iz, int cells[4][3])
{
    const int b = (a + 1) % 3, c = (a + 2) % 3;
    const int off[4][2] = {{-1, -1}, {0, -1}, {0, 0}, {-1, 0}};
    for (int k = 0; k < 4; ++k) {
        cells[k][0] = ix; cells[k][1] = iy; cells[k][2] = iz;
        cells[k][b] += off[k][0]; cells[k][c] += off[k][1];
    }
}

// The quad (v[0..3] the vertices of sn_quad_cells' cells) as two triangles split along v0 - v2, wound so that the normal points from
// the inside voxel to the outside one: along +a when the voxel itself is inside
GSR_HD void sn_quad_faces(const int32_t v[4], bool voxel_inside, int32_t tri[6])
{
    tri[0] = v[0]; tri[3] = v[0];
    if (voxel_inside) { tri[1] = v[1]; tri[2] = v[2]; tri[4] = v[2]; tri[5] = v[3]; }
    else { tri[1] = v[2]; tri[2] = v[1]; tri[4] = v[3]; tri[5] = v[2]; }
}

// The vertex of the active cell whose lowest corner is voxel (ix, iy, iz): the mean of the crossing points a + (b - a) f_a / (f_a - f_b)
// of its sign-changing edges, taken in a fixed order (x edges, then y, then z, each by ascending corner index k = x + 2 y + 4 z of its
// lower end), and the mean of the same interpolation of the corners' colours.  col(x, y, z, c): channel c of the voxel's colour.
template <class At, class Col>
GSR_HD void sn_vertex(const TsdfGrid &g, int ix, int iy, int iz, const At &at, const Col &col, float pos[3], float rgb[3])
{
    float f[8];
    for (int k = 0; k < 8; ++k) at(ix + sn_corner_x(k), iy + sn_corner_y(k), iz + sn_corner_z(k), f[k]);
    float acc[3] = {0.f, 0.f, 0.f}, cacc[3] = {0.f, 0.f, 0.f};
    int n = 0;
    for (int a = 0; a < 3; ++a)
        for (int ka = 0; ka < 8; ++ka) {
            if (ka & (1 << a)) continue;
            const int kb = ka | (1 << a);
            if ((f[ka] < 0.f) == (f[kb] < 0.f)) continue;
            const float t = f[ka] / (f[ka] - f[kb]);
            float p[3] = {(float)sn_corner_x(ka), (float)sn_corner_y(ka), (float)sn_corner_z(ka)};
            p[a] = t;
            for (int j = 0; j < 3; ++j) acc[j] += p[j];
            for (int c = 0; c < 3; ++c) {
                const float ca = col(ix + sn_corner_x(ka), iy + sn_corner_y(ka), iz + sn_corner_z(ka), c);
                const float cb = col(ix + sn_corner_x(kb), iy + sn_corner_y(kb), iz + sn_corner_z(kb), c);
                cacc[c] += fmaf(cb - ca, t, ca);
            }
            ++n;
        }
    const float inv = 1.f / (float)n;
    const float base[3] = {(float)ix, (float)iy, (float)iz}, o[3] = {g.ox, g.oy, g.oz};
    for (int j = 0; j < 3; ++j) pos[j] = fmaf(g.voxel, fmaf(acc[j], inv, base[j]), o[j]);
    for (int c = 0; c < 3; ++c) rgb[c] = cacc[c] * inv;
}

}  // namespace gsr
