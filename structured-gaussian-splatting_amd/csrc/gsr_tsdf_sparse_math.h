// gsr_tsdf_sparse_math.h — the sparse TSDF volume, per element, as GSR_HD inline functions in the manner of
// gsr_tsdf_math.h: the kernels of gsr_tsdf.hip call them on the device, tests/tsdf_sparse_host.cpp compiles the same text with g++.
//
// Bricks.  The virtual grid of nx ny nz voxels is cut into bricks of 8 x 8 x 8: brick (bx, by, bz) holds the voxels 8 bx .. 8 bx + 7
// along x and likewise along y and z; the grid's dimensions need not be multiples of 8 (a voxel beyond them is never touched).  Bricks
// are numbered x fastest (the brick table's order), a brick's voxels [z, y, x] (local index 64 lz + 8 ly + lx).
//
// Marking.  One pixel of a frame marks the bricks its depth can reach: the frustum piece of the pixel's footprint [px, px + 1] x
// [py, py + 1] between the view depths max(d - trunc, 0) and d + trunc, d = depth / alpha, holds every voxel centre that the fusion
// rule gives a sample |s| < trunc from this pixel.  Its eight corners go to world space through the inverse view matrix, then to
// voxel-index coordinates; their axis-aligned box grown by `pad` voxels holds every voxel within Chebyshev distance 1 of such a
// centre once pad >= 1 (plus the rounding of this binary32 evaluation, for which the callers demand pad >= 1.25).  Every multiply-add
// pair is an explicit fmaf.
#pragma once

#include "gsr_tsdf_math.h"

namespace gsr {

constexpr int kBrickSide = 8, kBrickShift = 3, kBrickVoxels = 512;

struct BrickDims { int nbx, nby, nbz; };

GSR_HD BrickDims brick_dims(int nx, int ny, int nz)
{
    BrickDims b;
    b.nbx = (nx + kBrickSide - 1) >> kBrickShift; b.nby = (ny + kBrickSide - 1) >> kBrickShift; b.nbz = (nz + kBrickSide - 1) >> kBrickShift;
    return b;
}

GSR_HD size_t brick_linear(const BrickDims &b, int bx, int by, int bz) { return ((size_t)bz * (size_t)b.nby + (size_t)by) * (size_t)b.nbx + (size_t)bx; }

// (e < 2^31: the brick table's limit)
GSR_HD void brick_of_linear(const BrickDims &b, size_t e, int &bx, int &by, int &bz)
{
    const uint32_t row = (uint32_t)e / (uint32_t)b.nbx;
    bx = (int)((uint32_t)e - row * (uint32_t)b.nbx); by = (int)(row % (uint32_t)b.nby); bz = (int)(row / (uint32_t)b.nby);
}

GSR_HD int brick_local(int x, int y, int z) { return ((z & 7) << 6) | ((y & 7) << 3) | (x & 7); }

// voxel l (0 .. 511) of brick (bx, by, bz) -> its grid coordinates
GSR_HD void brick_voxel(int bx, int by, int bz, int l, int &x, int &y, int &z)
{
    x = (bx << kBrickShift) + (l & 7); y = (by << kBrickShift) + ((l >> 3) & 7); z = (bz << kBrickShift) + (l >> 6);
}

struct BrickBox { int lo[3], hi[3]; };               // bricks lo .. hi (inclusive) along x, y, z

// The bricks pixel (px, py) marks; false: none (an invalid pixel by tsdf_sample's first two tests, or a box that misses the grid).
// Vinv: the inverse of the view matrix's affine part [4,4] row-major (p_world = p_view Vinv[:3,:3] + Vinv[3,:3]).
GSR_HD bool brick_mark_box(const TsdfGrid &g, const TsdfFrame &f, const float *Vinv, int px, int py, float depth, float alpha, float pad,
                           BrickBox &box)
{
    if (!(alpha >= f.alpha_min && depth > 0.f)) return false;
    const float d = depth / alpha;
    if (d > f.depth_max) return false;
    const float zs[2] = {fmaxf(d - g.trunc, 0.f), d + g.trunc};
    const float xs[2] = {((float)px - f.cx) / f.fx, ((float)(px + 1) - f.cx) / f.fx};
    const float ys[2] = {((float)py - f.cy) / f.fy, ((float)(py + 1) - f.cy) / f.fy};
    const float o[3] = {g.ox, g.oy, g.oz};
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int k = 0; k < 8; ++k) {
        const float z = zs[k >> 2], x = xs[k & 1] * z, y = ys[(k >> 1) & 1] * z;
        for (int j = 0; j < 3; ++j) {
            const float w = fmaf(x, Vinv[j], fmaf(y, Vinv[4 + j], fmaf(z, Vinv[8 + j], Vinv[12 + j])));
            const float v = (w - o[j]) / g.voxel;
            lo[j] = fminf(lo[j], v); hi[j] = fmaxf(hi[j], v);               // (a NaN is dropped by fminf and fmaxf: an empty box below)
        }
    }
    const int n[3] = {g.nx, g.ny, g.nz};
    for (int j = 0; j < 3; ++j) {
        // the integer voxel coordinates inside [lo - pad, hi + pad], cut to the grid; the comparison refuses an empty range and a NaN
        const float a = fmaxf(ceilf(lo[j] - pad), 0.f), b = fminf(floorf(hi[j] + pad), (float)(n[j] - 1));
        if (!(a <= b)) return false;
        box.lo[j] = (int)a >> kBrickShift; box.hi[j] = (int)b >> kBrickShift;
    }
    return true;
}

}  // namespace gsr
