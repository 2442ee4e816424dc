// tsdf_sparse_host.cpp — the per-element functions of csrc/gsr_tsdf_sparse_math.h that the sparse kernels of csrc/gsr_tsdf.hip call,
// run on the host so that they can be held to the binary64 restatement of tests/test_tsdf_sparse_ref.py and run under the address and
// undefined-behaviour sanitizers (that test builds this file with them).  Every array is a heap allocation of exactly its size, an
// image one per row: a mark one brick past the table, or a read one pixel past a row, stops the program.
//
//   tsdf_sparse_host marks in out   in:  int32 nx, ny, nz, frames; float origin[3], voxel, trunc, pad; per frame: int32 H, W; float
//                                        tanfovx, tanfovy, alpha_min, depth_max; Vinv [16]; depth, alpha [H,W]
//                                   out: per frame, uint8 marks [nbz,nby,nbx] (that frame's alone)
//   tsdf_sparse_host index nx ny nz      the brick arithmetic on every voxel of the grid: voxel -> (brick, local) -> voxel, brick ->
//                                        linear index -> brick, the linear indices ascending x fastest; exit status 0 when all agree
#include <stdio.h>
#include <stdlib.h>

#include <memory>
#include <vector>

#include "../structured-gaussian-splatting_amd/csrc/gsr_tsdf_sparse_math.h"

using namespace gsr;

struct Image {                                       // [H][W] floats, a heap allocation per row
    std::vector<std::unique_ptr<float[]>> rows;
    Image(int H, int W, FILE *f)
    {
        for (int r = 0; r < H; ++r) {
            rows.emplace_back(new float[(size_t)W]);
            if (W && fread(rows.back().get(), sizeof(float), (size_t)W, f) != (size_t)W) exit(4);
        }
    }
    float at(int y, int x) const { return rows[(size_t)y][(size_t)x]; }
};

static int run_marks(FILE *in, FILE *out)
{
    int32_t hdr[4];
    float gp[6];
    if (fread(hdr, sizeof(int32_t), 4, in) != 4 || fread(gp, sizeof(float), 6, in) != 6) return 4;
    const TsdfGrid g{hdr[0], hdr[1], hdr[2], gp[0], gp[1], gp[2], gp[3], gp[4]};
    const float pad = gp[5];
    const BrickDims bd = brick_dims(g.nx, g.ny, g.nz);
    const size_t ne = (size_t)bd.nbx * bd.nby * bd.nbz;
    for (int fr = 0; fr < hdr[3]; ++fr) {
        int32_t hw[2];
        float par[4], Vinv[16];
        if (fread(hw, sizeof(int32_t), 2, in) != 2 || fread(par, sizeof(float), 4, in) != 4 || fread(Vinv, sizeof(float), 16, in) != 16) return 4;
        const int H = hw[0], W = hw[1];
        const TsdfFrame f = tsdf_frame(H, W, par[0], par[1], par[2], par[3]);
        const Image depth(H, W, in), alpha(H, W, in);
        std::unique_ptr<unsigned char[]> marks(new unsigned char[ne]);
        for (size_t e = 0; e < ne; ++e) marks[e] = 0;
        for (int py = 0; py < H; ++py)
            for (int px = 0; px < W; ++px) {
                BrickBox box;
                if (!brick_mark_box(g, f, Vinv, px, py, depth.at(py, px), alpha.at(py, px), pad, box)) continue;
                for (int bz = box.lo[2]; bz <= box.hi[2]; ++bz)
                    for (int by = box.lo[1]; by <= box.hi[1]; ++by)
                        for (int bx = box.lo[0]; bx <= box.hi[0]; ++bx) marks[brick_linear(bd, bx, by, bz)] = 1;
            }
        fwrite(marks.get(), 1, ne, out);
    }
    return 0;
}

static int run_index(int nx, int ny, int nz)
{
    const BrickDims bd = brick_dims(nx, ny, nz);
    if (bd.nbx != (nx + 7) / 8 || bd.nby != (ny + 7) / 8 || bd.nbz != (nz + 7) / 8) return 1;
    size_t expect = 0;
    for (int bz = 0; bz < bd.nbz; ++bz)
        for (int by = 0; by < bd.nby; ++by)
            for (int bx = 0; bx < bd.nbx; ++bx, ++expect) {
                const size_t e = brick_linear(bd, bx, by, bz);
                int x, y, z;
                brick_of_linear(bd, e, x, y, z);
                if (e != expect || x != bx || y != by || z != bz) return 2;
            }
    std::vector<unsigned char> seen((size_t)kBrickVoxels);
    for (int iz = 0; iz < nz; ++iz)
        for (int iy = 0; iy < ny; ++iy)
            for (int ix = 0; ix < nx; ++ix) {
                const int l = brick_local(ix, iy, iz);
                int x, y, z;
                brick_voxel(ix >> kBrickShift, iy >> kBrickShift, iz >> kBrickShift, l, x, y, z);
                if (l < 0 || l >= kBrickVoxels || x != ix || y != iy || z != iz || l != (iz % 8) * 64 + (iy % 8) * 8 + ix % 8) return 3;
                seen[(size_t)l] = 1;
            }
    printf("index ok: %d x %d x %d voxels in %d x %d x %d bricks\n", nx, ny, nz, bd.nbx, bd.nby, bd.nbz);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && argv[1][0] == 'i') return run_index(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
    if (argc != 4 || argv[1][0] != 'm') { fprintf(stderr, "usage: tsdf_sparse_host marks in out | index nx ny nz\n"); return 2; }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    const int rc = run_marks(in, out);
    fclose(in); fclose(out);
    return rc;
}
