// tsdf_host.cpp — the per-element functions of csrc/gsr_tsdf_math.h that the kernels of csrc/gsr_tsdf.hip call, run on the host over
// whole cases so that they can be held to the binary64 restatement (tests/tsdf_ref.py) and run under the address and
// undefined-behaviour sanitizers (tests/test_tsdf_ref.py builds this file with them).  Every array is a heap allocation of exactly its
// size; a volume is one allocation per ROW of x, and an image one per row: a stencil that reads one voxel past a row, or a projection
// that lands one pixel past the image, stops the program.
//
//   tsdf_host fuse in out     in:  int32 nx, ny, nz, frames; float origin[3], voxel, trunc; per frame: int32 H, W; float tanfovx, tanfovy,
//                                  alpha_min, depth_max; V [16]; depth, alpha [H,W]; color [3,H,W]
//                             out: tsdf, weight [nz,ny,nx]; color [3,nz,ny,nx]
//   tsdf_host mesh in out     in:  int32 nx, ny, nz; float origin[3], voxel, min_weight; tsdf, weight [nz,ny,nx]; color [3,nz,ny,nx]
//                             out: int32 V, F; vertices [V,3]; colors [V,3]; faces [F,3] int32
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../structured-gaussian-splatting_amd/csrc/gsr_tsdf_math.h"

using namespace gsr;

struct Rows {                                        // [rows][len] floats, a heap allocation per row
    size_t n, len;
    std::vector<std::unique_ptr<float[]>> rows;
    Rows(size_t n_, size_t len_) : n(n_), len(len_)
    {
        for (size_t r = 0; r < n; ++r) {
            rows.emplace_back(new float[len]);
            for (size_t i = 0; i < len; ++i) rows.back()[i] = 0.f;
        }
    }
    float &at(size_t r, size_t i) { return rows[r][i]; }
    float at(size_t r, size_t i) const { return rows[r][i]; }
    void read(FILE *f) { for (auto &r : rows) if (len && fread(r.get(), sizeof(float), len, f) != len) exit(4); }
    void write(FILE *f) const { for (auto &r : rows) fwrite(r.get(), sizeof(float), len, f); }
};

struct Volume {
    int nx, ny, nz;
    Rows tsdf, weight;
    std::vector<Rows> color;
    Volume(int x, int y, int z) : nx(x), ny(y), nz(z), tsdf((size_t)y * z, (size_t)x), weight((size_t)y * z, (size_t)x)
    {
        for (int c = 0; c < 3; ++c) color.emplace_back((size_t)y * z, (size_t)x);
    }
    size_t row(int y, int z) const { return (size_t)z * ny + y; }
};

static int run_fuse(FILE *in, FILE *out)
{
    int32_t hdr[4];
    float gp[5];
    if (fread(hdr, sizeof(int32_t), 4, in) != 4 || fread(gp, sizeof(float), 5, in) != 5) return 4;
    const TsdfGrid g{hdr[0], hdr[1], hdr[2], gp[0], gp[1], gp[2], gp[3], gp[4]};
    Volume vol(g.nx, g.ny, g.nz);
    for (int fr = 0; fr < hdr[3]; ++fr) {
        int32_t hw[2];
        float par[4], V[16];
        if (fread(hw, sizeof(int32_t), 2, in) != 2 || fread(par, sizeof(float), 4, in) != 4 || fread(V, sizeof(float), 16, in) != 16) return 4;
        const int H = hw[0], W = hw[1];
        const TsdfFrame f = tsdf_frame(H, W, par[0], par[1], par[2], par[3]);
        Rows depth((size_t)H, (size_t)W), alpha((size_t)H, (size_t)W);
        std::vector<Rows> image;
        depth.read(in); alpha.read(in);
        for (int c = 0; c < 3; ++c) { image.emplace_back((size_t)H, (size_t)W); image.back().read(in); }
        for (int iz = 0; iz < g.nz; ++iz)
            for (int iy = 0; iy < g.ny; ++iy)
                for (int ix = 0; ix < g.nx; ++ix) {
                    int px, py;
                    float z, t;
                    if (!tsdf_project(g, f, V, ix, iy, iz, px, py, z)) continue;
                    if (!tsdf_sample(f, g.trunc, depth.at((size_t)py, (size_t)px), alpha.at((size_t)py, (size_t)px), z, t)) continue;
                    const size_t r = vol.row(iy, iz);
                    const float w = vol.weight.at(r, (size_t)ix);
                    vol.tsdf.at(r, (size_t)ix) = tsdf_mean(vol.tsdf.at(r, (size_t)ix), w, t);
                    for (int c = 0; c < 3; ++c)
                        vol.color[(size_t)c].at(r, (size_t)ix) = tsdf_mean(vol.color[(size_t)c].at(r, (size_t)ix), w, image[(size_t)c].at((size_t)py, (size_t)px));
                    vol.weight.at(r, (size_t)ix) = w + 1.f;
                }
    }
    vol.tsdf.write(out); vol.weight.write(out);
    for (auto &c : vol.color) c.write(out);
    return 0;
}

struct At {                                          // the accessors of gsr_tsdf_math.h over the whole volume
    const Volume &v; float min_weight;
    bool operator()(int x, int y, int z, float &f) const
    {
        if (x < 0 || y < 0 || z < 0 || x >= v.nx || y >= v.ny || z >= v.nz) abort();      // never asked about a voxel outside
        f = v.tsdf.at(v.row(y, z), (size_t)x);
        return v.weight.at(v.row(y, z), (size_t)x) >= min_weight;
    }
};
struct Col {
    const Volume &v;
    float operator()(int x, int y, int z, int c) const { return v.color[(size_t)c].at(v.row(y, z), (size_t)x); }
};

static int run_mesh(FILE *in, FILE *out)
{
    int32_t dims[3];
    float gp[5];
    if (fread(dims, sizeof(int32_t), 3, in) != 3 || fread(gp, sizeof(float), 5, in) != 5) return 4;
    const TsdfGrid g{dims[0], dims[1], dims[2], gp[0], gp[1], gp[2], gp[3], 0.f};
    const SnDims d{g.nx, g.ny, g.nz};
    Volume vol(g.nx, g.ny, g.nz);
    vol.tsdf.read(in); vol.weight.read(in);
    for (auto &c : vol.color) c.read(in);
    const At at{vol, gp[4]};
    const Col col{vol};
    const size_t n = (size_t)g.nx * g.ny * g.nz;
    std::vector<unsigned> own(n, 0u);
    std::vector<int32_t> vid(n, -1);
    std::vector<float> vertices, colors;
    std::vector<int32_t> faces;
    if (g.nx >= 2 && g.ny >= 2 && g.nz >= 2) {
        int32_t nv = 0;
        size_t i = 0;
        for (int iz = 0; iz < g.nz; ++iz)
            for (int iy = 0; iy < g.ny; ++iy)
                for (int ix = 0; ix < g.nx; ++ix, ++i) {
                    own[i] = sn_classify(d, ix, iy, iz, at);
                    if (!(own[i] & kSnVertex)) continue;
                    float pos[3], rgb[3];
                    sn_vertex(g, ix, iy, iz, at, col, pos, rgb);
                    vid[i] = nv++;
                    for (int j = 0; j < 3; ++j) { vertices.push_back(pos[j]); colors.push_back(rgb[j]); }
                }
        i = 0;
        for (int iz = 0; iz < g.nz; ++iz)
            for (int iy = 0; iy < g.ny; ++iy)
                for (int ix = 0; ix < g.nx; ++ix, ++i)
                    for (int a = 0; a < 3; ++a) {
                        if (!(own[i] & (1u << a))) continue;
                        int cells[4][3];
                        sn_quad_cells(a, ix, iy, iz, cells);
                        int32_t v[4], tri[6];
                        for (int k = 0; k < 4; ++k) {
                            v[k] = vid.at(((size_t)cells[k][2] * g.ny + cells[k][1]) * g.nx + cells[k][0]);
                            if (v[k] < 0) abort();                                        // a quad over a cell without a vertex
                        }
                        float f0;
                        at(ix, iy, iz, f0);
                        sn_quad_faces(v, f0 < 0.f, tri);
                        faces.insert(faces.end(), tri, tri + 6);
                    }
    }
    const int32_t counts[2] = {(int32_t)(vertices.size() / 3), (int32_t)(faces.size() / 3)};
    fwrite(counts, sizeof(int32_t), 2, out);
    if (!vertices.empty()) {                                                             // (an empty vector's data() may be null)
        fwrite(vertices.data(), sizeof(float), vertices.size(), out);
        fwrite(colors.data(), sizeof(float), colors.size(), out);
    }
    if (!faces.empty()) fwrite(faces.data(), sizeof(int32_t), faces.size(), out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: tsdf_host fuse|mesh in out\n"); return 2; }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    const int rc = strcmp(argv[1], "fuse") == 0 ? run_fuse(in, out) : strcmp(argv[1], "mesh") == 0 ? run_mesh(in, out) : 2;
    fclose(in); fclose(out);
    return rc;
}
