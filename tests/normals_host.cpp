// normals_host.cpp — the per-element functions of csrc/gsr_normals_math.h that the kernels of csrc/gsr_normals.hip call, run on the host
// over whole cases so that they can be held to the binary64 restatement (tests/normals_ref.py) and run under the address and
// undefined-behaviour sanitizers (tests/test_normals_ref.py builds this file with them).  Every array is a heap allocation of exactly
// its size, and an image is one allocation per ROW: a stencil that reads one pixel past a row, or a row past the image, stops the program.
//
//   normals_host maps  in out     in:  int32 H, W; float tanfovx, tanfovy, alpha_min, grad_loss; depth, alpha [H,W]; grad_n, N [3,H,W]
//                                 out: n [3,H,W]; ddepth, dalpha [H,W] (of grad_n); loss [1]; dN [3,H,W]; ddepth, dalpha [H,W] (of the loss)
//   normals_host gauss in out     in:  int32 P; V [16]; campos [3]; scales [P,3]; rotations [P,4]; means [P,3]; grad_out [P,3]
//                                 out: normals [P,3]; dq [P,4]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../structured-gaussian-splatting_amd/csrc/gsr_normals_math.h"

using namespace gsr;

struct Image {                                       // [H,W], a heap allocation per row
    int H, W;
    std::vector<std::unique_ptr<float[]>> rows;
    Image(int h, int w) : H(h), W(w)
    {
        for (int y = 0; y < H; ++y) {
            rows.emplace_back(new float[(size_t)W]);
            for (int x = 0; x < W; ++x) rows.back()[x] = 0.f;
        }
    }
    float &at(int x, int y) { return rows[(size_t)y][x]; }
    float at(int x, int y) const { return rows[(size_t)y][x]; }
    void read(FILE *f) { for (int y = 0; y < H; ++y) if (fread(rows[(size_t)y].get(), sizeof(float), (size_t)W, f) != (size_t)W) exit(4); }
    void write(FILE *f) const { for (int y = 0; y < H; ++y) fwrite(rows[(size_t)y].get(), sizeof(float), (size_t)W, f); }
};

struct Image3 {
    Image c[3];
    Image3(int h, int w) : c{Image(h, w), Image(h, w), Image(h, w)} {}
    void read(FILE *f) { for (auto &i : c) i.read(f); }
    void write(FILE *f) const { for (auto &i : c) i.write(f); }
};

struct ZAt {                                         // the accessor of gsr_normals_math.h over the whole image
    const Image &z;
    bool operator()(int x, int y, float &out) const { out = z.at(x, y); return out >= 0.f; }
};

// The backward as the kernel does it: the takes of every pixel, then the gather and the chain.  LOSS: g is formed from N and alpha.
static void backward(const NrmDims &d, const Image &z, const Image &alpha, const Image3 &gin, bool loss, float scale, Image3 *dN, Image &ddepth,
                     Image &dalpha)
{
    std::vector<Image> take;
    for (int s = 0; s < 4; ++s) take.emplace_back(d.H, d.W);
    const ZAt zat{z};
    for (int y = 0; y < d.H; ++y)
        for (int x = 0; x < d.W; ++x) {
            NrmStencil s;
            float gz[4] = {0.f, 0.f, 0.f, 0.f}, nv[3] = {0.f, 0.f, 0.f}, a = 0.f;
            const bool has = nrm_stencil(d, x, y, zat, s);
            if (has) {
                const float px = nrm_px(d, x), py = nrm_py(d, y);
                const float inv = nrm_normal_one(d, px, py, s, nv);
                float g[3] = {gin.c[0].at(x, y), gin.c[1].at(x, y), gin.c[2].at(x, y)};
                if (loss) {
                    a = alpha.at(x, y) * scale;
                    g[0] *= a; g[1] *= a; g[2] *= a;
                }
                nrm_normal_backward_one(d, px, py, s, nv, inv, g, gz);
            }
            for (int k = 0; k < 4; ++k) take[(size_t)k].at(x, y) = gz[k];
            if (dN) for (int c = 0; c < 3; ++c) dN->c[c].at(x, y) = has ? a * nv[c] : 0.f;
        }
    const auto taken = [&](int x, int y, int slot) { return take[(size_t)slot].at(x, y); };
    for (int y = 0; y < d.H; ++y)
        for (int x = 0; x < d.W; ++x) {
            float gd = 0.f, ga = 0.f;
            if (z.at(x, y) >= 0.f) nrm_chain(nrm_gather(d, x, y, taken), z.at(x, y), alpha.at(x, y), gd, ga);
            ddepth.at(x, y) = gd; dalpha.at(x, y) = ga;
        }
}

static int run_maps(FILE *in, FILE *out)
{
    int32_t hw[2];
    float par[4];
    if (fread(hw, sizeof(int32_t), 2, in) != 2 || fread(par, sizeof(float), 4, in) != 4) return 4;
    const int H = hw[0], W = hw[1];
    const NrmDims d = nrm_dims(H, W, par[0], par[1], par[2]);
    Image depth(H, W), alpha(H, W), z(H, W);
    Image3 g(H, W), N(H, W), n(H, W), dN(H, W);
    depth.read(in); alpha.read(in); g.read(in); N.read(in);
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) z.at(x, y) = nrm_valid(d, depth.at(x, y), alpha.at(x, y)) ? depth.at(x, y) / alpha.at(x, y) : -1.f;
    const ZAt zat{z};
    double total = 0.0;
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) {
            NrmStencil s;
            float nv[3] = {0.f, 0.f, 0.f};
            const bool has = nrm_stencil(d, x, y, zat, s);
            if (has) nrm_normal_one(d, nrm_px(d, x), nrm_py(d, y), s, nv);
            for (int c = 0; c < 3; ++c) n.c[c].at(x, y) = nv[c];
            const float Nv[3] = {N.c[0].at(x, y), N.c[1].at(x, y), N.c[2].at(x, y)};
            total += (double)nrm_loss_term(has, alpha.at(x, y), Nv, nv);
        }
    const float loss = H * W ? (float)(total * (1.0 / ((double)H * (double)W))) : 0.f;
    Image dd(H, W), da(H, W), ddl(H, W), dal(H, W);
    backward(d, z, alpha, g, false, 0.f, nullptr, dd, da);
    const float scale = H * W ? -(par[3] * (float)(1.0 / ((double)H * (double)W))) : 0.f;
    backward(d, z, alpha, N, true, scale, &dN, ddl, dal);
    n.write(out); dd.write(out); da.write(out);
    fwrite(&loss, sizeof(float), 1, out);
    dN.write(out); ddl.write(out); dal.write(out);
    return 0;
}

static std::unique_ptr<float[]> read_array(FILE *f, size_t n)
{
    std::unique_ptr<float[]> a(new float[n]);
    if (n && fread(a.get(), sizeof(float), n, f) != n) exit(4);
    return a;
}

static int run_gauss(FILE *in, FILE *out)
{
    int32_t P;
    if (fread(&P, sizeof(int32_t), 1, in) != 1) return 4;
    const size_t n = (size_t)P;
    const auto V = read_array(in, 16), cam = read_array(in, 3);
    const auto scales = read_array(in, 3 * n), rot = read_array(in, 4 * n), means = read_array(in, 3 * n), g = read_array(in, 3 * n);
    std::unique_ptr<float[]> o(new float[3 * n]), dq(new float[4 * n]);
    for (size_t i = 0; i < n; ++i) {
        nrm_gaussian_forward_one(&scales[3 * i], &rot[4 * i], &means[3 * i], V.get(), cam.get(), &o[3 * i]);
        nrm_gaussian_backward_one(&scales[3 * i], &rot[4 * i], &means[3 * i], V.get(), cam.get(), &g[3 * i], &dq[4 * i]);
    }
    fwrite(o.get(), sizeof(float), 3 * n, out);
    fwrite(dq.get(), sizeof(float), 4 * n, out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: normals_host maps|gauss in out\n"); return 2; }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    const int rc = strcmp(argv[1], "maps") == 0 ? run_maps(in, out) : strcmp(argv[1], "gauss") == 0 ? run_gauss(in, out) : 2;
    fclose(in); fclose(out);
    return rc;
}
