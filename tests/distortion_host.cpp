// distortion_host.cpp — the per-element functions of csrc/gsr_distortion_math.h that the kernels of csrc/gsr_distortion.hip call, run on
// the host over whole cases so that they can be held to the binary64 restatement (tests/distortion_ref.py) and run under the address
// and undefined-behaviour sanitizers (tests/test_distortion_ref.py builds this file with them).  Every array is a heap allocation of
// exactly its size: a read one element past a plane stops the program.  Plane 2 of the moments map is not even allocated.
//
//   distortion_host maps  in out   in:  int32 H, W; float grad_loss; M1, M2, alpha, grad_map [H W]
//                                  out: D [H W]; dM1, dM2, dM3, dalpha [H W] (of grad_map); loss [1]; dM1, dM2, dM3, dalpha [H W] (of the loss)
//   distortion_host gauss in out   in:  int32 P, mapping; float near, far; V [16]; means [P,3]; grad_out [P,3]
//                                  out: moments [P,3]; dmeans [P,3]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>

#include "../structured-gaussian-splatting_amd/csrc/gsr_distortion_math.h"

using namespace gsr;

typedef std::unique_ptr<float[]> Array;

static Array make_array(size_t n) { return Array(new float[n]); }

static Array read_array(FILE *f, size_t n)
{
    Array a = make_array(n);
    if (n && fread(a.get(), sizeof(float), n, f) != n) exit(4);
    return a;
}

static void backward(size_t n, const float *A, const float *M1, const float *M2, const float *g, float gs, bool loss, FILE *out)
{
    Array dM1 = make_array(n), dM2 = make_array(n), dM3 = make_array(n), dA = make_array(n);
    for (size_t i = 0; i < n; ++i) {
        dst_pixel_backward(loss ? gs : g[i], A[i], M1[i], M2[i], dA[i], dM1[i], dM2[i]);
        dM3[i] = 0.f;
    }
    fwrite(dM1.get(), sizeof(float), n, out); fwrite(dM2.get(), sizeof(float), n, out);
    fwrite(dM3.get(), sizeof(float), n, out); fwrite(dA.get(), sizeof(float), n, out);
}

static int run_maps(FILE *in, FILE *out)
{
    int32_t hw[2];
    float grad_loss;
    if (fread(hw, sizeof(int32_t), 2, in) != 2 || fread(&grad_loss, sizeof(float), 1, in) != 1) return 4;
    const size_t n = (size_t)hw[0] * (size_t)hw[1];
    const Array M1 = read_array(in, n), M2 = read_array(in, n), A = read_array(in, n), g = read_array(in, n);
    Array D = make_array(n);
    double total = 0.0;
    for (size_t i = 0; i < n; ++i) { D[i] = dst_pixel(A[i], M1[i], M2[i]); total += (double)D[i]; }
    fwrite(D.get(), sizeof(float), n, out);
    backward(n, A.get(), M1.get(), M2.get(), g.get(), 0.f, false, out);
    const float loss = n ? (float)(total * (1.0 / (double)n)) : 0.f;
    fwrite(&loss, sizeof(float), 1, out);
    backward(n, A.get(), M1.get(), M2.get(), nullptr, n ? dst_loss_scale(grad_loss, (int64_t)n) : 0.f, true, out);
    return 0;
}

static int run_gauss(FILE *in, FILE *out)
{
    int32_t pm[2];
    float planes[2];
    if (fread(pm, sizeof(int32_t), 2, in) != 2 || fread(planes, sizeof(float), 2, in) != 2) return 4;
    const size_t n = (size_t)pm[0];
    const DstMapping map = dst_mapping(pm[1], planes[0], planes[1]);
    const Array V = read_array(in, 16), means = read_array(in, 3 * n), g = read_array(in, 3 * n);
    Array o = make_array(3 * n), d = make_array(3 * n);
    for (size_t i = 0; i < n; ++i) {
        dst_moments_one(map, &means[3 * i], V.get(), &o[3 * i]);
        dst_moments_backward_one(map, &means[3 * i], V.get(), &g[3 * i], &d[3 * i]);
    }
    fwrite(o.get(), sizeof(float), 3 * n, out);
    fwrite(d.get(), sizeof(float), 3 * n, out);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: distortion_host maps|gauss in out\n"); return 2; }
    FILE *in = fopen(argv[2], "rb"), *out = fopen(argv[3], "wb");
    if (!in || !out) return 3;
    const int rc = strcmp(argv[1], "maps") == 0 ? run_maps(in, out) : strcmp(argv[1], "gauss") == 0 ? run_gauss(in, out) : 2;
    fclose(in); fclose(out);
    return rc;
}
