// camera_host.cpp — g++ twin of k_camera_bwd's per-Gaussian work, for tests/test_camera_grad_ref.py: the same camera_backward_one
// (csrc/gsr_math.h) the kernel calls, run on the host for every visible Gaussian of a small frame, so that its 27 terms can be held
// to the binary64 reference Gaussian by Gaussian without a GPU (test infrastructure, as host_harness.cpp: nothing in the product
// loads it).  The clamp mask of an SH colour is recomputed with sh_color_one, as the kernel does.
#include "../structured-gaussian-splatting_amd/csrc/gsr_math.h"

extern "C" void camera_terms_host(int n, int D, int M, int W, int H, float tanfovx, float tanfovy, float scale_modifier, const float *V,
                                  const float *PV, const float *campos, const float *means, const float *scales, const float *rots,
                                  const float *covpre, const float *shs, int has_colpre, const int *radii, const float *screen9,
                                  float *out27)
{
    using namespace gsr;
    FrameK f;
    f.P = n; f.D = D; f.M = M; f.W = W; f.H = H;
    f.Gx = (W + GSR_TILE - 1) / GSR_TILE; f.Gy = (H + GSR_TILE - 1) / GSR_TILE; f.ty0 = 0; f.ty1 = f.Gy;
    f.tanfovx = tanfovx; f.tanfovy = tanfovy;
    f.focal_x = (float)W / (2.f * tanfovx); f.focal_y = (float)H / (2.f * tanfovy);
    f.scale_modifier = scale_modifier;
    for (int i = 0; i < n; ++i) {
        float *c = out27 + (size_t)i * kCamTerms;
        for (int k = 0; k < kCamTerms; ++k) c[k] = 0.f;
        if (radii[i] <= 0) continue;
        const float *sh = shs ? shs + (size_t)i * M * 3 : nullptr;
        unsigned clamp_bits = 0;
        if (sh && !has_colpre) { float rgb[3]; sh_color_one<-1>(f, campos, means + 3 * i, sh, rgb, clamp_bits); }
        const float q0[4] = {1.f, 0.f, 0.f, 0.f}, s0[3] = {0.f, 0.f, 0.f};
        camera_backward_one<-1>(f, V, PV, campos, means + 3 * i, covpre ? s0 : scales + 3 * i, covpre ? q0 : rots + 4 * i,
                                covpre ? covpre + 6 * (size_t)i : nullptr, sh, has_colpre != 0, clamp_bits, screen9 + 9 * (size_t)i, c);
    }
}
