// antialias_host.cpp — g++ twin of the opacity compensation's per-Gaussian work, for tests/test_antialias_ref.py: the same
// opacity_compensation_one / opacity_compensation_backward_one (csrc/gsr_math.h) the kernels of csrc/gsr_antialias.hip call, run on
// the host so that they can be held to the binary64 restatement (tests/antialias_ref.py) without a GPU (test infrastructure, as
// structured_host.cpp: nothing in the product loads it).
// Usage: antialias_host IN OUT.  IN: a header line `W H tanfovx tanfovy scale_modifier raw` and the 16 floats of the (transposed)
// view matrix, then one Gaussian per line, 12 floats (mean[3], scale[3], rotation[4], opacity, dL/dout).  raw != 0: log-scales, raw
// quaternions and logits, activated here as the kernels' load does.  OUT: 12 floats per line (out, d opacity, d mean[3], d scale[3],
// d rotation[4]).
#include <stdio.h>

#include "../structured-gaussian-splatting_amd/csrc/gsr_math.h"

int main(int argc, char **argv)
{
    using namespace gsr;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    FrameK f = {};
    int raw = 0;
    float V[16];
    if (fscanf(in, "%d %d %f %f %f %d", &f.W, &f.H, &f.tanfovx, &f.tanfovy, &f.scale_modifier, &raw) != 6) { fprintf(stderr, "bad header\n"); return 1; }
    for (int k = 0; k < 16; ++k)
        if (fscanf(in, "%f", &V[k]) != 1) { fprintf(stderr, "bad view matrix\n"); return 1; }
    f.focal_x = (float)f.W / (2.f * f.tanfovx);        // csrc/gsr_internal.h make_frame
    f.focal_y = (float)f.H / (2.f * f.tanfovy);
    for (;;) {
        float v[12];
        int got = 0;
        while (got < 12 && fscanf(in, "%f", &v[got]) == 1) ++got;
        if (got == 0) break;
        if (got != 12) { fprintf(stderr, "short line\n"); return 1; }
        const float *p = v;
        float sc[3] = {v[3], v[4], v[5]}, q[4] = {v[6], v[7], v[8], v[9]}, opacity = v[10];
        const float logit = v[10], gin = v[11];
        RawAct act;
        if (raw) {
            activate_raw(v + 3, v + 6, logit, act);
            for (int k = 0; k < 3; ++k) sc[k] = act.scale[k];
            for (int k = 0; k < 4; ++k) q[k] = act.q[k];
            opacity = act.opacity;
        }
        const float o = opacity_compensation_one(f, V, p, sc, q, opacity, raw ? &logit : nullptr);
        GeomGrad g;
        opacity_compensation_backward_one(f, V, p, sc, q, opacity, raw ? &act : nullptr, gin, g);
        fprintf(out, "%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", o, g.dopacity, g.dmean[0], g.dmean[1], g.dmean[2],
                g.dscale[0], g.dscale[1], g.dscale[2], g.drot[0], g.drot[1], g.drot[2], g.drot[3]);
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
