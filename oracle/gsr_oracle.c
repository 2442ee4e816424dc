/* gsr_oracle.c — CPU oracle of the differentiable Gaussian rasterizer hot path.
 *
 * TEST INFRASTRUCTURE, NOT PRODUCT.  Only tests/, __graft_entry__.smoke() and the
 * `cpu_baseline` leg of bench.py may load this library; the product path
 * (structured-gaussian-splatting_amd/) never imports, links or calls it.
 *
 * What it restates: the reference's rasterizer lives in the un-vendored git submodule
 * graphdeco-inria/diff-gaussian-rasterization (.gitmodules:4-6 of the reference; directory empty,
 * pinned SHA unrecoverable).  Its published algorithm is restated here from SURVEY.md Appendix A
 * (A.0 .. A.11), anchored on the reference's own call site (gaussian_renderer/__init__.py:36-49,
 * 85-93) and on the in-tree Python twins of its sub-steps (utils/sh_utils.py:57-112,
 * utils/graphics_utils.py:22-71, utils/general_utils.py:64-110, scene/gaussian_model.py:25-29).
 *
 * PARITY STATUS: the sub-steps that have an in-tree twin (SH colour, camera matrices, point
 * transform) are pinned by golden vectors generated from the reference's own Python
 * (tests/golden/make_golden.py).  The rasterizer proper (EWA projection constants, tile binning,
 * alpha-blend skip/stop rules, the explicit backward) has no executable reference, test or golden
 * vector anywhere in /root/reference  =>  for those steps "PARITY UNPINNED" (SURVEY.md 8c); they are
 * held to self-consistency instead (fp64 autograd of an independent torch restatement, analytic
 * known-answer cases) in tests/test_oracle_*.py.
 *
 * Build: see oracle/Makefile (gcc, -O2 -ffp-contract=off so the float build is plain IEEE binary32).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/gsr_constants.h"

/* fragile_px: one bit per band a blend decision fell into (gsr_oracle.py FRAGILE_BITS names them) */
#define GSO_FRAG_POWER 1u   /* sign of the power */
#define GSO_FRAG_ALPHA 2u   /* alpha against 1/255 */
#define GSO_FRAG_DEPTH 4u   /* depth order of two list neighbours that both reach the pixel */
#define GSO_FRAG_TCUT  8u   /* transmittance against the cut-off */
#define GSO_FRAG_TILE  16u  /* tile membership of a splat that reaches the pixel */

/* backward_screen's front-to-back order restarts from the forward's state every GSO_SEG list entries, as the HIP backward
 * restarts from its checkpoints (csrc/gsr_internal.h kSeg) */
#define GSO_SEG 128

#define GSO_CAT_(a, b) a##b
#define GSO_CAT(a, b) GSO_CAT_(a, b)

/* ---- binary32 instantiation: gso_*_f32
 * R_VIEW: component k of p_view.  The one fused operation of the binary32 build: the reference's compiler contracts the
 * left-to-right sum of transformPoint4x3 into fma(p2, ., fma(p1, ., p0 * .)) + . (the depth band's "dB"), and the product's
 * csrc/gsr_math.h view_coord() evaluates exactly that.  At the identity camera it is the plain sum's result. */
#define REAL float
#define FN(name) GSO_CAT(GSO_CAT(gso_, name), _f32)
#define R_SQRT sqrtf
#define R_EXP expf
#define R_CEIL ceilf
#define R_FABS fabsf
#define R_VIEW(p, V, k) (fmaf((p)[2], (V)[8 + (k)], fmaf((p)[1], (V)[4 + (k)], (p)[0] * (V)[k])) + (V)[12 + (k)])
#include "gsr_oracle_impl.h"
#undef REAL
#undef FN
#undef R_SQRT
#undef R_EXP
#undef R_CEIL
#undef R_FABS
#undef R_VIEW

/* ---- binary64 instantiation: gso_*_f64 */
#define REAL double
#define FN(name) GSO_CAT(GSO_CAT(gso_, name), _f64)
#define R_SQRT sqrt
#define R_EXP exp
#define R_CEIL ceil
#define R_FABS fabs
#define R_VIEW(p, V, k) ((p)[0] * (V)[k] + (p)[1] * (V)[4 + (k)] + (p)[2] * (V)[8 + (k)] + (V)[12 + (k)])
#include "gsr_oracle_impl.h"
#undef REAL
#undef FN

int gso_version(void) { return 1; }

/* A.12 (next-row f2): mean squared distance to the 3 nearest other points, brute force.
 * Twin of the external simple_knn distCUDA2 called at scene/gaussian_model.py:144. */
void gso_dist2_knn3(int P, const float *xyz, float *out)
{
    for (int i = 0; i < P; ++i) {
        double best[3] = {1e300, 1e300, 1e300};
        for (int j = 0; j < P; ++j) {
            if (j == i) continue;
            double dx = (double)xyz[3 * i] - xyz[3 * j], dy = (double)xyz[3 * i + 1] - xyz[3 * j + 1],
                   dz = (double)xyz[3 * i + 2] - xyz[3 * j + 2];
            double d = dx * dx + dy * dy + dz * dz;
            if (d < best[2]) {
                best[2] = d;
                if (best[2] < best[1]) { double t = best[1]; best[1] = best[2]; best[2] = t; }
                if (best[1] < best[0]) { double t = best[0]; best[0] = best[1]; best[1] = t; }
            }
        }
        int n = P - 1 < 3 ? P - 1 : 3;
        double s = 0;
        for (int k = 0; k < n; ++k) s += best[k];
        out[i] = n > 0 ? (float)(s / 3.0) : 0.0f;
    }
}
