// structured_host.cpp — g++ twin of the structured composition's per-child work, for tests/test_structured_ref.py: the same
// compose_child / compose_child_backward (csrc/gsr_math.h) the kernels of csrc/gsr_structured.hip call, run on the host so that
// they can be held to the binary64 restatement (tests/structured_ref.py) without a GPU (test infrastructure, as camera_host.cpp:
// nothing in the product loads it).
// Usage: structured_host IN OUT.  IN: one child per line, 33 floats (c[11], s[11], g[11]: the child's decoder columns, its
// structure, the incoming gradient of the composed child).  OUT: 33 floats per line (composed[11], d_c[11], d_s[11]).
#include <stdio.h>

#include "../structured-gaussian-splatting_amd/csrc/gsr_math.h"

int main(int argc, char **argv)
{
    using namespace gsr;
    if (argc != 3) { fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    FILE *in = fopen(argv[1], "r"), *out = fopen(argv[2], "w");
    if (!in || !out) { fprintf(stderr, "cannot open the files\n"); return 2; }
    for (;;) {
        float v[3 * kChildGeom], r[3 * kChildGeom];
        int got = 0;
        while (got < 3 * kChildGeom && fscanf(in, "%f", &v[got]) == 1) ++got;
        if (got == 0) break;
        if (got != 3 * kChildGeom) { fprintf(stderr, "short line\n"); return 1; }
        compose_child(v, v + kChildGeom, r);
        compose_child_backward(v, v + kChildGeom, v + 2 * kChildGeom, r + kChildGeom, r + 2 * kChildGeom);
        for (int i = 0; i < 3 * kChildGeom; ++i) fprintf(out, "%.9g%c", r[i], i + 1 == 3 * kChildGeom ? '\n' : ' ');
    }
    fclose(in);
    return fclose(out) == 0 ? 0 : 1;
}
