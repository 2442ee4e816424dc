// gsr_structured.hip — the latent structured model's composition (include/gsrast.h gsr_structured_compose_*; the rules are
// written once in gsr_math.h compose_child / compose_child_backward): the decoder's [B, K D] output and the B structures become
// the rasterizer's raw-mode-2 inputs for P = B K children in ONE launch, and their gradients go back in ONE launch, where torch
// runs about twenty slicing and elementwise kernels each way.  HBM-bound; bytes per child in DESIGN.md §10.
//
// Both kernels walk two block ranges of one grid (the idiom of k_act_fwd):
//   [0, nb_sh)        the SH block: a re-striding copy between row stride D (start p D + 11: no alignment to speak of) and the
//                     contiguous [P, M, 3] table.  Indexed by flat table element, four to a thread: the table side moves as
//                     aligned 16-byte words, the decoder side as four dwords that consecutive lanes continue (whole runs of 3M).
//   [nb_sh, +nb_geo)  the geometry block: one thread per child (11 floats in, 11 out), plus its structure's 11.
// The backward's geometry range works in tiles of whole structures: a block takes 256 / K structures (their K children are adjacent
// rows, so no sum crosses a block), every thread writes its child's 11 structure terms to LDS, and after a barrier one thread per
// (structure, component) adds that structure's K terms IN ASCENDING k, ((g_0 + g_1) + g_2) + ... .  K > 256: one structure per
// tile, its children in chunks of 256, the same thread carrying the running sum from chunk to chunk — the same order.  No atomics.
// Grids are capped at kStructMaxBlocks per range and stride over the rest.
#include "gsr_internal.h"

namespace gsr {

constexpr int kStructBlock = 256;
constexpr unsigned kStructMaxBlocks = 2048;

struct StructGrid { unsigned nb_sh, nb_geo; };

static unsigned cap_blocks(int64_t b) { return (unsigned)(b < 1 ? 1 : (b > (int64_t)kStructMaxBlocks ? (int64_t)kStructMaxBlocks : b)); }

// The SH block, either way.  TO_TABLE: table[e] = decoded[p D + 11 + j];  else: decoded[p D + 11 + j] = table ? table[e] : 0
// (e = p 3M + j).  `block` of `blocks` in this range.
template <int M, bool TO_TABLE>
__device__ __forceinline__ void sh_restride(int64_t P, unsigned block, unsigned blocks, const float *__restrict__ src, float *__restrict__ dst)
{
    constexpr int n3 = 3 * M, D = kChildGeom + n3;
    const int64_t total = P * n3, nq = total / 4, stride = (int64_t)blocks * kStructBlock;
    for (int64_t q = (int64_t)block * kStructBlock + threadIdx.x; q < nq; q += stride) {
        const int64_t e = 4 * q, p = e / n3;
        int j = (int)(e - p * n3);
        int64_t row = p * D + kChildGeom;
        if (TO_TABLE) {
            float v[4];
            for (int i = 0; i < 4; ++i) { v[i] = src[row + j]; if (++j == n3) { j = 0; row += D; } }
            reinterpret_cast<float4 *>(dst)[q] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            const float4 g = src ? reinterpret_cast<const float4 *>(src)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float v[4] = {g.x, g.y, g.z, g.w};
            for (int i = 0; i < 4; ++i) { dst[row + j] = v[i]; if (++j == n3) { j = 0; row += D; } }
        }
    }
    if (block == 0 && (int64_t)threadIdx.x < total - nq * 4) {       // the last 1..3 elements
        const int64_t e = nq * 4 + threadIdx.x, p = e / n3, at = p * D + kChildGeom + (e - p * n3);
        if (TO_TABLE) dst[e] = src[at];
        else dst[at] = src ? src[e] : 0.f;
    }
}

__device__ __forceinline__ void load_structure(const gsr_structures &st, int b, float s[kChildGeom])
{
    for (int i = 0; i < 3; ++i) { s[i] = st.means[3 * (int64_t)b + i]; s[4 + i] = st.scales[3 * (int64_t)b + i]; }
    s[3] = st.opacities[b];
    for (int i = 0; i < 4; ++i) s[7 + i] = st.rotations[4 * (int64_t)b + i];
}

template <int M>
__global__ __launch_bounds__(kStructBlock) void k_structured_fwd(int B, int K, StructGrid grid, const float *__restrict__ decoded,
                                                                  gsr_structures st, gsr_children out)
{
    constexpr int D = kChildGeom + 3 * M;
    const int P = B * K;
    unsigned blk = blockIdx.x;
    if (blk < grid.nb_sh) {
        sh_restride<M, true>(P, blk, grid.nb_sh, decoded, out.features);
        return;
    }
    blk -= grid.nb_sh;
    const int stride = (int)grid.nb_geo * kStructBlock;      // <= 2^19
    for (int p = (int)blk * kStructBlock + threadIdx.x; p < P; p += stride) {
        const float *row = decoded + (int64_t)p * D;
        float c[kChildGeom], s[kChildGeom], o[kChildGeom];
        for (int i = 0; i < kChildGeom; ++i) c[i] = row[i];
        load_structure(st, p / K, s);
        compose_child(c, s, o);
        for (int i = 0; i < 3; ++i) { out.xyz[3 * (int64_t)p + i] = o[i]; out.scaling[3 * (int64_t)p + i] = o[4 + i]; }
        out.opacity[p] = o[3];
        reinterpret_cast<float4 *>(out.rotation)[p] = make_float4(o[7], o[8], o[9], o[10]);
    }
}

template <int M>
__global__ __launch_bounds__(kStructBlock) void k_structured_bwd(int B, int K, StructGrid grid, const float *__restrict__ decoded,
                                                                  gsr_structures st, gsr_children_grads gin, gsr_structured_grads out)
{
    constexpr int D = kChildGeom + 3 * M;
    __shared__ float part[kStructBlock * kChildGeom];        // [child of the tile][structure component]
    unsigned blk = blockIdx.x;
    if (blk < grid.nb_sh) {
        if (out.decoded) sh_restride<M, false>((int64_t)B * K, blk, grid.nb_sh, gin.features, out.decoded);
        return;
    }
    blk -= grid.nb_sh;
    const bool reduce = out.means || out.opacities || out.scales || out.rotations;
    const int ck = K < kStructBlock ? K : kStructBlock;      // children of ONE structure per chunk
    const int spb = kStructBlock / ck;                       // structures per tile (1 when K >= 256)
    const int tiles = (B + spb - 1) / spb;
    const int tid = threadIdx.x;
    for (int tile = (int)blk; tile < tiles; tile += (int)grid.nb_geo) {
        const int b0 = tile * spb, ns = min(spb, B - b0);
        float carry = 0.f;                                   // K > 256: thread r < 11 holds component r's sum over the chunks so far
        for (int k0 = 0; k0 < K; k0 += ck) {
            const int nk = min(ck, K - k0);
            const int sl = tid / nk, kk = tid - sl * nk;     // this thread's structure of the tile, child of the chunk
            if (sl < ns) {
                const int b = b0 + sl, p = b * K + k0 + kk;
                const float *row = decoded + (int64_t)p * D;
                float c[kChildGeom], s[kChildGeom], g[kChildGeom], d_c[kChildGeom], d_s[kChildGeom];
                for (int i = 0; i < kChildGeom; ++i) c[i] = row[i];
                load_structure(st, b, s);
                for (int i = 0; i < 3; ++i) {
                    g[i] = gin.xyz ? gin.xyz[3 * (int64_t)p + i] : 0.f;
                    g[4 + i] = gin.scaling ? gin.scaling[3 * (int64_t)p + i] : 0.f;
                }
                g[3] = gin.opacity ? gin.opacity[p] : 0.f;
                const float4 gr = gin.rotation ? reinterpret_cast<const float4 *>(gin.rotation)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
                g[7] = gr.x; g[8] = gr.y; g[9] = gr.z; g[10] = gr.w;
                compose_child_backward(c, s, g, d_c, d_s);
                if (out.decoded) {
                    float *drow = out.decoded + (int64_t)p * D;
                    for (int i = 0; i < kChildGeom; ++i) drow[i] = d_c[i];
                }
                if (reduce)
                    for (int i = 0; i < kChildGeom; ++i) part[tid * kChildGeom + i] = d_s[i];
            }
            if (!reduce) continue;                           // (block-uniform)
            __syncthreads();
            for (int r = tid; r < ns * kChildGeom; r += kStructBlock) {
                const int sr = r / kChildGeom, comp = r - sr * kChildGeom;
                float *dst = comp < 3 ? out.means : comp == 3 ? out.opacities : comp < 7 ? out.scales : out.rotations;
                if (!dst) continue;
                const float *term = part + (sr * nk) * kChildGeom + comp;
                float sum = k0 == 0 ? term[0] : carry + term[0];
                for (int k = 1; k < nk; ++k) sum += term[k * kChildGeom];        // ascending k
                if (k0 + nk < K) { carry = sum; continue; }
                const int64_t bs = b0 + sr;
                if (comp < 3) dst[3 * bs + comp] = sum;
                else if (comp == 3) dst[bs] = sum;
                else if (comp < 7) dst[3 * bs + comp - 4] = sum;
                else dst[4 * bs + comp - 7] = sum;
            }
            __syncthreads();                                 // the next chunk or tile overwrites `part`
        }
    }
}

}  // namespace gsr

using namespace gsr;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int validate_structured(const char *who, const gsr_structured_desc *d, const float *decoded, const gsr_structures *st)
{
    if (!d) { set_error("%s: desc is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->B < 0) { set_error("%s: B = %d must be >= 0", who, d->B); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->K < 1) { set_error("%s: K = %d must be >= 1", who, d->K); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->sh_coeffs != 1 && d->sh_coeffs != 4 && d->sh_coeffs != 9 && d->sh_coeffs != 16) {
        set_error("%s: sh_coeffs = %d must be 1, 4, 9 or 16", who, d->sh_coeffs);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((int64_t)d->B * d->K >= ((int64_t)1 << 28)) {
        set_error("%s: B K = %lld children must be < 2^28", who, (long long)d->B * d->K);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (d->B == 0) return GSR_OK;
    if (!decoded) { set_error("%s: decoded is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!st || !st->means || !st->opacities || !st->scales || !st->rotations) {
        set_error("%s: the four structure tensors are required", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static StructGrid struct_grid(const gsr_structured_desc &d, bool backward)
{
    const int64_t P = (int64_t)d.B * d.K;
    StructGrid g;
    g.nb_sh = cap_blocks((P * 3 * d.sh_coeffs / 4 + kStructBlock - 1) / kStructBlock);
    const int spb = kStructBlock / (d.K < kStructBlock ? d.K : kStructBlock);      // the backward's tiles: k_structured_bwd
    g.nb_geo = cap_blocks(backward ? ((int64_t)d.B + spb - 1) / spb : (P + kStructBlock - 1) / kStructBlock);
    return g;
}

extern "C" int gsr_structured_compose_forward(const gsr_structured_desc *desc, const float *decoded, const gsr_structures *structures,
                                              const gsr_children *out, void *stream)
{
    const char *who = "gsr_structured_compose_forward";
    if (int rc = validate_structured(who, desc, decoded, structures)) return rc;
    if (desc->B == 0) return GSR_OK;
    if (!out || !out->xyz || !out->opacity || !out->scaling || !out->rotation || !out->features) {
        set_error("%s: the five child tensors are required", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(out->xyz) || !aligned16(out->opacity) || !aligned16(out->scaling) || !aligned16(out->rotation) || !aligned16(out->features)) {
        set_error("%s: the child tensors must be 16-byte aligned", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    const StructGrid g = struct_grid(*desc, false);
    const dim3 blocks(g.nb_sh + g.nb_geo), threads(kStructBlock);
    ProfileScope prof("structured_fwd", s);
    switch (desc->sh_coeffs) {
    case 1: hipLaunchKernelGGL(k_structured_fwd<1>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *out); break;
    case 4: hipLaunchKernelGGL(k_structured_fwd<4>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *out); break;
    case 9: hipLaunchKernelGGL(k_structured_fwd<9>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *out); break;
    default: hipLaunchKernelGGL(k_structured_fwd<16>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *out); break;
    }
    GSR_LAUNCH_CHECK("structured_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_structured_compose_backward(const gsr_structured_desc *desc, const float *decoded, const gsr_structures *structures,
                                               const gsr_children_grads *grads_in, const gsr_structured_grads *out, void *stream)
{
    const char *who = "gsr_structured_compose_backward";
    if (int rc = validate_structured(who, desc, decoded, structures)) return rc;
    if (desc->B == 0) return GSR_OK;
    if (!grads_in || !out) { set_error("%s: the gradient structs are required (their fields may be NULL)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!aligned16(grads_in->xyz) || !aligned16(grads_in->opacity) || !aligned16(grads_in->scaling) || !aligned16(grads_in->rotation) ||
        !aligned16(grads_in->features)) {
        set_error("%s: the child gradients must be 16-byte aligned", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!out->decoded && !out->means && !out->opacities && !out->scales && !out->rotations) return GSR_OK;      // nothing wanted
    hipStream_t s = (hipStream_t)stream;
    const StructGrid g = struct_grid(*desc, true);
    const dim3 blocks(g.nb_sh + g.nb_geo), threads(kStructBlock);
    ProfileScope prof("structured_bwd", s);
    switch (desc->sh_coeffs) {
    case 1: hipLaunchKernelGGL(k_structured_bwd<1>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *grads_in, *out); break;
    case 4: hipLaunchKernelGGL(k_structured_bwd<4>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *grads_in, *out); break;
    case 9: hipLaunchKernelGGL(k_structured_bwd<9>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *grads_in, *out); break;
    default: hipLaunchKernelGGL(k_structured_bwd<16>, blocks, threads, 0, s, desc->B, desc->K, g, decoded, *structures, *grads_in, *out); break;
    }
    GSR_LAUNCH_CHECK("structured_bwd", false, s);
    return GSR_OK;
}
