// gsr_decoder.hip — the latent structured model's decoder (include/gsrast.h gsr_decoder_*): lin0 IN->32, ReLU; lin1 32->32 plus the
// residual, ReLU; lin2 32->OUT, forward and backward over B structures.  HBM-bound: the forward streams
// (pos_emb, latents) in and decoded out and writes nothing else, the backward recomputes the two hidden layers.
//
// Every product is v_mfma_f32_32x32x2_f32: exact binary32, bit for bit a k-ordered fmaf chain, bias as the initial accumulator.
// One wave owns a tile of 32 structures.  A 32x32 accumulator has its column on the lane (lane & 31) and its rows in the 16
// registers, row(r, h) = (r & 3) + 8 (r >> 2) + 4 h with h = lane >> 5; register r of such a tile X is, unconverted, one k-step
// (k = row(r, 0), row(r, 1)) of the next MFMA: as the B operand it gives A X, as the A operand X^T B, and the other operand is
// loaded at k = row(r, h).  The chain keeps HIDDEN ON THE ROWS and the STRUCTURE ON THE LANE:
//   H1^T = relu(W0 X^T + b0)            A = W0 (lane: row of W0), B = X^T (lane: its structure's input row), k = 2 t + h
//   H2^T = relu(W1 H1^T + b1 + H1^T)    H1^T as B
//   decoded tile = H2 W2^T + b2         H2^T as A: the output COLUMN is on the lane, stored in 128-byte runs
//   dH2^T = W2^T G^T                    B = G^T (lane: its structure's row of G), k = 2 t + h over OUT
//   dH1^T = W1^T dZ1^T + dZ1^T          dZ1^T as B, the residual as the initial accumulator
//   d latents tile = dZ0 W0[:, IN-L:]   dZ0^T as A: the latent column on the lane
// The weight gradients sum over the structure, the LANE index of those tiles, so they take the one transpose: each wave leaves
// H1, H2, dZ1, dZ0 of its tile in LDS as [structure][hidden] (stride 36: 16-byte rows, reads of one k spread over the banks), and
// after a barrier the block's waves share out the accumulator tiles (dW2's column tiles, dW1, dW0's row tiles), each adding the
// block's four tiles in ascending order: acc[i][j] += sum_s A[s][i] B[s][j] with j on the lane, so G and X are read coalesced and
// the bias gradient is the lane's own sum of the B operand.  A block walks a contiguous range of tile groups, writes one partial
// per wanted gradient to the workspace, and k_decoder_reduce adds the partials in ascending block order.  No atomics.
#include "gsr_internal.h"

namespace gsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kDecHidden = 32, kDecMaxIn = 128;
constexpr int kDecWaves = 4, kDecBlock = 64 * kDecWaves;
constexpr int kDecStride = 36;                     // floats per structure of an LDS image
constexpr int kDecImage = 32 * kDecStride;
constexpr int kDecW2Tiles = 4 * kDecWaves;         // dW2 column tiles per launch: four accumulator tiles per wave
constexpr int kDecMaxBlocks = 256;                 // backward partials: one block per CU is resident (LDS, registers)

struct DecShape { int B, IN, L, P0, OUT; };        // P0 = IN - L positional dims

#define GSR_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ int acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// element k of structure s's input row (pos_emb, latents, zeros up to the even k)
__device__ __forceinline__ float load_x(const DecShape &d, const float *__restrict__ pos, const float *__restrict__ lat, int64_t s, int k)
{
    if (s >= d.B) return 0.f;
    if (k < d.P0) return pos[s * d.P0 + k];
    k -= d.P0;
    return k < d.L ? lat[s * d.L + k] : 0.f;
}

// four consecutive floats of a 32-float weight row, 16-byte aligned: the k = row(4 g .. 4 g + 3, h) of one lane
__device__ __forceinline__ float4 load_w4(const float *__restrict__ w, int row, int g, int h)
{
    return *reinterpret_cast<const float4 *>(w + (int64_t)row * kDecHidden + 8 * g + 4 * h);
}

// z += sum over the k-steps t < steps of an MFMA with fa(t), fb(t) (which answer 0 past the end: such a step adds 0 * 0).  The
// loads of eight steps are issued together, and those of the next eight before this batch's MFMAs: at one wave per SIMD nothing
// else hides their latency.  The order of the chain is t ascending, whatever the batching.
template <typename FA, typename FB>
__device__ __forceinline__ void mfma_steps(f32x16 &z, int steps, FA fa, FB fb)
{
    float a[8], b[8], na[8] = {}, nb[8] = {};
#pragma unroll
    for (int i = 0; i < 8; ++i) { a[i] = fa(i); b[i] = fb(i); }
    for (int t0 = 0; t0 < steps; t0 += 8) {
        if (t0 + 8 < steps) {
#pragma unroll
            for (int i = 0; i < 8; ++i) { na[i] = fa(t0 + 8 + i); nb[i] = fb(t0 + 8 + i); }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) z = GSR_MFMA(a[i], b[i], z);
#pragma unroll
        for (int i = 0; i < 8; ++i) { a[i] = na[i]; b[i] = nb[i]; }
    }
}

// H1^T and H2^T of the tile whose structure on this lane is s
__device__ __forceinline__ void hidden_layers(const DecShape &d, const float *__restrict__ pos, const float *__restrict__ lat,
                                              const gsr_decoder_params &p, int64_t s, int c, int h, f32x16 &h1, f32x16 &h2)
{
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = p.b0[acc_row(r, h)];
    mfma_steps(z, (d.IN + 1) / 2,
               [&](int t) { const int k = 2 * t + h; return k < d.IN ? p.w0[c * d.IN + k] : 0.f; },
               [&](int t) { return load_x(d, pos, lat, s, 2 * t + h); });
#pragma unroll
    for (int r = 0; r < 16; ++r) h1[r] = fmaxf(z[r], 0.f);
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = p.b1[acc_row(r, h)];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 a = load_w4(p.w1, c, g, h);
        z = GSR_MFMA(a.x, h1[4 * g + 0], z);
        z = GSR_MFMA(a.y, h1[4 * g + 1], z);
        z = GSR_MFMA(a.z, h1[4 * g + 2], z);
        z = GSR_MFMA(a.w, h1[4 * g + 3], z);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) h2[r] = fmaxf(z[r] + h1[r], 0.f);
}

__global__ __launch_bounds__(kDecBlock) void k_decoder_fwd(DecShape d, const float *__restrict__ pos, const float *__restrict__ lat,
                                                           gsr_decoder_params p, float *__restrict__ decoded)
{
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5;
    const int64_t tile = (int64_t)blockIdx.x * kDecWaves + (threadIdx.x >> 6);
    if (tile * 32 >= d.B) return;
    f32x16 h1, h2;
    hidden_layers(d, pos, lat, p, tile * 32 + c, c, h, h1, h2);
    for (int o = c; o - c < d.OUT; o += 32) {                // column tiles; o: this lane's output column
        const bool ok = o < d.OUT;
        const float bias = ok ? p.b2[o] : 0.f;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = bias;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 b = ok ? load_w4(p.w2, o, g, h) : make_float4(0.f, 0.f, 0.f, 0.f);
            acc = GSR_MFMA(h2[4 * g + 0], b.x, acc);
            acc = GSR_MFMA(h2[4 * g + 1], b.y, acc);
            acc = GSR_MFMA(h2[4 * g + 2], b.z, acc);
            acc = GSR_MFMA(h2[4 * g + 3], b.w, acc);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int64_t row = tile * 32 + acc_row(r, h);
            if (ok && row < d.B) decoded[row * d.OUT + o] = acc[r];
        }
    }
}

// registers of an accumulator tile -> its LDS image [structure = column][hidden = row]
__device__ __forceinline__ void stash(float *__restrict__ img, const f32x16 &v, int c, int h)
{
#pragma unroll
    for (int g = 0; g < 4; ++g)
        *reinterpret_cast<float4 *>(img + c * kDecStride + 8 * g + 4 * h) = make_float4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
}

// The layout of one block's partial in the workspace, and of the reduction's index space: the six gradients back to back.
struct DecPartial {
    int w2, b2, w1, b1, w0, b0, total, stride;         // stride: floats between two blocks' partials (16-byte multiples)
    __host__ __device__ explicit DecPartial(int IN, int OUT)
    {
        w2 = 0; b2 = w2 + OUT * kDecHidden; w1 = b2 + OUT; b1 = w1 + kDecHidden * kDecHidden; w0 = b1 + kDecHidden;
        b0 = w0 + kDecHidden * IN; total = b0 + kDecHidden; stride = (total + 3) & ~3;
    }
};

// `first`: the launch that does everything, with dW2's column tiles [0, kDecW2Tiles); a later launch (OUT > 32 kDecW2Tiles) only
// recomputes H2 and adds the column tiles [ct_begin, ct_begin + kDecW2Tiles) of dW2.  gpb: tile groups (of kDecWaves tiles) per block.
__global__ __launch_bounds__(kDecBlock) void k_decoder_bwd(DecShape d, int gpb, int ct_begin, int first, const float *__restrict__ pos,
                                                           const float *__restrict__ lat, gsr_decoder_params p, const float *__restrict__ G,
                                                           gsr_decoder_grads out, float *__restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) float lds[kDecWaves][4][kDecImage];       // [tile of the group][H1, H2, dZ1, dZ0]
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, w = threadIdx.x >> 6;
    const bool want2 = out.w2 || out.b2, want1 = first && (out.w1 || out.b1), want0 = first && (out.w0 || out.b0);
    const bool sums = want2 || want1 || want0;
    const int ntiles = (d.B + 31) / 32, ngroups = (ntiles + kDecWaves - 1) / kDecWaves;
    const int nct2 = min((d.OUT + 31) / 32, ct_begin + kDecW2Tiles), nit0 = (d.IN + 31) / 32;

    f32x16 acc2[4], accs[2];                                 // dW2 tiles ct_begin + w + 4 u; small units v = w, w + 4 (0: dW1, 1 + i: dW0 rows 32 i ..)
    float bs2[4], bss[2];
#pragma unroll
    for (int u = 0; u < 4; ++u) { bs2[u] = 0.f; for (int r = 0; r < 16; ++r) acc2[u][r] = 0.f; }
#pragma unroll
    for (int u = 0; u < 2; ++u) { bss[u] = 0.f; for (int r = 0; r < 16; ++r) accs[u][r] = 0.f; }

    const int g_end = min((int)(blockIdx.x + 1) * gpb, ngroups);
    for (int grp = (int)blockIdx.x * gpb; grp < g_end; ++grp) {
        const int tile = grp * kDecWaves + w;
        if (tile < ntiles) {
            const int64_t s = (int64_t)tile * 32 + c;
            f32x16 h1, h2;
            hidden_layers(d, pos, lat, p, s, c, h, h1, h2);
            if (sums) stash(lds[w][1], h2, c, h);
            if (first) {
                f32x16 z;
#pragma unroll
                for (int r = 0; r < 16; ++r) z[r] = 0.f;
                const float *grow = G + s * d.OUT;
                mfma_steps(z, (d.OUT + 1) / 2,               // dH2^T = W2^T G^T
                           [&](int t) { const int k = 2 * t + h; return k < d.OUT ? p.w2[k * kDecHidden + c] : 0.f; },
                           [&](int t) { const int k = 2 * t + h; return k < d.OUT && s < d.B ? grow[k] : 0.f; });
                f32x16 dz1, dz0;
#pragma unroll
                for (int r = 0; r < 16; ++r) dz1[r] = h2[r] > 0.f ? z[r] : 0.f;
                z = dz1;                                     // the residual
#pragma unroll
                for (int r = 0; r < 16; ++r) z = GSR_MFMA(p.w1[acc_row(r, h) * kDecHidden + c], dz1[r], z);
#pragma unroll
                for (int r = 0; r < 16; ++r) dz0[r] = h1[r] > 0.f ? z[r] : 0.f;
                if (sums) { stash(lds[w][0], h1, c, h); stash(lds[w][2], dz1, c, h); stash(lds[w][3], dz0, c, h); }
                if (out.latents)
                    for (int j = c; j - c < d.L; j += 32) {  // j: this lane's latent column
                        const bool ok = j < d.L;
#pragma unroll
                        for (int r = 0; r < 16; ++r) z[r] = 0.f;
#pragma unroll
                        for (int r = 0; r < 16; ++r) z = GSR_MFMA(dz0[r], ok ? p.w0[acc_row(r, h) * d.IN + d.P0 + j] : 0.f, z);
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int64_t row = (int64_t)tile * 32 + acc_row(r, h);
                            if (ok && row < d.B) out.latents[row * d.L + j] = z[r];
                        }
                    }
            }
        }
        if (!sums) continue;                                 // (block-uniform)
        __syncthreads();
        const int nt = min(kDecWaves, ntiles - grp * kDecWaves);
        for (int tt = 0; tt < nt; ++tt) {                    // the group's tiles in ascending order
            const int64_t s0 = ((int64_t)grp * kDecWaves + tt) * 32;
            const float *img = lds[tt][0];
            if (want2) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int ct = ct_begin + w + kDecWaves * u;
                    if (ct >= nct2) continue;
                    const int o = ct * 32 + c;
                    float a[16], b[16];                      // acc[hidden][o] += sum_s H2[s][hidden] G[s][o]; the loads first
#pragma unroll
                    for (int t = 0; t < 16; ++t) {
                        const int k = 2 * t + h;
                        a[t] = img[kDecImage + k * kDecStride + c];
                        b[t] = o < d.OUT && s0 + k < d.B ? G[(s0 + k) * d.OUT + o] : 0.f;
                    }
#pragma unroll
                    for (int t = 0; t < 16; ++t) { acc2[u] = GSR_MFMA(a[t], b[t], acc2[u]); bs2[u] += b[t]; }
                }
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const int v = w + kDecWaves * u;
                if (v == 0 ? !want1 : (!want0 || v - 1 >= nit0)) continue;
                float a[16], b[16];
#pragma unroll
                for (int t = 0; t < 16; ++t) {
                    const int k = 2 * t + h;
                    if (v == 0) {                            // acc[hidden in][hidden out] += sum_s H1[s][in] dZ1[s][out]
                        a[t] = img[k * kDecStride + c];
                        b[t] = img[2 * kDecImage + k * kDecStride + c];
                    } else {                                 // acc[input][hidden] += sum_s X[s][input] dZ0[s][hidden]
                        a[t] = load_x(d, pos, lat, s0 + k, (v - 1) * 32 + c);
                        b[t] = img[3 * kDecImage + k * kDecStride + c];
                    }
                }
#pragma unroll
                for (int t = 0; t < 16; ++t) { accs[u] = GSR_MFMA(a[t], b[t], accs[u]); bss[u] += b[t]; }
            }
        }
        __syncthreads();                                     // the next group overwrites the images
    }
    if (!sums) return;

    // this block's partial: tile element [row(r, h)][c] is gradient element [c][row(r, h)] of its unit
    const DecPartial at(d.IN, d.OUT);
    float *part = ws + (int64_t)blockIdx.x * at.stride;
    if (want2) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int ct = ct_begin + w + kDecWaves * u;
            if (ct >= nct2) continue;
            const int o = ct * 32 + c;
            const float b = bs2[u] + __shfl_xor(bs2[u], 32);
            if (o >= d.OUT) continue;
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4 *>(part + at.w2 + o * kDecHidden + 8 * g + 4 * h) =
                    make_float4(acc2[u][4 * g], acc2[u][4 * g + 1], acc2[u][4 * g + 2], acc2[u][4 * g + 3]);
            if (h == 0) part[at.b2 + o] = b;
        }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const int v = w + kDecWaves * u;
        if (v == 0 ? !want1 : (!want0 || v - 1 >= nit0)) continue;
        const float b = bss[u] + __shfl_xor(bss[u], 32);
        if (v == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) part[at.w1 + c * kDecHidden + acc_row(r, h)] = accs[u][r];
            if (h == 0) part[at.b1 + c] = b;
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int in = (v - 1) * 32 + acc_row(r, h);
                if (in < d.IN) part[at.w0 + c * d.IN + in] = accs[u][r];
            }
            if (v == 1 && h == 0) part[at.b0 + c] = b;
        }
    }
}

// one thread per gradient element: the block partials in ascending block order
__global__ __launch_bounds__(256) void k_decoder_reduce(int IN, int OUT, int nblocks, const float *__restrict__ ws, gsr_decoder_grads out)
{
    const DecPartial at(IN, OUT);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= at.total) return;
    float *dst = e < at.b2 ? out.w2 : e < at.w1 ? out.b2 : e < at.b1 ? out.w1 : e < at.w0 ? out.b1 : e < at.b0 ? out.w0 : out.b0;
    const int base = e < at.b2 ? at.w2 : e < at.w1 ? at.b2 : e < at.b1 ? at.w1 : e < at.w0 ? at.b1 : e < at.b0 ? at.w0 : at.b0;
    if (!dst) return;
    float sum = 0.f;
    for (int b0 = 0; b0 < nblocks; b0 += 16) {               // sixteen loads in flight, added in ascending order
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = b0 + i < nblocks ? ws[(int64_t)(b0 + i) * at.stride + e] : 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) if (b0 + i < nblocks) sum = b0 + i ? sum + v[i] : v[i];
    }
    dst[e - base] = sum;
}

}  // namespace gsr

using namespace gsr;

static bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

static int validate_decoder(const char *who, const gsr_decoder_desc *d)
{
    if (!d) { set_error("%s: desc is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->B < 0 || d->B > (1 << 30)) { set_error("%s: B = %d must be in [0, 2^30]", who, d->B); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->hidden_size != kDecHidden) {
        set_error("%s: hidden_size = %d is not supported (the kernels are built for %d)", who, d->hidden_size, kDecHidden);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (d->latent_size < 1 || d->in_size < d->latent_size || d->in_size > kDecMaxIn) {
        set_error("%s: 1 <= latent_size = %d <= in_size = %d <= %d is required", who, d->latent_size, d->in_size, kDecMaxIn);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (d->out_size < 1 || d->out_size > (1 << 20)) {
        set_error("%s: out_size = %d must be in [1, 2^20]", who, d->out_size);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

static int validate_decoder_inputs(const char *who, const gsr_decoder_desc *d, const float *pos_emb, const float *latents,
                                   const gsr_decoder_params *p)
{
    if (!latents) { set_error("%s: latents is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if ((pos_emb != nullptr) != (d->in_size > d->latent_size)) {
        set_error("%s: pos_emb must be given exactly when in_size = %d > latent_size = %d", who, d->in_size, d->latent_size);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!p || !p->w0 || !p->b0 || !p->w1 || !p->b1 || !p->w2 || !p->b2) {
        set_error("%s: the six decoder parameters are required", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!aligned16(p->w1) || !aligned16(p->w2)) { set_error("%s: w1 and w2 must be 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

struct DecGrid { int gpb, nblocks; };

// a function of B alone: at most kDecMaxBlocks blocks, each a contiguous run of gpb tile groups
static DecGrid decoder_grid(int B)
{
    const int ntiles = (int)(((int64_t)B + 31) / 32), ngroups = (ntiles + kDecWaves - 1) / kDecWaves;
    DecGrid g;
    g.gpb = (ngroups + kDecMaxBlocks - 1) / kDecMaxBlocks;
    if (g.gpb < 1) g.gpb = 1;
    g.nblocks = (ngroups + g.gpb - 1) / g.gpb;
    return g;
}

static DecShape decoder_shape(const gsr_decoder_desc &d)
{
    DecShape s;
    s.B = d.B; s.IN = d.in_size; s.L = d.latent_size; s.P0 = d.in_size - d.latent_size; s.OUT = d.out_size;
    return s;
}

extern "C" int gsr_decoder_workspace_size(const gsr_decoder_desc *desc, size_t *bytes)
{
    const char *who = "gsr_decoder_workspace_size";
    if (int rc = validate_decoder(who, desc)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    const DecPartial at(desc->in_size, desc->out_size);
    *bytes = align_up((size_t)decoder_grid(desc->B).nblocks * at.stride * sizeof(float));
    return GSR_OK;
}

extern "C" int gsr_decoder_forward(const gsr_decoder_desc *desc, const float *pos_emb, const float *latents, const gsr_decoder_params *params,
                                   float *decoded, void *stream)
{
    const char *who = "gsr_decoder_forward";
    if (int rc = validate_decoder(who, desc)) return rc;
    if (desc->B == 0) return GSR_OK;
    if (int rc = validate_decoder_inputs(who, desc, pos_emb, latents, params)) return rc;
    if (!decoded) { set_error("%s: decoded is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    const int ntiles = (int)(((int64_t)desc->B + 31) / 32);
    ProfileScope prof("decoder_fwd", s);
    hipLaunchKernelGGL(k_decoder_fwd, dim3((ntiles + kDecWaves - 1) / kDecWaves), dim3(kDecBlock), 0, s, decoder_shape(*desc), pos_emb, latents,
                       *params, decoded);
    GSR_LAUNCH_CHECK("decoder_fwd", false, s);
    return GSR_OK;
}

extern "C" int gsr_decoder_backward(const gsr_decoder_desc *desc, const float *pos_emb, const float *latents, const gsr_decoder_params *params,
                                    const float *d_decoded, const gsr_decoder_grads *grads, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gsr_decoder_backward";
    if (int rc = validate_decoder(who, desc)) return rc;
    if (desc->B == 0) return GSR_OK;
    if (int rc = validate_decoder_inputs(who, desc, pos_emb, latents, params)) return rc;
    if (!d_decoded) { set_error("%s: d_decoded is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!grads) { set_error("%s: grads is NULL (its fields may be)", who); return GSR_ERR_INVALID_ARGUMENT; }
    const bool sums = grads->w0 || grads->b0 || grads->w1 || grads->b1 || grads->w2 || grads->b2;
    if (!sums && !grads->latents) return GSR_OK;             // nothing wanted
    const DecGrid g = decoder_grid(desc->B);
    const DecPartial at(desc->in_size, desc->out_size);
    if (sums) {
        const size_t need = align_up((size_t)g.nblocks * at.stride * sizeof(float));      // = gsr_decoder_workspace_size
        if (!workspace || workspace_bytes < need) {
            set_error("%s: workspace of %zu bytes, %zu needed (gsr_decoder_workspace_size)", who, workspace ? workspace_bytes : (size_t)0, need);
            return GSR_ERR_WORKSPACE;
        }
        if (!aligned16(workspace)) { set_error("%s: workspace must be 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    }
    hipStream_t s = (hipStream_t)stream;
    const DecShape shape = decoder_shape(*desc);
    const int nct2 = (desc->out_size + 31) / 32;
    {
        ProfileScope prof("decoder_bwd", s);
        hipLaunchKernelGGL(k_decoder_bwd, dim3(g.nblocks), dim3(kDecBlock), 0, s, shape, g.gpb, 0, 1, pos_emb, latents, *params, d_decoded,
                           *grads, (float *)workspace);
        if (grads->w2 || grads->b2)
            for (int ct = kDecW2Tiles; ct < nct2; ct += kDecW2Tiles)
                hipLaunchKernelGGL(k_decoder_bwd, dim3(g.nblocks), dim3(kDecBlock), 0, s, shape, g.gpb, ct, 0, pos_emb, latents, *params,
                                   d_decoded, *grads, (float *)workspace);
        GSR_LAUNCH_CHECK("decoder_bwd", false, s);
    }
    if (sums) {
        ProfileScope prof("decoder_reduce", s);
        hipLaunchKernelGGL(k_decoder_reduce, dim3((at.total + 255) / 256), dim3(256), 0, s, desc->in_size, desc->out_size, g.nblocks,
                           (const float *)workspace, *grads);
        GSR_LAUNCH_CHECK("decoder_reduce", false, s);
    }
    return GSR_OK;
}
