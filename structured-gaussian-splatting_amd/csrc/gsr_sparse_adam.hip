// gsr_sparse_adam.hip — the optimizer step of gsr_optim.hip over the rows a frame saw (upstream's optimizer_type = "sparse_adam":
// a Gaussian with radii <= 0 has an exactly zero gradient, and its parameter and both moments keep their bits).
// Every tensor of the step has the same number of rows; tensor t has `width[t]` contiguous floats per row; ONE per-row mask governs
// the launch.  Per element of a visible row: the three statements of GSR_ADAM1 (gsr_optim.hip), so an all-visible mask is the dense
// step bit for bit.  Per element of a hidden row: nothing is read but the row's mask entry.
//
// Work item = the dense kernel's: kSparseChunk consecutive float4 of one tensor, a thread takes kSparsePer of them 256 apart, and
// all of a thread's loads are issued before its first store.  A thread decides per float4 from the mask entries of the (at most
// two, for width >= 3) rows under it: all hidden -> no load and no store; partly hidden -> loaded, the hidden components stored
// back as they were.  There is no vote: a wave whose 64 float4 are hidden skips the loads on its empty exec mask.
//
// The row of an element: ONE 64-bit division per work item (block-uniform: row and column of the item's first element), then a
// 32-bit division of an offset < width + 4096 by the width, which is a compile-time constant for the widths of the model's
// tensors (1, 3, 4 and 3 M for M = 4, 9, 16: a multiply-high and a shift).  Any other width takes the run-time divisions.
#include "gsr_internal.h"

namespace gsr {

constexpr int kSparseBlock = 256;
constexpr int kSparsePer = 4;
constexpr int kSparseChunk = kSparseBlock * kSparsePer;          // float4 per work item, as k_adam_multi's

struct AdamSparse {
    float *p[GSR_ADAM_MAX_TENSORS]; const float *g[GSR_ADAM_MAX_TENSORS]; float *m[GSR_ADAM_MAX_TENSORS]; float *v[GSR_ADAM_MAX_TENSORS];
    unsigned long long n[GSR_ADAM_MAX_TENSORS];
    unsigned long long item_end[GSR_ADAM_MAX_TENSORS];           // running count of work items; entries [count, ...) are not set
    float step_head[GSR_ADAM_MAX_TENSORS], step_tail[GSR_ADAM_MAX_TENSORS], inv_bc2_sqrt[GSR_ADAM_MAX_TENSORS];
    uint32_t width[GSR_ADAM_MAX_TENSORS], split[GSR_ADAM_MAX_TENSORS];      // split == width: one learning rate
    const void *mask;                                            // one entry per row
    int mask_bytes;                                              // 1: non-zero = visible; 4: int32 > 0 = visible
    int count;
};

struct AdamConsts { float one_minus_b1, b2, one_minus_b2, eps; };

__device__ __forceinline__ bool row_seen(const AdamSparse &a, unsigned long long r)
{
    return a.mask_bytes == 1 ? static_cast<const uint8_t *>(a.mask)[r] != 0 : static_cast<const int32_t *>(a.mask)[r] > 0;
}

// the entries of rows r .. r + 3 as bits 0 .. 3: one load (the compiler words the copy for the alignment it may assume)
__device__ __forceinline__ uint32_t rows_seen4(const AdamSparse &a, unsigned long long r)
{
    if (a.mask_bytes == 1) {
        uint32_t b;
        __builtin_memcpy(&b, static_cast<const uint8_t *>(a.mask) + r, 4);
        return ((b & 0xffu) != 0) | ((b & 0xff00u) != 0) << 1 | ((b & 0xff0000u) != 0) << 2 | ((b & 0xff000000u) != 0) << 3;
    }
    int32_t d[4];
    __builtin_memcpy(d, static_cast<const int32_t *>(a.mask) + r, 16);
    return (uint32_t)(d[0] > 0) | (uint32_t)(d[1] > 0) << 1 | (uint32_t)(d[2] > 0) << 2 | (uint32_t)(d[3] > 0) << 3;
}

// W: the tensor's width when it is one of the specialised ones, 0: read it from the launch
template <int W>
__device__ __forceinline__ void adam_sparse_item(const AdamSparse &a, const int t, const unsigned long long first, const AdamConsts c)
{
    const uint32_t w = W ? (uint32_t)W : a.width[t];
    const unsigned long long n = a.n[t], n4 = n / 4;
    // row and column of the item's first element.  An item starts at a multiple of 4096 elements: column 0 where w divides that
    const unsigned long long e0 = first * 4;
    const unsigned long long row0 = e0 / w;
    const uint32_t col0 = (W && (4 * kSparseChunk) % (W ? W : 1) == 0) ? 0u : (uint32_t)(e0 - row0 * w);
    float4 *p4 = reinterpret_cast<float4 *>(a.p[t]), *m4 = reinterpret_cast<float4 *>(a.m[t]), *v4 = reinterpret_cast<float4 *>(a.v[t]);
    const float4 *g4 = reinterpret_cast<const float4 *>(a.g[t]);
    const float sh = a.step_head[t], stl = a.step_tail[t], ib = a.inv_bc2_sqrt[t];
    const uint32_t split = a.split[t];
    const float one_minus_b1 = c.one_minus_b1, b2 = c.b2, one_minus_b2 = c.one_minus_b2, eps = c.eps;

    // per float4: which components lie in a visible row (bit e: component e) and, above them, the column of component 0
    uint32_t vis[kSparsePer];
#pragma unroll
    for (int k = 0; k < kSparsePer; ++k) {
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kSparseBlock;
        vis[k] = 0;
        if (i >= n4) continue;
        const uint32_t x = col0 + 4u * (threadIdx.x + (uint32_t)k * kSparseBlock);        // < w + 4096
        const uint32_t q = x / w, col = x - q * w;
        if (W == 1) {                                            // four rows, whose entries lie side by side
            vis[k] = rows_seen4(a, row0 + x);
        } else if (w >= 3) {                                     // four elements lie in at most two rows
            const bool over = col + 3 >= w;                      // ... the second one exists (and is < rows) exactly then
            const bool v0 = row_seen(a, row0 + q);
            const bool v1 = over ? row_seen(a, row0 + q + 1) : false;
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) vis[k] |= (uint32_t)(col + e >= w ? v1 : v0) << e;
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) vis[k] |= (uint32_t)row_seen(a, row0 + (x + e) / w) << e;
        }
        vis[k] |= col << 4;
    }
    float4 pp[kSparsePer], mm[kSparsePer], vv[kSparsePer], gg[kSparsePer];
#pragma unroll
    for (int k = 0; k < kSparsePer; ++k) {
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kSparseBlock;
        if (vis[k] & 15u) { pp[k] = p4[i]; mm[k] = m4[i]; vv[k] = v4[i]; gg[k] = g4[i]; }
    }
#pragma unroll
    for (int k = 0; k < kSparsePer; ++k) {
        if (!(vis[k] & 15u)) continue;
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kSparseBlock;
        float4 st = make_float4(sh, sh, sh, sh);
        if (split < w) {
            // the column of component e: col + e, less one or (w < 3) several rows
            auto pick = [&](uint32_t cc) { cc = w >= 3 ? (cc >= w ? cc - w : cc) : cc % w; return cc < split ? sh : stl; };
            const uint32_t col = vis[k] >> 4;
            st = make_float4(pick(col), pick(col + 1), pick(col + 2), pick(col + 3));
        }
        const float4 p0 = pp[k], m0 = mm[k], v0 = vv[k];
        // the statements of gsr_optim.hip's GSR_ADAM1: the two kernels are held to each other bit for bit.  The first and the third
        // contract in one way only.  The second, v b2 + (1 - b2) g g, has two (either product can become the addend), and under
        // -ffp-contract=fast the choice depends on the code around it: k_adam_multi's float4 body rounds v b2 and fuses the other
        // product, its trailing-element path does the opposite.  Written out here as each of them has it.
#define GSR_ADAM1(c)                                                                      \
        mm[k].c = mm[k].c + (gg[k].c - mm[k].c) * one_minus_b1;                           \
        vv[k].c = __builtin_fmaf(one_minus_b2 * gg[k].c, gg[k].c, vv[k].c * b2);          \
        pp[k].c = pp[k].c - st.c * (mm[k].c / (sqrtf(vv[k].c) * ib + eps));
        GSR_ADAM1(x) GSR_ADAM1(y) GSR_ADAM1(z) GSR_ADAM1(w)
#undef GSR_ADAM1
        if ((vis[k] & 15u) != 15u) {                                     // a float4 across a visible and a hidden row: the hidden part keeps its bits
#define GSR_KEEP(c, bit)                                                                  \
            if (!(vis[k] & (bit))) { pp[k].c = p0.c; mm[k].c = m0.c; vv[k].c = v0.c; }
            GSR_KEEP(x, 1u) GSR_KEEP(y, 2u) GSR_KEEP(z, 4u) GSR_KEEP(w, 8u)
#undef GSR_KEEP
        }
        p4[i] = pp[k]; m4[i] = mm[k]; v4[i] = vv[k];
    }
    // the tensor's last item also takes the n % 4 trailing elements
    if (first <= n4 && first + kSparseChunk > n4 && threadIdx.x < (unsigned)(n - n4 * 4)) {
        const unsigned long long i = n4 * 4 + threadIdx.x;
        const uint32_t x = col0 + (uint32_t)(i - e0);
        const uint32_t q = x / w, col = x - q * w;
        if (row_seen(a, row0 + q)) {
            float m1 = a.m[t][i], v1 = a.v[t][i];
            const float g1 = a.g[t][i];
            m1 = m1 + (g1 - m1) * one_minus_b1;
            v1 = __builtin_fmaf(v1, b2, one_minus_b2 * g1 * g1);          // (k_adam_multi's trailing elements: this product is the rounded one)
            const float st = col >= split ? stl : sh;
            a.p[t][i] = a.p[t][i] - st * (m1 / (sqrtf(v1) * ib + eps));
            a.m[t][i] = m1; a.v[t][i] = v1;
        }
    }
}

__global__ __launch_bounds__(kSparseBlock) void k_adam_sparse_multi(AdamSparse a, AdamConsts c)
{
    const unsigned long long items = a.item_end[a.count - 1];
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        int t = 0;
        while (t + 1 < a.count && it >= a.item_end[t]) ++t;            // block-uniform, never past the last tensor
        const unsigned long long first = (it - (t ? a.item_end[t - 1] : 0ull)) * kSparseChunk;     // float4 index inside tensor t
        switch (a.width[t]) {                                          // the widths of the model's tensors: [P,1] [P,3] [P,4] [P,M,3]
        case 1: adam_sparse_item<1>(a, t, first, c); break;
        case 3: adam_sparse_item<3>(a, t, first, c); break;
        case 4: adam_sparse_item<4>(a, t, first, c); break;
        case 12: adam_sparse_item<12>(a, t, first, c); break;
        case 27: adam_sparse_item<27>(a, t, first, c); break;
        case 48: adam_sparse_item<48>(a, t, first, c); break;
        default: adam_sparse_item<0>(a, t, first, c); break;
        }
    }
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_adam_step_sparse_multi(int32_t count, const gsr_adam_tensor *tensors, int64_t rows, const void *visible,
                                          int32_t visible_elem_bytes, float beta1, float beta2, float eps, void *stream)
{
    if (count < 0 || count > GSR_ADAM_MAX_TENSORS || (count > 0 && !tensors)) {
        set_error("gsr_adam_step_sparse_multi: 0 .. %d tensors", GSR_ADAM_MAX_TENSORS);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (rows < 0) {
        set_error("gsr_adam_step_sparse_multi: rows = %lld", (long long)rows);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (visible_elem_bytes != 1 && visible_elem_bytes != 4) {
        set_error("gsr_adam_step_sparse_multi: visible_elem_bytes = %d (1: bool / uint8 per row, 4: int32 radii per row)", visible_elem_bytes);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (rows > 0 && !visible) {
        set_error("gsr_adam_step_sparse_multi: visible is NULL for %lld rows", (long long)rows);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    AdamSparse a;
    a.count = 0;
    a.mask = visible; a.mask_bytes = visible_elem_bytes;
    unsigned long long items = 0;
    for (int i = 0; i < count; ++i) {
        const gsr_adam_tensor &t = tensors[i];
        if (t.step < 1) {
            set_error("gsr_adam_step_sparse_multi: tensor %d: step = %lld (step >= 1)", i, (long long)t.step);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (t.n < 0 || (rows == 0 && t.n != 0) || (rows > 0 && (t.n % rows != 0 || t.n / rows < 1 || t.n / rows > INT32_MAX))) {
            set_error("gsr_adam_step_sparse_multi: tensor %d: n = %lld is not rows = %lld times a width >= 1 (n %% rows != 0)", i,
                      (long long)t.n, (long long)rows);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (rows == 0) continue;
        const int64_t w = t.n / rows;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) {
            set_error("gsr_adam_step_sparse_multi: tensor %d: NULL pointer", i);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (t.row_len != 0 && (t.row_len != w || t.split < 0 || t.split > t.row_len)) {
            set_error("gsr_adam_step_sparse_multi: tensor %d: row_len = %d is neither 0 nor the width %lld, or split outside 0 .. row_len", i,
                      t.row_len, (long long)w);
            return GSR_ERR_INVALID_ARGUMENT;
        }
        const int k = a.count++;
        // GSR_ADAM_STEP_UNCORRECTED: no bias correction (upstream's sparse kernel applies none): both corrections are exactly 1
        const bool plain = t.step == GSR_ADAM_STEP_UNCORRECTED;
        const double bc1 = plain ? 1.0 : 1.0 - pow((double)beta1, (double)t.step), bc2 = plain ? 1.0 : 1.0 - pow((double)beta2, (double)t.step);
        a.p[k] = t.param; a.g[k] = t.grad; a.m[k] = t.exp_avg; a.v[k] = t.exp_avg_sq;
        a.n[k] = (unsigned long long)t.n;
        a.step_head[k] = (float)((double)t.lr / bc1); a.step_tail[k] = (float)((double)t.lr_tail / bc1);
        a.inv_bc2_sqrt[k] = (float)(1.0 / sqrt(bc2));
        a.width[k] = (uint32_t)w; a.split[k] = t.row_len ? (uint32_t)t.split : (uint32_t)w;
        items += ((unsigned long long)t.n / 4 + kSparseChunk - 1) / kSparseChunk;
        if (((unsigned long long)t.n / 4) % kSparseChunk == 0 && t.n % 4 != 0) items += 1;      // an item for the trailing elements alone
        a.item_end[k] = items;
    }
    if (a.count == 0) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long blocks = items < 16384 ? items : 16384;
    const AdamConsts c = {1.f - beta1, beta2, 1.f - beta2, eps};
    ProfileScope prof("adam_sparse", s);
    hipLaunchKernelGGL(k_adam_sparse_multi, dim3((unsigned)blocks), dim3(kSparseBlock), 0, s, a, c);
    GSR_LAUNCH_CHECK("adam_sparse", false, s);
    return GSR_OK;
}
