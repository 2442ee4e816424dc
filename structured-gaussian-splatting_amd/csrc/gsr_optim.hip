// gsr_optim.hip — SURVEY 8f row f1: the optimizer step of the reference's training loop (train.py:140-142,
// torch.optim.Adam with eps = 1e-15, scene/gaussian_model.py:159-177) as ONE pass over (param, grad, m, v) of every tensor:
// 16 B read + 12 B written per element, where the foreach implementation makes ~8 passes per tensor.  The rule of one element is
// adam_update (gsr_math.h); two kernels walk the same table of tensors: k_adam_multi steps every element, k_adam_sparse_multi the
// rows a frame saw.  They share the rule, the table, the work items and the choice of a column's learning rate, so a visible row
// of the sparse step is the dense step's row bit for bit.
#include "gsr_internal.h"

namespace gsr {

// Work item = kAdamChunk consecutive float4 of one tensor (a block walks items blockIdx.x, + gridDim.x, ...; each thread takes
// kAdamPer float4 of the item 256 apart: all of a thread's 4 kAdamPer loads are issued before the first store).  The tensor's last
// item also takes its n % 4 trailing elements.  Five launches of a one-tensor kernel left four kernel boundaries and four tails in
// a 0.35 ms step.
constexpr int kAdamBlock = 256;
constexpr int kAdamPer = 4;
constexpr int kAdamChunk = kAdamBlock * kAdamPer;            // float4 per work item

// Rows of `width` floats whose first `split` step with step_head and the rest with step_tail: the interleaved SH table [P, 16, 3]
// of this package's GaussianModel, where the reference keeps f_dc (lr = feature_lr) and f_rest (lr = feature_lr / 20) as two
// tensors (scene/gaussian_model.py:166-168).  split == width: one learning rate.  width == 0 (dense step only): a tensor without
// rows, one learning rate.
struct AdamTable {
    float *p[GSR_ADAM_MAX_TENSORS]; const float *g[GSR_ADAM_MAX_TENSORS]; float *m[GSR_ADAM_MAX_TENSORS]; float *v[GSR_ADAM_MAX_TENSORS];
    unsigned long long n[GSR_ADAM_MAX_TENSORS];
    unsigned long long item_end[GSR_ADAM_MAX_TENSORS];       // running count of work items; entries [count, ...) repeat the last
    float step_head[GSR_ADAM_MAX_TENSORS], step_tail[GSR_ADAM_MAX_TENSORS], inv_bc2_sqrt[GSR_ADAM_MAX_TENSORS];
    uint32_t width[GSR_ADAM_MAX_TENSORS], split[GSR_ADAM_MAX_TENSORS];
    const void *mask;                                        // sparse step: one entry per row
    int mask_bytes;                                          // 1: non-zero = visible; 4: int32 > 0 = visible
    int count;
};

// the tensor of work item `it` (block-uniform, <= 8 steps) and the item's first float4 inside it
__device__ __forceinline__ int adam_item(const AdamTable &a, unsigned long long it, unsigned long long &first)
{
    int t = 0;
    while (it >= a.item_end[t]) ++t;
    first = (it - (t ? a.item_end[t - 1] : 0ull)) * kAdamChunk;
    return t;
}

__device__ __forceinline__ void adam_update4(float4 &p, float4 &m, float4 &v, const float4 &g, const float st[4], float ib, const AdamConsts &c)
{
    adam_update(p.x, m.x, v.x, g.x, st[0], ib, c);
    adam_update(p.y, m.y, v.y, g.y, st[1], ib, c);
    adam_update(p.z, m.z, v.z, g.z, st[2], ib, c);
    adam_update(p.w, m.w, v.w, g.w, st[3], ib, c);
}

__global__ __launch_bounds__(kAdamBlock) void k_adam_multi(AdamTable a, AdamConsts c)
{
    const unsigned long long items = a.item_end[a.count - 1];
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        unsigned long long first;
        const int t = adam_item(a, it, first);
        const unsigned long long n = a.n[t], n4 = n / 4;
        float4 *p4 = reinterpret_cast<float4 *>(a.p[t]), *m4 = reinterpret_cast<float4 *>(a.m[t]), *v4 = reinterpret_cast<float4 *>(a.v[t]);
        const float4 *g4 = reinterpret_cast<const float4 *>(a.g[t]);
        const float sh = a.step_head[t], stl = a.step_tail[t], ib = a.inv_bc2_sqrt[t];
        const uint32_t row_len = a.width[t], split = a.split[t];             // row_len: 0 or >= 4
        float4 pp[kAdamPer], mm[kAdamPer], vv[kAdamPer], gg[kAdamPer];
#pragma unroll
        for (int k = 0; k < kAdamPer; ++k) {
            const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kAdamBlock;
            if (i < n4) { pp[k] = p4[i]; mm[k] = m4[i]; vv[k] = v4[i]; gg[k] = g4[i]; }
        }
#pragma unroll
        for (int k = 0; k < kAdamPer; ++k) {
            const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kAdamBlock;
            if (i >= n4) continue;
            float st[4] = {sh, sh, sh, sh};
            if (row_len) {
                const uint32_t col = (uint32_t)((i * 4) % row_len);
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) st[e] = adam_step_size(col + e, row_len, split, sh, stl, true);
            }
            adam_update4(pp[k], mm[k], vv[k], gg[k], st, ib, c);
            p4[i] = pp[k]; m4[i] = mm[k]; v4[i] = vv[k];
        }
        // The trailing elements take the rule of the float4 body.  (Written out beside it, their v' had fused the other product of
        // b2 v + ((1 - b2) g) g: one rounding apart, inside the same bound.)
        if (first <= n4 && first + kAdamChunk > n4 && threadIdx.x < (unsigned)(n - n4 * 4)) {
            const unsigned long long i = n4 * 4 + threadIdx.x;
            const float st = row_len ? adam_step_size((uint32_t)(i % row_len), row_len, split, sh, stl, true) : sh;
            adam_update(a.p[t][i], a.m[t][i], a.v[t][i], a.g[t][i], st, ib, c);
        }
    }
}

// ---- the same step over the rows a frame saw (upstream's optimizer_type = "sparse_adam": a Gaussian with radii <= 0 has an exactly
// zero gradient, and its parameter and both moments keep their bits).  Every tensor of the step has the same number of rows; ONE
// per-row mask governs the launch.  Per element of a hidden row: nothing is read but the row's mask entry.
//
// A thread decides per float4 from the mask entries of the (at most two, for width >= 3) rows under it: all hidden -> no load and no
// store; partly hidden -> loaded, the hidden components stored back as they were.  There is no vote: a wave whose 64 float4 are
// hidden skips the loads on its empty exec mask.
//
// The row of an element: ONE 64-bit division per work item (block-uniform: row and column of the item's first element), then a
// 32-bit division of an offset < width + 4096 by the width, which is a compile-time constant for the widths of the model's
// tensors (1, 3, 4 and 3 M for M = 4, 9, 16: a multiply-high and a shift).  Any other width takes the run-time divisions.
__device__ __forceinline__ bool row_seen(const AdamTable &a, unsigned long long r)
{
    return a.mask_bytes == 1 ? static_cast<const uint8_t *>(a.mask)[r] != 0 : static_cast<const int32_t *>(a.mask)[r] > 0;
}

// the entries of rows r .. r + 3 as bits 0 .. 3: one load (the compiler words the copy for the alignment it may assume)
__device__ __forceinline__ uint32_t rows_seen4(const AdamTable &a, unsigned long long r)
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
__device__ __forceinline__ void adam_sparse_item(const AdamTable &a, const int t, const unsigned long long first, const AdamConsts &c)
{
    const uint32_t w = W ? (uint32_t)W : a.width[t];
    const unsigned long long n = a.n[t], n4 = n / 4;
    // row and column of the item's first element.  An item starts at a multiple of 4096 elements: column 0 where w divides that
    const unsigned long long e0 = first * 4;
    const unsigned long long row0 = e0 / w;
    const uint32_t col0 = (W && (4 * kAdamChunk) % (W ? W : 1) == 0) ? 0u : (uint32_t)(e0 - row0 * w);
    float4 *p4 = reinterpret_cast<float4 *>(a.p[t]), *m4 = reinterpret_cast<float4 *>(a.m[t]), *v4 = reinterpret_cast<float4 *>(a.v[t]);
    const float4 *g4 = reinterpret_cast<const float4 *>(a.g[t]);
    const float sh = a.step_head[t], stl = a.step_tail[t], ib = a.inv_bc2_sqrt[t];
    const uint32_t split = a.split[t];

    // per float4: which components lie in a visible row (bit e: component e) and, above them, the column of component 0
    uint32_t vis[kAdamPer];
#pragma unroll
    for (int k = 0; k < kAdamPer; ++k) {
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kAdamBlock;
        vis[k] = 0;
        if (i >= n4) continue;
        const uint32_t x = col0 + 4u * (threadIdx.x + (uint32_t)k * kAdamBlock);          // < w + 4096
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
    float4 pp[kAdamPer], mm[kAdamPer], vv[kAdamPer], gg[kAdamPer];
#pragma unroll
    for (int k = 0; k < kAdamPer; ++k) {
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kAdamBlock;
        if (vis[k] & 15u) { pp[k] = p4[i]; mm[k] = m4[i]; vv[k] = v4[i]; gg[k] = g4[i]; }
    }
#pragma unroll
    for (int k = 0; k < kAdamPer; ++k) {
        if (!(vis[k] & 15u)) continue;
        const unsigned long long i = first + threadIdx.x + (unsigned long long)k * kAdamBlock;
        float st[4] = {sh, sh, sh, sh};
        if (split < w) {
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e) st[e] = adam_step_size((vis[k] >> 4) + e, w, split, sh, stl, w >= 3);
        }
        const float4 p0 = pp[k], m0 = mm[k], v0 = vv[k];
        adam_update4(pp[k], mm[k], vv[k], gg[k], st, ib, c);
        if ((vis[k] & 15u) != 15u) {                                     // a float4 across a visible and a hidden row: the hidden part keeps its bits
#define GSR_KEEP(c, bit)                                                                  \
            if (!(vis[k] & (bit))) { pp[k].c = p0.c; mm[k].c = m0.c; vv[k].c = v0.c; }
            GSR_KEEP(x, 1u) GSR_KEEP(y, 2u) GSR_KEEP(z, 4u) GSR_KEEP(w, 8u)
#undef GSR_KEEP
        }
        p4[i] = pp[k]; m4[i] = mm[k]; v4[i] = vv[k];
    }
    // the trailing elements, by the rule of the float4 body as in k_adam_multi
    if (first <= n4 && first + kAdamChunk > n4 && threadIdx.x < (unsigned)(n - n4 * 4)) {
        const unsigned long long i = n4 * 4 + threadIdx.x;
        const uint32_t x = col0 + (uint32_t)(i - e0);
        const uint32_t q = x / w, col = x - q * w;
        if (row_seen(a, row0 + q))
            adam_update(a.p[t][i], a.m[t][i], a.v[t][i], a.g[t][i], adam_step_size(col, w, split, sh, stl, true), ib, c);
    }
}

__global__ __launch_bounds__(kAdamBlock) void k_adam_sparse_multi(AdamTable a, AdamConsts c)
{
    const unsigned long long items = a.item_end[a.count - 1];
    for (unsigned long long it = blockIdx.x; it < items; it += gridDim.x) {
        unsigned long long first;
        const int t = adam_item(a, it, first);
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

// ---- densification bookkeeping of one training iteration (train.py:127-130 + scene/gaussian_model.py:415-417):
//   max_radii2D[vis] = max(max_radii2D[vis], radii[vis]);  xyz_gradient_accum[vis] += |viewspace grad.xy|;  denom[vis] += 1
// with vis = radii > 0.  One pass and no host synchronisation, where boolean-mask indexing costs four nonzero()
// compactions (each a device->host size readback) and ~20 kernels.
__global__ __launch_bounds__(256) void k_densify_stats(int P, const int32_t *__restrict__ radii, const float *__restrict__ vs_grad,
                                                       float *__restrict__ max_radii2D, float *__restrict__ grad_accum,
                                                       float *__restrict__ denom)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const int r = radii[i];
    if (r <= 0) return;
    max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
    const float gx = vs_grad[3 * (size_t)i], gy = vs_grad[3 * (size_t)i + 1];
    grad_accum[i] += sqrtf(gx * gx + gy * gy);
    denom[i] += 1.f;
}

// One launch of `kernel` over the C ABI's array.  width_of(i, t) is the entry point's own test of tensor i: its floats per row (0: a
// tensor without rows), or a negative value after set_error.  A tensor with n == 0 takes no entry.
template <class WidthOf>
static int adam_launch(void (*kernel)(AdamTable, AdamConsts), const char *who, const char *profile_name, int32_t count,
                       const gsr_adam_tensor *tensors, const void *mask, int mask_bytes, float beta1, float beta2, float eps, void *stream,
                       WidthOf width_of)
{
    if (count < 0 || count > GSR_ADAM_MAX_TENSORS || (count > 0 && !tensors)) {
        set_error("%s: 0 .. %d tensors", who, GSR_ADAM_MAX_TENSORS);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    AdamTable a;
    a.count = 0;
    a.mask = mask; a.mask_bytes = mask_bytes;
    unsigned long long items = 0;
    for (int i = 0; i < count; ++i) {
        const gsr_adam_tensor &t = tensors[i];
        const int64_t w = width_of(i, t);
        if (w < 0) return GSR_ERR_INVALID_ARGUMENT;
        if (t.n == 0) continue;
        const int k = a.count++;
        // GSR_ADAM_STEP_UNCORRECTED: no bias correction (upstream's sparse kernel applies none): both corrections are exactly 1
        const bool plain = t.step == GSR_ADAM_STEP_UNCORRECTED;
        const double bc1 = plain ? 1.0 : 1.0 - pow((double)beta1, (double)t.step), bc2 = plain ? 1.0 : 1.0 - pow((double)beta2, (double)t.step);
        a.p[k] = t.param; a.g[k] = t.grad; a.m[k] = t.exp_avg; a.v[k] = t.exp_avg_sq;
        a.n[k] = (unsigned long long)t.n;
        a.step_head[k] = (float)((double)t.lr / bc1); a.step_tail[k] = (float)((double)t.lr_tail / bc1);
        a.inv_bc2_sqrt[k] = (float)(1.0 / sqrt(bc2));
        a.width[k] = (uint32_t)w; a.split[k] = t.row_len ? (uint32_t)t.split : (uint32_t)w;
        items += ((unsigned long long)t.n / 4 + kAdamChunk - 1) / kAdamChunk;
        if (((unsigned long long)t.n / 4) % kAdamChunk == 0 && t.n % 4 != 0) items += 1;        // an item for the trailing elements alone
        a.item_end[k] = items;
    }
    if (a.count == 0) return GSR_OK;
    for (int k = a.count; k < GSR_ADAM_MAX_TENSORS; ++k) a.item_end[k] = items;                  // adam_item's search ends there at the latest
    hipStream_t s = (hipStream_t)stream;
    const unsigned long long blocks = items < 16384 ? items : 16384;
    const AdamConsts c = {1.f - beta1, beta2, 1.f - beta2, eps};
    ProfileScope prof(profile_name, s);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kAdamBlock), 0, s, a, c);
    GSR_LAUNCH_CHECK(profile_name, false, s);
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" int gsr_densify_stats(int32_t P, const int32_t *radii, const float *viewspace_grad, float *max_radii2D,
                                 float *xyz_gradient_accum, float *denom, void *stream)
{
    if (P < 0 || (P > 0 && (!radii || !viewspace_grad || !max_radii2D || !xyz_gradient_accum || !denom))) {
        set_error("gsr_densify_stats: bad argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    hipStream_t s = (hipStream_t)stream;
    ProfileScope prof("densify_stats", s);
    hipLaunchKernelGGL(k_densify_stats, dim3((P + 255) / 256), dim3(256), 0, s, P, radii, viewspace_grad, max_radii2D,
                       xyz_gradient_accum, denom);
    GSR_LAUNCH_CHECK("densify_stats", false, s);
    return GSR_OK;
}

extern "C" int gsr_adam_step_multi(int32_t count, const gsr_adam_tensor *tensors, float beta1, float beta2, float eps, void *stream)
{
    return adam_launch(k_adam_multi, "gsr_adam_step_multi", "adam", count, tensors, nullptr, 0, beta1, beta2, eps, stream,
                       [](int i, const gsr_adam_tensor &t) -> int64_t {
        if (t.n < 0 || t.step < 1 || (t.n > 0 && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) ||
            (t.row_len != 0 && (t.row_len < 4 || t.split < 0 || t.split > t.row_len || t.n % t.row_len != 0))) {
            set_error("gsr_adam_step_multi: bad tensor %d (row_len 0 or >= 4 and dividing n, 0 <= split <= row_len, step >= 1)", i);
            return -1;
        }
        return t.row_len;
    });
}

// The one-tensor calls are gsr_adam_step_multi with a table of one entry.
extern "C" int gsr_adam_step(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float lr, float beta1,
                             float beta2, float eps, int64_t step, void *stream)
{
    if (n < 0 || step < 1 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) {
        set_error("gsr_adam_step: bad argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const gsr_adam_tensor t = {param, grad, exp_avg, exp_avg_sq, n, lr, lr, step, 0, 0};
    return gsr_adam_step_multi(1, &t, beta1, beta2, eps, stream);
}

extern "C" int gsr_adam_step_split(int64_t rows, int32_t row_len, int32_t split, float *param, const float *grad, float *exp_avg,
                                   float *exp_avg_sq, float lr_head, float lr_tail, float beta1, float beta2, float eps, int64_t step,
                                   void *stream)
{
    if (rows < 0 || step < 1 || row_len < 4 || split < 0 || split > row_len ||
        (rows > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) {
        set_error("gsr_adam_step_split: bad argument (row_len >= 4, 0 <= split <= row_len)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const gsr_adam_tensor t = {param, grad, exp_avg, exp_avg_sq, rows * row_len, lr_head, lr_tail, step, row_len, split};
    return gsr_adam_step_multi(1, &t, beta1, beta2, eps, stream);
}

extern "C" int gsr_adam_step_sparse_multi(int32_t count, const gsr_adam_tensor *tensors, int64_t rows, const void *visible,
                                          int32_t visible_elem_bytes, float beta1, float beta2, float eps, void *stream)
{
    const char *who = "gsr_adam_step_sparse_multi";
    if (rows < 0) {
        set_error("%s: rows = %lld", who, (long long)rows);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (visible_elem_bytes != 1 && visible_elem_bytes != 4) {
        set_error("%s: visible_elem_bytes = %d (1: bool / uint8 per row, 4: int32 radii per row)", who, visible_elem_bytes);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (rows > 0 && !visible) {
        set_error("%s: visible is NULL for %lld rows", who, (long long)rows);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return adam_launch(k_adam_sparse_multi, who, "adam_sparse", count, tensors, visible, visible_elem_bytes, beta1, beta2, eps, stream,
                       [=](int i, const gsr_adam_tensor &t) -> int64_t {
        if (t.step < 1) {
            set_error("%s: tensor %d: step = %lld (step >= 1)", who, i, (long long)t.step);
            return -1;
        }
        if (t.n < 0 || (rows == 0 && t.n != 0) || (rows > 0 && (t.n % rows != 0 || t.n / rows < 1 || t.n / rows > INT32_MAX))) {
            set_error("%s: tensor %d: n = %lld is not rows = %lld times a width >= 1 (n %% rows != 0)", who, i, (long long)t.n, (long long)rows);
            return -1;
        }
        if (rows == 0) return 0;
        const int64_t w = t.n / rows;
        if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq) {
            set_error("%s: tensor %d: NULL pointer", who, i);
            return -1;
        }
        if (t.row_len != 0 && (t.row_len != w || t.split < 0 || t.split > t.row_len)) {
            set_error("%s: tensor %d: row_len = %d is neither 0 nor the width %lld, or split outside 0 .. row_len", who, i, t.row_len, (long long)w);
            return -1;
        }
        return w;
    });
}
