// gsr_vq.hip — vector quantisation of a [P, D] table against a [K, D] codebook (include/gsrast.h gsr_vq_*): Lloyd's assignment
// step as a fused GEMM + argmin, and the centroid update as a stable sort + one wave per code.  DESIGN.md §18.
//
// ASSIGN.  score(p, k) = |c_k|^2 - 2 x_p . c_k, one fmaf of the dot product and the code's norm; idx[p] = the lowest k of the
// smallest score, dist2[p] = max(0, |x_p|^2 + score).  The dot products are v_mfma_f32_32x32x2_f32: exact binary32, bit for bit a
// k-ascending fmaf chain from 0 (D zero-padded: a padded step adds 0 * 0).  Both norms are the same chain of the row with itself
// (row_norm2), so that a point equal to a code has dot == |x|^2 == |c|^2 bit for bit and dist2 == 0.
// CODES ON THE ROWS (operand A), POINTS ON THE LANE (operand B): a 32x32 accumulator has its column on the lane (lane & 31) and
// its rows in the 16 registers, row(r, h) = (r & 3) + 8 (r >> 2) + 4 h with h = lane >> 5.  A lane therefore sees 16 codes of each
// code tile for ITS point, in ascending code index, and keeps the running (min, argmin) in two registers with a strict <; the two
// half-waves (rows 4 h .. of every group of 8) are merged once at the end, ties to the lower index.  The P x K matrix exists only
// as accumulator registers.
// A wave owns kVqTiles = 2 tiles of 32 points; a point's inputs stay in registers (k = 2 t + h of step t: STEPS registers per tile)
// across the whole codebook.  A block of four waves stages kStage codes at a time in LDS, each code's row split into its even-k and
// odd-k halves ([h][t]) so that a lane reads four consecutive steps of its code with one ds_read_b128; the row stride 2 STEPS + 4
// floats is an odd number of 16-byte slots, which spreads the 16 lanes of every ds_read_b128 group over the 16 slots of the bank row.
// The kernel is instantiated for STEPS in {4, 8, 16, 24, 32, 48, 64}: D <= 2 STEPS picks the smallest.
//
// UPDATE.  (idx[p], p) pairs go through the library's stable radix sort: each code's members then lie in one run, in ascending point
// index.  k_vq_runs marks where every run starts and ends (plain stores: one position per code qualifies), and one wave per code
// adds its members' rows one after the other in that order (lane = column; sixteen row loads in flight), divides by the count, or
// copies the previous row when there is no member.  From P >= 64 K on a code gets four waves, one per quarter of its run, and the
// quarters are added as (q0 + q1) + (q2 + q3).  No floating-point atomics, no scan over floats: the same inputs give the same bits.
#include <math.h>

#include "gsr_internal.h"

namespace gsr {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kVqMaxD = 128;
constexpr int kVqWaves = 4, kVqBlock = 64 * kVqWaves;
constexpr int kVqTiles = 2;                                   // 32-point tiles per wave
constexpr int kVqBlockPoints = kVqWaves * kVqTiles * 32;
constexpr int64_t kVqMaxP = (int64_t)1 << 30;
constexpr int kVqMaxK = 1 << 30;
constexpr int kVqLongRun = 64;                              // members per code, on average, from which a code gets a block of its own
constexpr int kVqInFlight = 16;                              // member rows a wave of the update loads before it adds them

#define GSR_VQ_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

template <int STEPS> struct VqLayout {
    static_assert(STEPS % 4 == 0, "a lane reads four steps per ds_read_b128, and the stride must be an odd number of 16-byte slots");
    static constexpr int kStride = 2 * STEPS + 4;             // floats per code row in LDS
    static constexpr int kStage = STEPS > 32 ? 64 : 128;      // codes per stage: <= 34 KB of LDS, several blocks per CU
};

// |row|^2 as the k-ascending fmaf chain from 0: what the MFMA computes for the product of the row with itself
__device__ __forceinline__ float row_norm2(const float *__restrict__ row, int D)
{
    float n = 0.f;
    for (int k = 0; k < D; ++k) { const float v = row[k]; n = fmaf(v, v, n); }
    return n;
}

__global__ __launch_bounds__(256) void k_vq_code_norms(int K, int D, const float *__restrict__ cb, float *__restrict__ cnorm)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) cnorm[k] = row_norm2(cb + (int64_t)k * D, D);
}

template <int STEPS>
__global__ __launch_bounds__(kVqBlock) void k_vq_assign(int64_t P, int K, int D, const float *__restrict__ x, const float *__restrict__ cb,
                                                        const float *__restrict__ cnorm, int32_t *__restrict__ idx, float *__restrict__ dist2)
{
    constexpr int S = VqLayout<STEPS>::kStride, KT = VqLayout<STEPS>::kStage;
    static_assert(kVqTiles == 2, "the epilogue gives tile h to half-wave h");
    static_assert(KT % 32 == 0 && KT <= kVqBlock, "whole code tiles; one thread per staged norm");
    __shared__ __attribute__((aligned(16))) float codes[KT * S];
    __shared__ __attribute__((aligned(16))) float cn[KT];
    const int lane = threadIdx.x & 63, c = lane & 31, h = lane >> 5, w = threadIdx.x >> 6;
    const int64_t p0 = ((int64_t)blockIdx.x * kVqWaves + w) * (32 * kVqTiles);       // no wave leaves early: the MFMAs and barriers need all

    float xb[kVqTiles][STEPS];
#pragma unroll
    for (int nt = 0; nt < kVqTiles; ++nt) {
        const int64_t p = p0 + nt * 32 + c;
#pragma unroll
        for (int t = 0; t < STEPS; ++t) {
            const int k = 2 * t + h;
            xb[nt][t] = p < P && k < D ? x[p * D + k] : 0.f;
        }
    }
    float best[kVqTiles];
    int bi[kVqTiles];
#pragma unroll
    for (int nt = 0; nt < kVqTiles; ++nt) { best[nt] = INFINITY; bi[nt] = 0; }

    for (int k0 = 0; k0 < K; k0 += KT) {
        __syncthreads();                                      // the previous stage has been read
        for (int e = threadIdx.x; e < KT * 2 * STEPS; e += kVqBlock) {
            const int j = e / (2 * STEPS), k = e % (2 * STEPS);
            const float v = j < K - k0 && k < D ? cb[(int64_t)(k0 + j) * D + k] : 0.f;
            codes[j * S + (k & 1) * STEPS + (k >> 1)] = v;
        }
        if ((int)threadIdx.x < KT) cn[threadIdx.x] = (int)threadIdx.x < K - k0 ? cnorm[k0 + threadIdx.x] : INFINITY;    // a padded code never wins
        __syncthreads();
        const int ntile = (min(KT, K - k0) + 31) / 32;        // (block-uniform)
        for (int tile = 0; tile < ntile; ++tile) {
            f32x16 acc[kVqTiles];
#pragma unroll
            for (int nt = 0; nt < kVqTiles; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
            const float *row = codes + (tile * 32 + c) * S + h * STEPS;
#pragma unroll
            for (int g = 0; g < STEPS / 4; ++g) {
                const float4 a = *reinterpret_cast<const float4 *>(row + 4 * g);
#pragma unroll
                for (int nt = 0; nt < kVqTiles; ++nt) {
                    acc[nt] = GSR_VQ_MFMA(a.x, xb[nt][4 * g + 0], acc[nt]);
                    acc[nt] = GSR_VQ_MFMA(a.y, xb[nt][4 * g + 1], acc[nt]);
                    acc[nt] = GSR_VQ_MFMA(a.z, xb[nt][4 * g + 2], acc[nt]);
                    acc[nt] = GSR_VQ_MFMA(a.w, xb[nt][4 * g + 3], acc[nt]);
                }
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {                     // registers 4 g .. 4 g + 3: codes 8 g + 4 h .. + 3 of the tile, ascending
                const float4 n4 = *reinterpret_cast<const float4 *>(cn + tile * 32 + 8 * g + 4 * h);
                const float nn[4] = {n4.x, n4.y, n4.z, n4.w};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int code = k0 + tile * 32 + 8 * g + 4 * h + i;
#pragma unroll
                    for (int nt = 0; nt < kVqTiles; ++nt) {
                        const float s = fmaf(-2.f, acc[nt][4 * g + i], nn[i]);
                        if (s < best[nt]) { best[nt] = s; bi[nt] = code; }
                    }
                }
            }
        }
    }

    // the other half-wave saw the other 16 codes of every tile for the same points; then half-wave h finishes tile h
    float mine = 0.f;
    int mine_i = 0;
#pragma unroll
    for (int nt = 0; nt < kVqTiles; ++nt) {
        const float ob = __shfl_xor(best[nt], 32);
        const int oi = __shfl_xor(bi[nt], 32);
        const bool take = ob < best[nt] || (ob == best[nt] && oi < bi[nt]);
        const float b = take ? ob : best[nt];
        const int i = take ? oi : bi[nt];
        if (nt == h) { mine = b; mine_i = i; }
    }
    const int64_t p = p0 + h * 32 + c;
    if (p < P) {
        idx[p] = mine_i;
        dist2[p] = fmaxf(row_norm2(x + p * D, D) + mine, 0.f);
    }
}

// keys = the code (K for an index outside [0, K): such a point is no one's member), vals = the point
__global__ __launch_bounds__(256) void k_vq_keys(uint32_t P, int K, const int32_t *__restrict__ idx, uint32_t *__restrict__ keys,
                                                 uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P) return;
    const uint32_t k = (uint32_t)idx[i];
    keys[i] = k < (uint32_t)K ? k : (uint32_t)K;
    vals[i] = i;
}

// runs[k] = first sorted position of code k, runs[K + 1 + k] = one past its last (both stay 0 for a code without members)
__global__ __launch_bounds__(256) void k_vq_runs(uint32_t P, int K, const uint32_t *__restrict__ keys, uint32_t *__restrict__ runs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= P) return;
    const uint32_t k = keys[i];
    if (i == 0 || keys[i - 1] != k) runs[k] = i;
    if (i == P - 1 || keys[i + 1] != k) runs[(uint32_t)K + 1u + k] = i + 1u;
}

// WAVES waves per code, lane = column (two columns per lane past 64).  WAVES = 1 (four codes per block): the code's members' rows in
// ascending point index, one add each.  WAVES = 4 (one code per block, for long runs): the run is cut into four quarters of
// ceil(n / 4) members, wave w adds quarter w the same way, and the code's sum is (q0 + q1) + (q2 + q3).
template <int WAVES>
__global__ __launch_bounds__(256) void k_vq_means(int K, int D, const float *__restrict__ x, const uint32_t *__restrict__ members,
                                                  const uint32_t *__restrict__ runs, const float *cb, float *out, int32_t *__restrict__ counts)
{
    static_assert(WAVES == 1 || WAVES == 4, "a block is four waves");
    __shared__ float part[WAVES == 4 ? 4 * kVqMaxD : 1];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = WAVES == 4 ? (int)blockIdx.x : (int)blockIdx.x * 4 + w;
    if (j >= K) return;                                       // (WAVES = 4: the grid is K blocks, no block leaves)
    const uint32_t b = runs[j], e = runs[(uint32_t)K + 1u + j], n = e - b;
    if (threadIdx.x == (WAVES == 4 ? 0 : w * 64)) counts[j] = (int32_t)n;
    uint32_t lo = b, hi = e;
    if (WAVES == 4) {
        const uint32_t q = (n + 3u) / 4u;
        lo = min(b + (uint32_t)w * q, e);
        hi = min(lo + q, e);
    }
    for (int d = lane; d < D; d += 64) {
        const int64_t at = (int64_t)j * D + d;
        float s = 0.f;
        for (uint32_t i = lo; i < hi; i += kVqInFlight) {
            float v[kVqInFlight];
#pragma unroll
            for (int u = 0; u < kVqInFlight; ++u) v[u] = i + u < hi ? x[(int64_t)members[i + u] * D + d] : 0.f;
#pragma unroll
            for (int u = 0; u < kVqInFlight; ++u) if (i + u < hi) s += v[u];
        }
        if (WAVES == 4) part[w * kVqMaxD + d] = s;
        else out[at] = n ? s / (float)n : cb[at];
    }
    if (WAVES == 4) {
        __syncthreads();
        for (int d = threadIdx.x; d < D; d += 256) {
            const int64_t at = (int64_t)j * D + d;
            const float s = (part[d] + part[kVqMaxD + d]) + (part[2 * kVqMaxD + d] + part[3 * kVqMaxD + d]);
            out[at] = n ? s / (float)n : cb[at];
        }
    }
}

struct VqWS { float *cnorm; uint32_t *keys[2], *vals[2], *runs; void *radix_temp; size_t total; };

static VqWS carve_vq(void *base, int64_t P, int K)
{
    char *b = (char *)base;
    size_t o = 0;
    const size_t Pn = P > 0 ? (size_t)P : 1;
    VqWS w;
    w.cnorm = (float *)(b + o); o += align_up((size_t)K * 4);
    for (int i = 0; i < 2; ++i) { w.keys[i] = (uint32_t *)(b + o); o += align_up(Pn * 4); }
    for (int i = 0; i < 2; ++i) { w.vals[i] = (uint32_t *)(b + o); o += align_up(Pn * 4); }
    w.runs = (uint32_t *)(b + o); o += align_up(2 * ((size_t)K + 1) * 4);
    w.radix_temp = b + o; o += radix_temp_bytes();
    w.total = o;
    return w;
}

template <int STEPS>
static void launch_assign(int64_t P, int K, int D, const float *x, const float *cb, const float *cnorm, int32_t *idx, float *dist2, hipStream_t s)
{
    const unsigned blocks = (unsigned)((P + kVqBlockPoints - 1) / kVqBlockPoints);
    hipLaunchKernelGGL(k_vq_assign<STEPS>, dim3(blocks), dim3(kVqBlock), 0, s, P, K, D, x, cb, cnorm, idx, dist2);
}

}  // namespace gsr

using namespace gsr;

static int validate_vq(const char *who, int64_t P, int32_t K, int32_t D)
{
    if (D < 1 || D > kVqMaxD) { set_error("%s: D = %d must be in [1, %d]", who, D, kVqMaxD); return GSR_ERR_INVALID_ARGUMENT; }
    if (K < 1 || K > kVqMaxK) { set_error("%s: K = %d must be in [1, 2^30]", who, K); return GSR_ERR_INVALID_ARGUMENT; }
    if (P < 0 || P > kVqMaxP) { set_error("%s: P = %lld must be in [0, 2^30]", who, (long long)P); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int validate_vq_workspace(const char *who, int64_t P, int32_t K, const void *workspace, size_t workspace_bytes)
{
    const size_t need = carve_vq(nullptr, P, K).total;
    if (!workspace || workspace_bytes < need) {
        set_error("%s: workspace of %zu bytes, %zu needed (gsr_vq_workspace_size)", who, workspace ? workspace_bytes : (size_t)0, need);
        return GSR_ERR_WORKSPACE;
    }
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) { set_error("%s: workspace must be 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

extern "C" int gsr_vq_workspace_size(int64_t P, int32_t K, int32_t D, size_t *bytes)
{
    const char *who = "gsr_vq_workspace_size";
    if (int rc = validate_vq(who, P, K, D)) return rc;
    if (!bytes) { set_error("%s: bytes is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = carve_vq(nullptr, P, K).total;
    return GSR_OK;
}

extern "C" int gsr_vq_assign(int64_t P, int32_t K, int32_t D, const float *x, const float *codebook, int32_t *idx, float *dist2,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gsr_vq_assign";
    if (int rc = validate_vq(who, P, K, D)) return rc;
    if (P == 0) return GSR_OK;
    if (!x) { set_error("%s: x is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!codebook) { set_error("%s: codebook is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!idx) { set_error("%s: idx is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!dist2) { set_error("%s: dist2 is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = validate_vq_workspace(who, P, K, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const VqWS ws = carve_vq(workspace, P, K);
    {
        ProfileScope prof("vq_code_norms", s);
        hipLaunchKernelGGL(k_vq_code_norms, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, K, D, codebook, ws.cnorm);
        GSR_LAUNCH_CHECK("vq_code_norms", false, s);
    }
    ProfileScope prof("vq_assign", s);
    const int steps = (D + 1) / 2;
    if (steps <= 4) launch_assign<4>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else if (steps <= 8) launch_assign<8>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else if (steps <= 16) launch_assign<16>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else if (steps <= 24) launch_assign<24>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else if (steps <= 32) launch_assign<32>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else if (steps <= 48) launch_assign<48>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    else launch_assign<64>(P, K, D, x, codebook, ws.cnorm, idx, dist2, s);
    GSR_LAUNCH_CHECK("vq_assign", false, s);
    return GSR_OK;
}

extern "C" int gsr_vq_update(int64_t P, int32_t K, int32_t D, const float *x, const int32_t *idx, const float *codebook,
                             float *new_codebook, int32_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    const char *who = "gsr_vq_update";
    if (int rc = validate_vq(who, P, K, D)) return rc;
    if (P > 0 && !x) { set_error("%s: x is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (P > 0 && !idx) { set_error("%s: idx is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!codebook) { set_error("%s: codebook is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!new_codebook) { set_error("%s: new_codebook is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!counts) { set_error("%s: counts is NULL", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (int rc = validate_vq_workspace(who, P, K, workspace, workspace_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const VqWS ws = carve_vq(workspace, P, K);
    GSR_HIP_CHECK(hipMemsetAsync(ws.runs, 0, 2 * ((size_t)K + 1) * 4, s));
    int result = 0;
    if (P > 0) {
        const unsigned grid = (unsigned)((P + 255) / 256);
        hipLaunchKernelGGL(k_vq_keys, dim3(grid), dim3(256), 0, s, (uint32_t)P, K, idx, ws.keys[0], ws.vals[0]);
        GSR_LAUNCH_CHECK("vq_keys", false, s);
        if (int rc = launch_radix_sort<uint32_t>(ws.keys, ws.vals, nullptr, (uint32_t)P, (uint64_t)P, nullptr, 0, bit_width((uint32_t)K),
                                                 ws.radix_temp, &result, "vq_sort", false, s))
            return rc;
        hipLaunchKernelGGL(k_vq_runs, dim3(grid), dim3(256), 0, s, (uint32_t)P, K, ws.keys[result], ws.runs);
        GSR_LAUNCH_CHECK("vq_runs", false, s);
    }
    ProfileScope prof("vq_means", s);
    if (P >= (int64_t)kVqLongRun * K)                          // a function of the shape alone: the order of a sum never depends on the data
        hipLaunchKernelGGL(k_vq_means<4>, dim3((unsigned)K), dim3(256), 0, s, K, D, x, ws.vals[result], ws.runs, codebook, new_codebook, counts);
    else
        hipLaunchKernelGGL(k_vq_means<1>, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s, K, D, x, ws.vals[result], ws.runs, codebook,
                           new_codebook, counts);
    GSR_LAUNCH_CHECK("vq_means", false, s);
    return GSR_OK;
}
