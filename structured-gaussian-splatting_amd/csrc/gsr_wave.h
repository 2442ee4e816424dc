// gsr_wave.h — the wave- and block-level integer idioms of the pipeline between preprocess and blend (gsr_select.hip,
// gsr_sort.hip, gsr_binning.hip), written once: scan, reduction, a block's slice of a range, the counters in front of a block,
// one round of a stable partition.  Device code only.
//
// BARRIER CONTRACT (block_incl_scan, block_incl_scan_walk, partition_round): a helper contains exactly the barriers between ITS OWN stores to the LDS
// it is handed and its own reads of them.  The reuse hazard belongs to the caller: every thread's reads of a previous call on
// the same LDS must be behind a barrier before the next call stores to it.  A call site that needs a barrier of its own for
// that says so in a comment naming the barrier; a site without such a comment uses its LDS once.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gsr {

constexpr int kWave = 64;                 // CDNA wavefront

// the value `off` lanes below; a scanned type of several words supplies its own overload (Triple, gsr_select.hip)
__device__ __forceinline__ uint32_t lane_up(uint32_t v, int off) { return __shfl_up(v, off); }
__device__ __forceinline__ unsigned long long lane_up(unsigned long long v, int off) { return __shfl_up(v, off); }

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v)
{
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const T t = lane_up(v, off);
        if (lane >= off) v = v + t;
    }
    return v;
}

// every lane receives the result
template <typename T>
__device__ __forceinline__ T wave_sum(T v)
{
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <typename T>
__device__ __forceinline__ T wave_max(T v)
{
#pragma unroll
    for (int off = kWave / 2; off >= 1; off >>= 1) { const T u = __shfl_xor(v, off); v = u > v ? u : v; }
    return v;
}

// Inclusive scan of one value per thread over a block of waves, through the waves' totals in sh_wave[waves of the block].
// One barrier: between the store of the waves' totals and their read (the contract above).
template <typename T>
__device__ __forceinline__ T block_scan_wave_totals(T v, T *sh_wave)      // the wave's inclusive values; sh_wave is published
{
    const T inc = wave_incl_scan(v);
    if ((threadIdx.x & (kWave - 1)) == kWave - 1) sh_wave[threadIdx.x >> 6] = inc;
    __syncthreads();
    return inc;
}

// total = the block's sum, in every thread; NW = waves of the block
template <int NW, typename T>
__device__ __forceinline__ T block_incl_scan(T v, T *sh_wave, T &total)
{
    const int w = threadIdx.x >> 6;
    const T inc = block_scan_wave_totals(v, sh_wave);
    T base{}, tot{};
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const T s = sh_wave[i];
        if (i < w) base = base + s;
        tot = tot + s;
    }
    total = tot;
    return inc + base;
}

// The same scan without the total, WALKING: a wave reads the totals in front of it only, one after the other, so it holds one
// of them at a time where block_incl_scan holds all NW.  For kernels short of registers, not for speed (with block_incl_scan at
// its scans k_chunk_sort_small<16384>, which is at its 128 registers, spilled 68 bytes per lane instead of 40).
template <typename T>
__device__ __forceinline__ T block_incl_scan_walk(T v, T *sh_wave)
{
    const int w = threadIdx.x >> 6;
    T inc = block_scan_wave_totals(v, sh_wave);
    for (int i = 0; i < w; ++i) inc = inc + sh_wave[i];
    return inc;
}

// This block's slice [lo, hi) of [0, n): equal slices for all blocks of the grid, rounded up to whole rounds of `round` elements
template <typename I>
__device__ __forceinline__ void block_slice(I n, I round, I &lo, I &hi)
{
    I per = (n + (I)gridDim.x - 1) / (I)gridDim.x;
    per = (per + round - 1) / round * round;
    const long long l = (long long)blockIdx.x * per, h = l + per;
    lo = l < (long long)n ? (I)l : n;
    hi = h < (long long)n ? (I)h : n;
}

// cnt[b0] + ... + cnt[b1 - 1] by the calling wave (per-block counters of a count pass; with b0 = 0, b1 = blockIdx.x: the entries of
// the blocks in front of this one)
__device__ __forceinline__ uint32_t wave_sum_counters(const uint32_t *__restrict__ cnt, int b0, int b1)
{
    uint32_t s = 0;
    for (int b = b0 + (int)(threadIdx.x & (kWave - 1)); b < b1; b += kWave) s += cnt[b];
    return wave_sum(s);
}

// One round of a stable partition by a block of NW waves into up to MAXW ways: every thread offers at most one element (way < 0:
// none) and receives its position.  run[k] = the next free position of way k: the caller sets it before the first round, behind
// a barrier; the round advances it.  Elements of a way keep thread order, rounds follow each other.
// Two barriers: per-wave counts -> one thread per way walks the waves -> positions.  A following round needs no barrier in
// between: it stores w before its first barrier (w was last read before this round's second one) and pre / run behind it.
// (declared __align__(16), the walk moves a way's counts and prefixes as 16-byte words)
template <int MAXW, int NW>
struct PartitionLds { uint32_t w[MAXW][NW], pre[MAXW][NW], run[MAXW]; };

template <int MAXW, int NW>
__device__ __forceinline__ uint32_t partition_round(int way, int nways, PartitionLds<MAXW, NW> &sh)
{
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x >> 6;
    const unsigned long long below = (1ull << lane) - 1ull;
    uint32_t rank = 0;
    for (int k = 0; k < nways; ++k) {
        const unsigned long long m = __ballot(way == k);
        if (way == k) rank = (uint32_t)__popcll(m & below);
        if (lane == 0) sh.w[k][wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if ((int)threadIdx.x < nways) {
        uint32_t run = sh.run[threadIdx.x];
#pragma unroll
        for (int w = 0; w < NW; ++w) { sh.pre[threadIdx.x][w] = run; run += sh.w[threadIdx.x][w]; }
        sh.run[threadIdx.x] = run;
    }
    __syncthreads();
    return way >= 0 ? sh.pre[way][wv] + rank : 0u;
}

}  // namespace gsr
