// gsr_geom.hip — per-Gaussian kernels: forward preprocess (K1), geometry backward (K8+K9 fused),
// frustum test (K10).  One thread per Gaussian; the maths lives in gsr_math.h.
//
// HBM traffic per Gaussian: K1 reads 44 + 12K B (means 12, scale 12, quat 16, opacity 4,
// K SH triples) and writes 48 (record) + 4 (radii) + 4 (tiles) + 1 (clamp mask); K8+K9 reads
// 48 (screen grads) + 44 + 12K + 5 and writes 40 + 12M.  Camera matrices are wave-uniform loads that
// the compiler scalarises (s_load) — they never cost vector memory bandwidth.
//
// The backward kernels (k_geom_bwd, k_geom_bwd_sparse, k_geom_bwd_depth, k_camera_bwd) share their row rule (visit_row), their
// liveness test (load_screen_row), their inputs (load_backward_inputs) and their stores (store_geom_grad); every launch templated
// on the SH degree and the raw mode goes through dispatch_deg_raw.
#include <type_traits>

#include "gsr_internal.h"

namespace gsr {

constexpr int kGeomBlock = 256;

// One Gaussian's inputs in registers.  RAW != 0: the tensors are the optimizer's raw parameters and
// the activations (exp / normalize / sigmoid) happen here, in registers.  RAW == 1: the SH coefficients arrive as the reference's
// two tensors (features_dc [P,1,3], features_rest [P,M-1,3]) and are joined in registers (its torch.cat); RAW == 2: they are ONE
// interleaved table [P,M,3] (scene.GaussianModel's packed leaf), read and differentiated exactly like activated input.
template <int DEG, int RAW>
struct GaussIn {
    float p[3], sc[3], q[4], cv[6], opacity;
    float shl[RAW == 1 ? 3 * (DEG + 1) * (DEG + 1) : 1];     // RAW == 1: the [K,3] coefficients, features_dc ++ features_rest
    const float *sh_global;   // otherwise: this Gaussian's [M,3] coefficients in the shs tensor (or null)
    RawAct act;
    // what preprocess_one / geom_backward_one read; no pointer member aliases shl, so the array stays in registers
    __device__ __forceinline__ const float *sh() const { if constexpr (RAW == 1) return shl; else return sh_global; }
    // the precomputed covariance, when the frame has one (never in raw mode)
    __device__ __forceinline__ const float *cov(const float *covpre) const { return (!RAW && covpre) ? cv : nullptr; }
};

template <int DEG, int RAW>
__device__ __forceinline__ void load_gaussian(int i, int M, const float *__restrict__ means, const float *__restrict__ scales,
                                              const float *__restrict__ rots, const float *__restrict__ covpre,
                                              const float *__restrict__ opac, const float *__restrict__ shs,
                                              const float *__restrict__ shs_rest, bool with_sh, GaussIn<DEG, RAW> &in)
{
    in.p[0] = means[3 * i]; in.p[1] = means[3 * i + 1]; in.p[2] = means[3 * i + 2];
    in.sc[0] = in.sc[1] = in.sc[2] = 0.f;
    in.q[0] = 1.f; in.q[1] = in.q[2] = in.q[3] = 0.f;
    if constexpr (RAW) {
        const float ls[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        const float4 qq = reinterpret_cast<const float4 *>(rots)[i];
        const float rq[4] = {qq.x, qq.y, qq.z, qq.w};
        activate_raw(ls, rq, opac[i], in.act);
#pragma unroll
        for (int k = 0; k < 3; ++k) in.sc[k] = in.act.scale[k];
#pragma unroll
        for (int k = 0; k < 4; ++k) in.q[k] = in.act.q[k];
        in.opacity = in.act.opacity;
        if constexpr (RAW == 1) {
            constexpr int K = (DEG + 1) * (DEG + 1);
            if (with_sh) {                       // culled Gaussians never read their coefficients
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) in.shl[ch] = shs[3 * (size_t)i + ch];
                const float *rest = shs_rest + (size_t)i * (M - 1) * 3;
#pragma unroll
                for (int k = 3; k < 3 * K; ++k) in.shl[k] = rest[k - 3];
            } else {
#pragma unroll
                for (int k = 0; k < 3 * K; ++k) in.shl[k] = 0.f;
            }
            in.sh_global = nullptr;
        } else {
            in.sh_global = shs ? shs + (size_t)i * M * 3 : nullptr;
        }
    } else {
        if (covpre) {
#pragma unroll
            for (int k = 0; k < 6; ++k) in.cv[k] = covpre[6 * (size_t)i + k];
        } else {
            in.sc[0] = scales[3 * i]; in.sc[1] = scales[3 * i + 1]; in.sc[2] = scales[3 * i + 2];
            const float4 qq = reinterpret_cast<const float4 *>(rots)[i];
            in.q[0] = qq.x; in.q[1] = qq.y; in.q[2] = qq.z; in.q[3] = qq.w;
        }
        in.opacity = opac ? opac[i] : 0.f;
        in.sh_global = shs ? shs + (size_t)i * M * 3 : nullptr;
    }
}

template <int DEG, int RAW, bool LAZY>
__global__ __launch_bounds__(kGeomBlock) void k_preprocess(FrameK f, const float *__restrict__ view,
                                                           const float *__restrict__ proj, const float *__restrict__ campos,
                                                           const float *__restrict__ means, const float *__restrict__ scales,
                                                           const float *__restrict__ rots, const float *__restrict__ covpre,
                                                           const float *__restrict__ opac, const float *__restrict__ shs,
                                                           const float *__restrict__ shs_rest,
                                                           const float *__restrict__ colpre, float4 *__restrict__ records,
                                                           uint2 *__restrict__ tiles_mass, uint8_t *__restrict__ clamped,
                                                           int32_t *__restrict__ radii, uint32_t *__restrict__ sort_keys,
                                                           uint32_t *__restrict__ sort_vals, uint32_t *__restrict__ prefilter_flag,
                                                           uint4 *__restrict__ zero16, int zero16_n)
{
    const int i = blockIdx.x * kGeomBlock + threadIdx.x;
    // the selection's histograms (SelState, 130 KB) start every frame at zero: cleared here, one 16-byte store per thread,
    // instead of by a memset launch of its own in front of this kernel (the histogram kernels run after this one)
    for (int z = i; z < zero16_n; z += (int)gridDim.x * kGeomBlock) zero16[z] = make_uint4(0u, 0u, 0u, 0u);
    if (i >= f.P) return;
    float V[16], PV[16], cp[3];
#pragma unroll
    for (int k = 0; k < 16; ++k) { V[k] = view[k]; PV[k] = proj[k]; }
    cp[0] = campos[0]; cp[1] = campos[1]; cp[2] = campos[2];
    GaussIn<DEG, RAW> in;
    const float p0[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    const bool near_ok = in_frustum(p0, V);
    // prefiltered = "the caller guarantees every point passes the frustum test" (the upstream kernel traps when one
    // does not); here the frame is refused with GSR_ERR_PREFILTERED after the plan readback
    if (prefilter_flag && !near_ok) *prefilter_flag = 1u;
    // LAZY: SH colours are evaluated per depth chunk (k_chunk_colors), only for the chunks that get binned; this kernel then
    // reads no coefficient at all (two thirds of its bytes at degree 3)
    load_gaussian<DEG, RAW>(i, f.M, means, scales, rots, covpre, opac, shs, shs_rest, near_ok && !LAZY, in);
    PreOut o;
    preprocess_one<DEG>(f, V, PV, cp, in.p, in.sc, in.q, in.cov(covpre), in.opacity, LAZY ? nullptr : in.sh(),
                        (!RAW && colpre) ? colpre + 3 * (size_t)i : nullptr, o);
    radii[i] = o.radius;
    // mass in fixed point: integer sums are order-independent
    tiles_mass[i] = make_uint2(o.tiles, (uint32_t)fminf(o.mass * kMassUnitsPerPixelNeper, 4294967040.f));
    clamped[i] = (uint8_t)o.clamped;
    records[3 * (size_t)i + 0] = make_float4(o.s.x, o.s.y, o.s.cA, o.s.cB);
    records[3 * (size_t)i + 1] = make_float4(o.s.cC, o.s.op, o.s.r, o.s.g);
    records[3 * (size_t)i + 2] = make_float4(o.s.b, o.s.depth, o.s.rect_x, o.s.rect_y);
    // depth-sort key: binary32 pattern of the (positive) view depth; invisible Gaussians sort last.  Visibility
    // is that of the FULL image (radius > 0), not of this rank's slab, so that the depth order is identical on
    // every rank of a sharded render (the multi-GPU gradient exchange selects by depth key).
    sort_keys[i] = o.radius > 0 ? __float_as_uint(o.s.depth) : 0xFFFFFFFFu;
    (void)sort_vals;                           // the depth order is built by selection (gsr_select.hip)
}

int launch_preprocess(const FrameK &f, const gsr_camera &cam, const gsr_gaussians &g, GeomWS &ws, int32_t *radii,
                      bool prefiltered, bool debug, hipStream_t s)
{
    if (f.P == 0) return GSR_OK;
    const int grid = (f.P + kGeomBlock - 1) / kGeomBlock;
    uint32_t *prefilter_flag = nullptr;
    if (prefiltered) {
        prefilter_flag = &ws.ctrl->prefilter_violation;
        GSR_HIP_CHECK(hipMemsetAsync(prefilter_flag, 0, 4, s));
    }
    ProfileScope prof("preprocess", s);
#define GSR_PRE(DEG, RAW, LAZY)                                                                                     \
    hipLaunchKernelGGL((k_preprocess<DEG, RAW, LAZY>), dim3(grid), dim3(kGeomBlock), 0, s, f, cam.viewmatrix, cam.projmatrix,  \
                       cam.campos, g.means3D, g.scales, g.rotations, g.cov3D_precomp, g.opacities, g.shs, g.shs_rest,   \
                       g.colors_precomp, ws.records, ws.tiles_mass, ws.clamped, radii, ws.sort_keys[0],                 \
                       ws.sort_vals[0], prefilter_flag, reinterpret_cast<uint4 *>(ws.sel), (int)(sizeof(SelState) / 16))
    if (g.shs) {                  // colours from SH: lazily, per binned chunk
        if (g.raw) GSR_PRE(0, 1, true);            // lazy colours: no coefficient is read here, the SH layout does not matter
        else GSR_PRE(0, 0, true);
    } else {
        GSR_PRE(0, 0, false);  // precomputed colours are copied into the record here
    }
#undef GSR_PRE
    GSR_LAUNCH_CHECK("preprocess", debug, s);
    return GSR_OK;
}

// raw mode with the reference's two SH tensors (features_dc + features_rest): raw == 1.  raw == 2: one interleaved [P,M,3] table
static inline bool raw_split_sh(const gsr_gaussians &g) { return g.raw == 1; }
// the RAW template argument of the backward kernels: 0 activated input, 1 raw with split SH, 2 raw with one SH table
static inline int raw_mode(const gsr_gaussians &g) { return !g.raw ? 0 : (raw_split_sh(g) ? 1 : 2); }

// Calls fn(integral_constant<int, DEG>, integral_constant<int, RAW>) with DEG = D clamped to [0, 3] and RAW = mode < NRAW: the one
// place where the run-time SH degree and raw mode pick a kernel instantiation.
template <int NRAW, class F>
static inline void dispatch_deg_raw(int D, int mode, F &&fn)
{
    auto with_deg = [&](auto deg) {
        if (mode == 0) fn(deg, std::integral_constant<int, 0>{});
        else if (NRAW == 2 || mode == 1) fn(deg, std::integral_constant<int, 1>{});
        else if constexpr (NRAW > 2) fn(deg, std::integral_constant<int, 2>{});
    };
    switch (D > 3 ? 3 : (D < 0 ? 0 : D)) {
        case 0: with_deg(std::integral_constant<int, 0>{}); break;
        case 1: with_deg(std::integral_constant<int, 1>{}); break;
        case 2: with_deg(std::integral_constant<int, 2>{}); break;
        default: with_deg(std::integral_constant<int, 3>{}); break;
    }
}

// ---- A.6, lazily: SH colour (+ clamp flags) of the Gaussians of depth ranks [r0, r1) — one binned chunk — patched into
// their splat records right before the chunk is blended.  On a depth-complex frame that is a few thousand Gaussians
// instead of all the visible ones.
template <int DEG, int RAW>
__global__ __launch_bounds__(kGeomBlock) void k_chunk_colors(FrameK f, int r0, int r1, const uint32_t *__restrict__ order,
                                                             const uint32_t *__restrict__ cnt_open,
                                                             const float *__restrict__ campos, const float *__restrict__ means,
                                                             const float *__restrict__ shs, const float *__restrict__ shs_rest,
                                                             float4 *__restrict__ records, uint8_t *__restrict__ clamped)
{
    const int r = r0 + blockIdx.x * kGeomBlock + threadIdx.x;
    if (r >= r1) return;
    if (cnt_open[r] == 0u) return;               // no tile took this Gaussian (a late chunk: most tiles are closed): nobody reads its colour
    const int i = (int)order[r];
    const float cp[3] = {campos[0], campos[1], campos[2]};
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    constexpr int K = (DEG + 1) * (DEG + 1);
    float shl[3 * K];
    if constexpr (RAW == 1) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) shl[ch] = shs[3 * (size_t)i + ch];
        const float *rest = shs_rest + (size_t)i * (f.M - 1) * 3;
#pragma unroll
        for (int k = 3; k < 3 * K; ++k) shl[k] = rest[k - 3];
    } else {
        const float *src = shs + (size_t)i * f.M * 3;
        if constexpr ((3 * K) % 4 == 0) {
            if ((f.M * 3) % 4 == 0) {              // the row starts on a 16-byte boundary: a gathered row is 12 x 16 B, not 48 x 4 B
                const float4 *src4 = reinterpret_cast<const float4 *>(src);
#pragma unroll
                for (int k = 0; k < 3 * K / 4; ++k) {
                    const float4 v = src4[k];
                    shl[4 * k] = v.x; shl[4 * k + 1] = v.y; shl[4 * k + 2] = v.z; shl[4 * k + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 3 * K; ++k) shl[k] = src[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3 * K; ++k) shl[k] = src[k];
        }
    }
    float rgb[3];
    unsigned cl;
    sh_color_one<DEG>(f, cp, p, shl, rgb, cl);
    float *rec = reinterpret_cast<float *>(records + 3 * (size_t)i);
    rec[6] = rgb[0]; rec[7] = rgb[1]; rec[8] = rgb[2];          // record = {x, y, qA, qB | qC, lop, r, g | b, depth, rect, rect}
    clamped[i] = (uint8_t)cl;
}

// The same for a chunk that holds EVERY visible Gaussian (a frame that does not saturate: one chunk): Gaussians are taken in
// index order, so a wave's 64 coefficient rows are one contiguous run, loaded with full 16-byte-per-lane coalescing into
// LDS rows (a gather by depth rank reads 192-byte rows scattered over the tensor).  Invisible Gaussians (zeroed record)
// are skipped.
template <int DEG, int RAW>
__global__ __launch_bounds__(kGeomBlock) void k_chunk_colors_all(FrameK f, const float *__restrict__ campos, const float *__restrict__ means,
                                                                 const float *__restrict__ shs, const float *__restrict__ shs_rest,
                                                                 float4 *__restrict__ records, uint8_t *__restrict__ clamped)
{
    constexpr int K = (DEG + 1) * (DEG + 1);
    constexpr int kRow = 3 * K + 1;                            // +1: lanes read their rows conflict-free
    __shared__ float sh_stage[(kGeomBlock / 64) * 64 * kRow];
    const int i = blockIdx.x * kGeomBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wave_first = i - lane;
    const int n_rows = min(64, f.P - wave_first);
    if (n_rows <= 0) return;
    const bool visible = i < f.P && reinterpret_cast<const float *>(records + 3 * (size_t)i)[9] > 0.f;      // record.depth
    if (__ballot(visible) == 0ull) return;
    float *stage = sh_stage + wv * (64 * kRow);
    const int rowf = 3 * f.M;                                  // stored floats per Gaussian (>= 3 K)
    if constexpr (RAW == 1) {
        for (int e = lane; e < n_rows * 3; e += 64) stage[(e / 3) * kRow + e % 3] = shs[(size_t)wave_first * 3 + e];
        if constexpr (K > 1) {
            const int row = rowf - 3;
            const float *src = shs_rest + (size_t)wave_first * row;
            for (int e = lane; e < n_rows * row; e += 64) {
                const int c = e % row;
                if (c < 3 * K - 3) stage[(e / row) * kRow + 3 + c] = src[e];
            }
        }
    } else {
        const float *src = shs + (size_t)wave_first * rowf;
        const int total = n_rows * rowf;
        if ((((uintptr_t)src) & 15) == 0 && rowf == 3 * K && K == 16 && n_rows == 64) {
            // the common shape (degree 3 stored and active, a full wave): all twelve 1-KB loads in flight before the first LDS store
            const float4 *src4 = reinterpret_cast<const float4 *>(src);
            float4 v[12];
#pragma unroll
            for (int it = 0; it < 12; ++it) v[it] = src4[lane + 64 * it];
#pragma unroll
            for (int it = 0; it < 12; ++it) {
                const int e = 4 * (lane + 64 * it), r = e / 48, c = e - r * 48;
                float *d = stage + r * kRow + c;
                d[0] = v[it].x; d[1] = v[it].y; d[2] = v[it].z; d[3] = v[it].w;
            }
        } else if ((((uintptr_t)src) & 15) == 0 && rowf % 4 == 0) {
            const float4 *src4 = reinterpret_cast<const float4 *>(src);
            for (int e4 = lane; e4 < total / 4; e4 += 64) {
                const float4 v = src4[e4];
                const int e = 4 * e4, r = e / rowf, c = e - r * rowf;          // rowf % 4 == 0: the four floats share a row
                if (c < 3 * K) {                                               // (3 K) % 4 == 0 whenever K > 1; K == 1 has rowf % 4 != 0 unless M % 4 == 0
                    float *d = stage + r * kRow + c;
                    d[0] = v.x;
                    if (c + 1 < 3 * K) d[1] = v.y;
                    if (c + 2 < 3 * K) d[2] = v.z;
                    if (c + 3 < 3 * K) d[3] = v.w;
                }
            }
        } else {
            for (int e = lane; e < total; e += 64) {
                const int r = e / rowf, c = e - r * rowf;
                if (c < 3 * K) stage[r * kRow + c] = src[e];
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    if (!visible) return;
    const float cp[3] = {campos[0], campos[1], campos[2]};
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    float shl[3 * K];
#pragma unroll
    for (int k = 0; k < 3 * K; ++k) shl[k] = stage[lane * kRow + k];
    float rgb[3];
    unsigned cl;
    sh_color_one<DEG>(f, cp, p, shl, rgb, cl);
    float *rec = reinterpret_cast<float *>(records + 3 * (size_t)i);
    rec[6] = rgb[0]; rec[7] = rgb[1]; rec[8] = rgb[2];
    clamped[i] = (uint8_t)cl;
}

int launch_chunk_colors(const FrameK &f, const gsr_camera &cam, const gsr_gaussians &g, int r0, int r1, int num_visible, GeomWS &ws,
                        bool debug, hipStream_t s)
{
    if (!g.shs || r1 <= r0) return GSR_OK;           // precomputed colours went into the records in the preprocess
    ProfileScope prof("chunk_colors", s);
    if (colors_in_index_order(r0, r1, num_visible, f.P)) {
        const int grid_all = (f.P + kGeomBlock - 1) / kGeomBlock;
        // (no activations in these kernels: RAW only names the SH layout)
        dispatch_deg_raw<2>(f.D, raw_split_sh(g) ? 1 : 0, [&](auto deg, auto raw) {
            hipLaunchKernelGGL((k_chunk_colors_all<decltype(deg)::value, decltype(raw)::value>), dim3(grid_all), dim3(kGeomBlock), 0, s, f,
                               cam.campos, g.means3D, g.shs, g.shs_rest, ws.records, ws.clamped);
        });
        GSR_LAUNCH_CHECK("chunk_colors_all", debug, s);
        return GSR_OK;
    }
    const int grid = (r1 - r0 + kGeomBlock - 1) / kGeomBlock;
    dispatch_deg_raw<2>(f.D, raw_split_sh(g) ? 1 : 0, [&](auto deg, auto raw) {
        hipLaunchKernelGGL((k_chunk_colors<decltype(deg)::value, decltype(raw)::value>), dim3(grid), dim3(kGeomBlock), 0, s, f, r0, r1,
                           ws.order, ws.cnt_open, cam.campos, g.means3D, g.shs, g.shs_rest, ws.records, ws.clamped);
    });
    GSR_LAUNCH_CHECK("chunk_colors", debug, s);
    return GSR_OK;
}

// ---- K8 + K9: dL/d(screen-space quantities) -> dL/d(inputs) for Gaussians [g0, g1).
__device__ __forceinline__ bool sh_wanted_or_read(const float *shs, int has_colpre) { return shs != nullptr && !has_colpre; }

// The row rule: the Gaussian that thread t of a backward kernel visits, or -1.  Dense: g0 + t.  SPARSE: rank t of `order` (an
// exchange list entry nobody filled is -1), skipped when this frame binned no instance of the rank (cnt_open, optional: its
// screen-space row is zero or was never written).  Invisible Gaussians (their row may be undefined) are skipped.
template <bool SPARSE>
__device__ __forceinline__ int visit_row(int t, int g0, const uint32_t *__restrict__ order, const uint32_t *__restrict__ cnt_open, int P,
                                         const int32_t *__restrict__ radii)
{
    int i = g0 + t;
    if constexpr (SPARSE) {
        if (cnt_open && cnt_open[t] == 0u) return -1;
        i = (int)order[t];
        if (i < 0 || i >= P) return -1;
    }
    return radii[i] > 0 ? i : -1;
}

// Reads Gaussian i's screen-space gradient row; returns whether it is live.  A Gaussian that no pixel accepted (occluded behind
// saturated tiles, or just too faint everywhere) has an all-zero row; every output of A.10 and every camera term is linear in it,
// so its results are exact zeros and none of its inputs need to be read.  In depth-complex scenes that is the vast majority of the
// visible set.  The geometry and the camera kernels share this test: their rows and sums stop together.
__device__ __forceinline__ bool load_screen_row(const float4 *__restrict__ screen, int i, float4 &s0, float4 &s1, float4 &s2)
{
    s0 = screen[3 * (size_t)i]; s1 = screen[3 * (size_t)i + 1]; s2 = screen[3 * (size_t)i + 2];
    return (s0.x != 0.f) | (s0.y != 0.f) | (s0.z != 0.f) | (s0.w != 0.f) | (s1.x != 0.f) | (s1.y != 0.f) | (s1.z != 0.f) |
           (s1.w != 0.f) | (s2.x != 0.f);
}

// What geom_backward_one / camera_backward_one read for one live Gaussian.  STAGED: the SH row is `staged_sh` (k_geom_bwd's LDS
// row), a compile-time choice so that the RAW == 1 register array never meets a pointer select; otherwise it comes from global memory.
// The clamp mask of an SH colour is recomputed from the coefficients (the forward's own function), not read: colours are evaluated
// lazily, only for Gaussians some tile of THIS frame took, and a rank of a sharded render back-propagates Gaussians that only the
// other ranks binned.
template <int DEG, int RAW>
struct BwdIn {
    float V[16], PV[16], cp[3], sg[9];
    GaussIn<DEG, RAW> in;
    unsigned clamp_bits;
};

template <int DEG, int RAW, bool STAGED>
__device__ __forceinline__ void load_backward_inputs(const FrameK &f, int i, const float *__restrict__ view, const float *__restrict__ proj,
                                                     const float *__restrict__ campos, const float *__restrict__ means,
                                                     const float *__restrict__ scales, const float *__restrict__ rots,
                                                     const float *__restrict__ covpre, const float *__restrict__ opac,
                                                     const float *__restrict__ shs, const float *__restrict__ shs_rest, int has_colpre,
                                                     const uint8_t *__restrict__ clamped, const float4 &s0, const float4 &s1,
                                                     const float4 &s2, const float *staged_sh, BwdIn<DEG, RAW> &b)
{
#pragma unroll
    for (int k = 0; k < 16; ++k) { b.V[k] = view[k]; b.PV[k] = proj[k]; }
    b.cp[0] = campos[0]; b.cp[1] = campos[1]; b.cp[2] = campos[2];
    load_gaussian<DEG, RAW>(i, f.M, means, scales, rots, covpre, opac, STAGED ? nullptr : shs, STAGED ? nullptr : shs_rest, !STAGED, b.in);
    b.sg[0] = s0.x; b.sg[1] = s0.y; b.sg[2] = s0.z; b.sg[3] = s0.w; b.sg[4] = s1.x; b.sg[5] = s1.y; b.sg[6] = s1.z; b.sg[7] = s1.w; b.sg[8] = s2.x;
    b.clamp_bits = clamped[i];
    if (shs && !has_colpre) {
        float rgb_[3];
        if constexpr (STAGED) sh_color_one<DEG>(f, b.cp, b.in.p, staged_sh, rgb_, b.clamp_bits);
        else sh_color_one<DEG>(f, b.cp, b.in.p, b.in.sh(), rgb_, b.clamp_bits);
    }
}

// Gaussian i's rows of every wanted parameter gradient except dL/dsh (and means2D's third column, which only the dense kernel writes).
__device__ __forceinline__ void store_geom_grad(const gsr_grads &out, int i, const GeomGrad &g, int has_colpre, const float *covpre)
{
    if (out.means3D) { out.means3D[3 * i] = g.dmean[0]; out.means3D[3 * i + 1] = g.dmean[1]; out.means3D[3 * i + 2] = g.dmean[2]; }
    if (out.means2D) { out.means2D[3 * i] = g.dmean2D[0]; out.means2D[3 * i + 1] = g.dmean2D[1]; }
    if (out.opacities) out.opacities[i] = g.dopacity;
    if (out.colors_precomp && has_colpre) {
        out.colors_precomp[3 * i] = g.dcolor[0]; out.colors_precomp[3 * i + 1] = g.dcolor[1]; out.colors_precomp[3 * i + 2] = g.dcolor[2];
    }
    if (out.scales && !covpre) { out.scales[3 * i] = g.dscale[0]; out.scales[3 * i + 1] = g.dscale[1]; out.scales[3 * i + 2] = g.dscale[2]; }
    if (out.rotations && !covpre) reinterpret_cast<float4 *>(out.rotations)[i] = make_float4(g.drot[0], g.drot[1], g.drot[2], g.drot[3]);
    if (out.cov3D_precomp && covpre) {
#pragma unroll
        for (int k = 0; k < 6; ++k) out.cov3D_precomp[6 * (size_t)i + k] = g.dcov[k];
    }
}

template <int DEG, int RAW>
__global__ __launch_bounds__(kGeomBlock) void k_geom_bwd(FrameK f, int g0, int g1, const float *__restrict__ view,
                                                         const float *__restrict__ proj, const float *__restrict__ campos,
                                                         const float *__restrict__ means, const float *__restrict__ scales,
                                                         const float *__restrict__ rots, const float *__restrict__ covpre,
                                                         const float *__restrict__ opac, const float *__restrict__ shs,
                                                         const float *__restrict__ shs_rest, int has_colpre,
                                                         const int32_t *__restrict__ radii, const uint8_t *__restrict__ clamped,
                                                         const float4 *__restrict__ screen, gsr_grads out)
{
    __shared__ float sh_stage[(kGeomBlock / 64) * 64 * 49];
    const int i = g0 + blockIdx.x * kGeomBlock + threadIdx.x;
    const bool in_range = i < g1;
    const int M = f.M;
    const bool visible = in_range && visit_row<false>(i - g0, g0, nullptr, nullptr, f.P, radii) >= 0;
    GeomGrad g{};                                // zeros: the rows of dead and invisible Gaussians
    constexpr int K = (DEG + 1) * (DEG + 1);
    // dL/dsh leaves through LDS: every lane owns one staging row of 3M (+1 pad) floats; geom_backward_one writes the
    // 3K live entries straight into it, the rest is zero-filled, and the wave then stores its 64 rows as one
    // contiguous, lane-coalesced run
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int rowf = 3 * M;                                       // floats per Gaussian incl. the DC triple
    float *my_row = sh_stage + wv * (64 * 49) + lane * (rowf + 1);
    const bool sh_wanted = shs && (out.shs || (RAW == 1 && out.shs_rest));
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0, s2 = s0;
    const bool live = visible && load_screen_row(screen, i, s0, s1, s2);       // a dead row's outputs are exact zeros
    // The wave's SH rows ([M,3] per Gaussian, consecutive Gaussians contiguous in memory) come in through the same LDS
    // staging rows the gradients leave by: 64 lanes x 16 B per load instruction instead of 64 single dwords 192 B apart (the
    // per-lane strided form re-fetches every 64-B sector sixteen times).  geom_backward_one reads coefficient k and then
    // overwrites it with its gradient, so one row serves both directions.
    const int wave_first = i - lane;                           // first Gaussian of this wave
    const int n_rows = min(64, g1 - wave_first);
    const unsigned long long live_mask = __ballot(live);
    const bool wave_live = live_mask != 0ull;
    // few live lanes (a frame whose back Gaussians sit behind saturated pixels: 19 % live at 5e6 Gaussians / 4K, in index order
    // every wave holds some): each live lane fetches its own row, three whole 64-byte sectors, instead of the wave staging all 64
    // rows for a dozen readers (0.96 GB of the kernel's 2.6 GB there)
    const bool own_rows = RAW != 1 && __popcll(live_mask) * 3 < 64 && rowf % 4 == 0 && (((uintptr_t)shs) & 15) == 0;
    if (sh_wanted_or_read(shs, has_colpre) && wave_live && rowf > 0 && n_rows > 0 && own_rows) {
        if (live) {
            const float4 *src4 = reinterpret_cast<const float4 *>(shs + (size_t)i * rowf);
            for (int e4 = 0; e4 < rowf / 4; ++e4) {
                const float4 v = src4[e4];
                my_row[4 * e4] = v.x; my_row[4 * e4 + 1] = v.y; my_row[4 * e4 + 2] = v.z; my_row[4 * e4 + 3] = v.w;
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    } else if (sh_wanted_or_read(shs, has_colpre) && wave_live && rowf > 0 && n_rows > 0) {
        float *stage_w = sh_stage + wv * (64 * 49);
        if constexpr (RAW == 1) {
            for (int e = lane; e < n_rows * 3; e += 64) stage_w[(e / 3) * (rowf + 1) + e % 3] = shs[(size_t)wave_first * 3 + e];
            const int row = rowf - 3;
            if (row > 0) {
                const float *src = shs_rest + (size_t)wave_first * row;
                for (int e = lane; e < n_rows * row; e += 64) stage_w[(e / row) * (rowf + 1) + 3 + e % row] = src[e];
            }
        } else {
            const float *src = shs + (size_t)wave_first * rowf;
            const int total = n_rows * rowf;
            if ((((uintptr_t)src) & 15) == 0 && rowf == 48 && n_rows == 64) {
                // the common shape (16 coefficients, a full wave): all twelve 1-KB loads in flight before the first LDS store
                const float4 *src4 = reinterpret_cast<const float4 *>(src);
                float4 v[12];
#pragma unroll
                for (int it = 0; it < 12; ++it) v[it] = src4[lane + 64 * it];
#pragma unroll
                for (int it = 0; it < 12; ++it) {
                    const int e = 4 * (lane + 64 * it), r = e / 48, c = e - r * 48;
                    float *d = stage_w + r * 49 + c;
                    d[0] = v[it].x; d[1] = v[it].y; d[2] = v[it].z; d[3] = v[it].w;
                }
            } else if ((((uintptr_t)src) & 15) == 0) {
                const float4 *src4 = reinterpret_cast<const float4 *>(src);
                for (int e4 = lane; e4 < total / 4; e4 += 64) {
                    const float4 v = src4[e4];
                    const int e = 4 * e4;
                    stage_w[(e / rowf) * (rowf + 1) + e % rowf] = v.x;
                    stage_w[((e + 1) / rowf) * (rowf + 1) + (e + 1) % rowf] = v.y;
                    stage_w[((e + 2) / rowf) * (rowf + 1) + (e + 2) % rowf] = v.z;
                    stage_w[((e + 3) / rowf) * (rowf + 1) + (e + 3) % rowf] = v.w;
                }
                for (int e = (total / 4) * 4 + lane; e < total; e += 64) stage_w[(e / rowf) * (rowf + 1) + e % rowf] = src[e];
            } else {
                for (int e = lane; e < total; e += 64) stage_w[(e / rowf) * (rowf + 1) + e % rowf] = src[e];
            }
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (live) {
        BwdIn<DEG, RAW> b;
        load_backward_inputs<DEG, RAW, true>(f, i, view, proj, campos, means, scales, rots, covpre, opac, shs, shs_rest, has_colpre, clamped, s0,
                                             s1, s2, my_row, b);
        geom_backward_one<DEG>(f, b.V, b.PV, b.cp, b.in.p, b.in.sc, b.in.q, b.in.cov(covpre), shs ? my_row : nullptr, has_colpre != 0,
                               b.clamp_bits, b.sg, g, my_row, sh_wanted);
        if constexpr (RAW) activate_raw_backward(b.in.act, g);
    }
    if (in_range) {                              // (lanes past the end only help with the cooperative SH store below)
        store_geom_grad(out, i, g, has_colpre, covpre);
        if (out.means2D) out.means2D[3 * i + 2] = 0.f;
    }
    if (sh_wanted && rowf > 0) {
        const bool any_live = wave_live;
        if (any_live) {
            const int nlive = live ? 3 * K : 0;
            for (int k = nlive; k < rowf; ++k) my_row[k] = 0.f;    // rows of dead lanes, coefficients above the active degree
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        const float *stage = sh_stage + wv * (64 * 49);
        if constexpr (RAW == 1) {
            if (in_range && out.shs) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) out.shs[3 * (size_t)i + ch] = any_live ? my_row[ch] : 0.f;
            }
            const int row = rowf - 3;                              // _features_rest: floats per Gaussian
            if (out.shs_rest && row > 0 && n_rows > 0) {
                float *dst = out.shs_rest + (size_t)wave_first * row;
                const int total = n_rows * row;
                if (!any_live) { for (int e = lane; e < total; e += 64) dst[e] = 0.f; }
                else { for (int e = lane; e < total; e += 64) dst[e] = stage[(e / row) * (rowf + 1) + 3 + e % row]; }
            }
        } else if (n_rows > 0) {
            float *dst = out.shs + (size_t)wave_first * rowf;
            const int total = n_rows * rowf;
            if (rowf == 48 && n_rows == 64 && (((uintptr_t)dst) & 15) == 0) {      // twelve 1-KB stores instead of forty-eight 256-B ones
                float4 *dst4 = reinterpret_cast<float4 *>(dst);
#pragma unroll
                for (int it = 0; it < 12; ++it) {
                    const int e = 4 * (lane + 64 * it), r = e / 48, c = e - r * 48;
                    const float *q = stage + r * 49 + c;
                    dst4[lane + 64 * it] = any_live ? make_float4(q[0], q[1], q[2], q[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            else if (!any_live) { for (int e = lane; e < total; e += 64) dst[e] = 0.f; }
            else { for (int e = lane; e < total; e += 64) dst[e] = stage[(e / rowf) * (rowf + 1) + e % rowf]; }
        }
    }
}

// ---- sparse variant for depth-complex frames: every output was zero-filled by memset; only the Gaussians of the
// binned depth prefix (rank < n_ranks) can have a non-zero screen-space gradient.  One thread per rank, rows
// written individually (they are few).
template <int DEG, int RAW>
__global__ __launch_bounds__(kGeomBlock) void k_geom_bwd_sparse(FrameK f, int n_ranks, const uint32_t *__restrict__ order,
                                                                const float *__restrict__ view, const float *__restrict__ proj,
                                                                const float *__restrict__ campos, const float *__restrict__ means,
                                                                const float *__restrict__ scales, const float *__restrict__ rots,
                                                                const float *__restrict__ covpre, const float *__restrict__ opac,
                                                                const float *__restrict__ shs, const float *__restrict__ shs_rest,
                                                                int has_colpre, const int32_t *__restrict__ radii,
                                                                const uint8_t *__restrict__ clamped,
                                                                const float4 *__restrict__ screen, gsr_grads out,
                                                                const uint32_t *__restrict__ cnt_open)
{
    const int r = blockIdx.x * kGeomBlock + threadIdx.x;
    if (r >= n_ranks) return;
    const int i = visit_row<true>(r, 0, order, cnt_open, f.P, radii);
    if (i < 0) return;
    float4 s0, s1, s2;
    if (!load_screen_row(screen, i, s0, s1, s2)) return;
    const int M = f.M;
    BwdIn<DEG, RAW> b;
    load_backward_inputs<DEG, RAW, false>(f, i, view, proj, campos, means, scales, rots, covpre, opac, shs, shs_rest, has_colpre, clamped, s0,
                                          s1, s2, nullptr, b);
    GeomGrad g;
    float dsh[3 * (DEG + 1) * (DEG + 1)];          // constant indices only: stays in registers
    geom_backward_one<DEG>(f, b.V, b.PV, b.cp, b.in.p, b.in.sc, b.in.q, b.in.cov(covpre), b.in.sh(), has_colpre != 0, b.clamp_bits,
                           b.sg, g, dsh, shs != nullptr);
    if constexpr (RAW) activate_raw_backward(b.in.act, g);
    store_geom_grad(out, i, g, has_colpre, covpre);
    constexpr int K3 = 3 * (DEG + 1) * (DEG + 1);
    if constexpr (RAW == 1) {
        if (out.shs) { out.shs[3 * (size_t)i] = dsh[0]; out.shs[3 * (size_t)i + 1] = dsh[1]; out.shs[3 * (size_t)i + 2] = dsh[2]; }
        if (out.shs_rest) {
            float *dst = out.shs_rest + (size_t)i * (M - 1) * 3;
#pragma unroll
            for (int k = 3; k < K3; ++k) dst[k - 3] = dsh[k];
        }
    } else if (out.shs && shs) {
        float *dst = out.shs + (size_t)i * M * 3;
#pragma unroll
        for (int k = 0; k < K3; ++k)
            if (k < 3 * M) dst[k] = dsh[k];
    }
}

// ---- the aux backward's z chain: z = (means3D . viewmatrix)_z in the header's row-vector convention, so dL/dmeans3D gains
// dL/dz (V[0][2], V[1][2], V[2][2]) = dL/dz (view[2], view[6], view[10]); dL/dz is screen_grads slot 9.  Runs behind the geometry
// backward over the same rows (SPARSE: the ranks it visited; otherwise [g0, g0 + n)) and adds to the means3D rows it wrote.
template <bool SPARSE>
__global__ __launch_bounds__(kGeomBlock) void k_geom_bwd_depth(int g0, int n, int P, const uint32_t *__restrict__ order,
                                                               const uint32_t *__restrict__ cnt_open, const float *__restrict__ view,
                                                               const int32_t *__restrict__ radii, const float4 *__restrict__ screen,
                                                               float *__restrict__ dmeans)
{
    const int t = blockIdx.x * kGeomBlock + threadIdx.x;
    if (t >= n) return;
    const int i = visit_row<SPARSE>(t, g0, order, cnt_open, P, radii);
    if (i < 0) return;
    const float dz = screen[3 * (size_t)i + 2].y;
    if (dz == 0.f) return;
    dmeans[3 * (size_t)i] += dz * view[2];
    dmeans[3 * (size_t)i + 1] += dz * view[6];
    dmeans[3 * (size_t)i + 2] += dz * view[10];
}

// ---- absgrad: screen_grads slots 10, 11 (the abs blend backward's per-pixel absolute sums of d/dmean2D) as a [P,3] tensor laid out
// like the means2D gradient.  The rows the geometry backward visits (visit_row) get (slot 10, slot 11, 0); every other row is zero:
// DENSE writes it here, SPARSE relies on the caller's fill - rows outside the binned prefix are never read.
template <bool SPARSE>
__global__ __launch_bounds__(kGeomBlock) void k_screen_absgrad(int n, int P, const uint32_t *__restrict__ order,
                                                               const uint32_t *__restrict__ cnt_open, const int32_t *__restrict__ radii,
                                                               const float4 *__restrict__ screen, float *__restrict__ out)
{
    const int t = blockIdx.x * kGeomBlock + threadIdx.x;
    if (t >= n) return;
    const int i = visit_row<SPARSE>(t, 0, order, cnt_open, P, radii);
    if constexpr (SPARSE) {
        if (i < 0) return;
    }
    const int row = SPARSE ? i : t;
    float ax = 0.f, ay = 0.f;
    if (i >= 0) { const float4 s2 = screen[3 * (size_t)i + 2]; ax = s2.z; ay = s2.w; }
    out[3 * (size_t)row] = ax; out[3 * (size_t)row + 1] = ay; out[3 * (size_t)row + 2] = 0.f;
}

// ---- camera gradients: dL/dviewmatrix, dL/dprojmatrix, dL/dcampos = sums over Gaussians of camera_backward_one's
// 27 terms.  Runs behind the geometry backward over the rows it visited (SPARSE: the ranks of the binned depth prefix through
// order / cnt_open; otherwise [0, n)).  Every sum has an order the program fixes, so the result is bit-reproducible: the lanes of a
// wave by DPP adds (each row of 16 lanes by a butterfly that leaves the row's sum in all of its lanes, then the four rows in
// row order), the waves of a block through LDS in wave order, one 27-float partial per block (at most kCamMaxBlocks blocks, each
// thread striding over the rows in increasing order); k_camera_reduce adds the partials in block order.  No global atomics.  Invisible, dead (all-zero row) and out-of-range lanes contribute exact zeros.
template <int CTRL>
__device__ __forceinline__ float dpp_add(float v)
{
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

__device__ __forceinline__ float wave_sum_fixed(float v)
{
    v = dpp_add<0xB1>(v);          // quad_perm:[1,0,3,2]
    v = dpp_add<0x4E>(v);          // quad_perm:[2,3,0,1]
    v = dpp_add<0x141>(v);         // row_half_mirror
    v = dpp_add<0x140>(v);         // row_mirror: every lane of a row of 16 holds the row's sum
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 0));
    const float r1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 32));
    const float r3 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 48));
    return ((r0 + r1) + r2) + r3;
}

constexpr int kCamMaxBlocks = 1024;    // four blocks per CU; k_camera_reduce then adds at most 32 partials per thread

template <int DEG, int RAW, bool SPARSE>
__global__ __launch_bounds__(kGeomBlock) void k_camera_bwd(FrameK f, int n, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ cnt_open, const float *__restrict__ view,
                                                           const float *__restrict__ proj, const float *__restrict__ campos,
                                                           const float *__restrict__ means, const float *__restrict__ scales,
                                                           const float *__restrict__ rots, const float *__restrict__ covpre,
                                                           const float *__restrict__ opac, const float *__restrict__ shs,
                                                           const float *__restrict__ shs_rest, int has_colpre,
                                                           const int32_t *__restrict__ radii, const uint8_t *__restrict__ clamped,
                                                           const float4 *__restrict__ screen, int depth_chain,
                                                           float *__restrict__ partials)
{
    __shared__ float wave_part[kGeomBlock / 64][kCamTerms];
    float c[kCamTerms];
#pragma unroll
    for (int k = 0; k < kCamTerms; ++k) c[k] = 0.f;
    // grid-stride: at most kCamMaxBlocks blocks (and partials); a thread adds its Gaussians' terms in increasing index order
    for (int t = blockIdx.x * kGeomBlock + threadIdx.x; t < n; t += (int)gridDim.x * kGeomBlock) {
        const int i = visit_row<SPARSE>(t, 0, order, cnt_open, f.P, radii);
        if (i < 0) continue;
        float4 s0, s1, s2;
        const bool live = load_screen_row(screen, i, s0, s1, s2);
        const float dz = depth_chain ? s2.y : 0.f;
        if (live) {
            BwdIn<DEG, RAW> b;
            load_backward_inputs<DEG, RAW, false>(f, i, view, proj, campos, means, scales, rots, covpre, opac, shs, shs_rest, has_colpre,
                                                  clamped, s0, s1, s2, nullptr, b);
            camera_backward_one<DEG>(f, b.V, b.PV, b.cp, b.in.p, b.in.sc, b.in.q, b.in.cov(covpre), b.in.sh(), has_colpre != 0, b.clamp_bits,
                                     b.sg, c);
        }
        if (dz != 0.f) {                             // the depth map's chain (k_geom_bwd_depth's rows): z = sum_r ph_r V[4r+2]
            c[2] += means[3 * i] * dz; c[5] += means[3 * i + 1] * dz; c[8] += means[3 * i + 2] * dz; c[11] += dz;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < kCamTerms; ++k) {
        const float s = wave_sum_fixed(c[k]);
        if (lane == 0) wave_part[wv][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < kCamTerms) {
        float s = wave_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kGeomBlock / 64; ++w) s += wave_part[w][threadIdx.x];
        partials[(size_t)blockIdx.x * kCamTerms + threadIdx.x] = s;
    }
}

// Second launch: one block adds the per-block partials in block order.  The sums cancel (sum |t_i| / |sum t_i| of a few hundred
// on deep frames), so they are accumulated in binary64, full rate on this part: thread (g, k) adds term k of the blocks
// [g chunk, (g + 1) chunk) in order, then term k's kCamGroups group sums are added in group order.  Writes the three tensors, the
// structural zeros (column 3 of dview, column 2 of dproj) included; any output may be NULL.  n_blocks == 0 writes zeros.
constexpr int kCamReduceBlock = 1024, kCamGroups = kCamReduceBlock / 32;

__global__ __launch_bounds__(kCamReduceBlock) void k_camera_reduce(int n_blocks, const float *__restrict__ partials,
                                                                   float *__restrict__ dview, float *__restrict__ dproj,
                                                                   float *__restrict__ dcampos)
{
    __shared__ double group_sum[kCamGroups][kCamTerms];
    const int k = threadIdx.x & 31, g = threadIdx.x >> 5;
    const int chunk = (n_blocks + kCamGroups - 1) / kCamGroups;
    if (k < kCamTerms) {
        double s = 0.0;
        const int b1 = min(n_blocks, (g + 1) * chunk);
        for (int b = g * chunk; b < b1; ++b) s += (double)partials[(size_t)b * kCamTerms + k];
        group_sum[g][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < 35) {
        const int e = threadIdx.x;                  // dview[16] | dproj[16] | dcampos[3]
        int term = -1;
        if (e < 16) { if ((e & 3) != 3) term = 3 * (e >> 2) + (e & 3); }
        else if (e < 32) { const int col = e & 3; if (col != 2) term = 12 + 3 * ((e - 16) >> 2) + (col == 3 ? 2 : col); }
        else term = 24 + (e - 32);
        double s = 0.0;
        if (term >= 0)
            for (int gg = 0; gg < kCamGroups; ++gg) s += group_sum[gg][term];
        const float v = (float)s;
        if (e < 16) { if (dview) dview[e] = v; }
        else if (e < 32) { if (dproj) dproj[e - 16] = v; }
        else if (dcampos) dcampos[e - 32] = v;
    }
}

size_t camera_grad_workspace_bytes(int P)
{
    const size_t blocks = ((size_t)(P > 0 ? P : 0) + kGeomBlock - 1) / kGeomBlock;
    return align_up((blocks > 0 ? blocks : 1) * kCamTerms * sizeof(float));
}

int launch_camera_bwd(const FrameK &f, const gsr_camera &cam, const gsr_gaussians &g, const int32_t *radii, const GeomWS &gw,
                      const float *screen_grads, const GeomRows &rows, bool depth_chain, float *partials, const gsr_camera_grads &out,
                      bool debug, hipStream_t s)
{
    const int n = rows.count();
    const int grid = min((n + kGeomBlock - 1) / kGeomBlock, kCamMaxBlocks);
    if (grid > 0) {
        ProfileScope prof("camera_bwd", s);
        dispatch_deg_raw<3>(f.D, raw_mode(g), [&](auto deg, auto raw) {
            auto *kernel = rows.sparse ? k_camera_bwd<decltype(deg)::value, decltype(raw)::value, true>
                                       : k_camera_bwd<decltype(deg)::value, decltype(raw)::value, false>;
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(kGeomBlock), 0, s, f, n, rows.rows, rows.cnt_open, cam.viewmatrix,
                               cam.projmatrix, cam.campos, g.means3D, g.scales, g.rotations, g.cov3D_precomp, g.opacities, g.shs,
                               g.shs_rest, g.colors_precomp ? 1 : 0, radii, gw.clamped, reinterpret_cast<const float4 *>(screen_grads),
                               depth_chain ? 1 : 0, partials);
        });
        GSR_LAUNCH_CHECK("camera_bwd", debug, s);
    }
    ProfileScope prof("camera_reduce", s);
    hipLaunchKernelGGL(k_camera_reduce, dim3(1), dim3(kCamReduceBlock), 0, s, grid, partials, out.viewmatrix, out.projmatrix, out.campos);
    GSR_LAUNCH_CHECK("camera_reduce", debug, s);
    return GSR_OK;
}

// ---- one launch that zero-fills up to nine output tensors (the sparse path's "memset"): the segments are laid end to
// end in a virtual float index space; each thread clears a float4 where the 16 bytes lie inside one segment.
__global__ __launch_bounds__(kGeomBlock) void k_zero_segments(ZeroSegs z)
{
    const unsigned block = blockIdx.x, blocks = gridDim.x;
    const size_t total = z.end[z.n - 1];
    const size_t stride = (size_t)blocks * kGeomBlock * 4;
    for (size_t v = ((size_t)block * kGeomBlock + threadIdx.x) * 4; v < total; v += stride) {
        int sgm = 0;
        while (v >= z.end[sgm]) ++sgm;
        const size_t off = v - (sgm ? z.end[sgm - 1] : 0);           // multiple of 4 inside the segment
        float *p = z.ptr[sgm] + off;
        if (off + 4 <= z.len[sgm] && (((uintptr_t)p) & 15) == 0) *reinterpret_cast<float4 *>(p) = make_float4(0.f, 0.f, 0.f, 0.f);
        else
            for (int e = 0; e < 4; ++e)
                if (off + e < z.len[sgm]) p[e] = 0.f;
    }
}

ZeroSegs zero_segments(const FrameK &f, const gsr_gaussians &g, float *screen, const gsr_grads &out, uint8_t *row_valid, size_t valid_bytes)
{
    const size_t P = (size_t)f.P;
    ZeroSegs z;
    z.n = 0;
    auto add = [&](float *ptr, size_t floats) {
        if (ptr && floats) { z.ptr[z.n] = ptr; z.len[z.n] = floats; z.end[z.n] = (z.n ? z.end[z.n - 1] : 0) + ((floats + 3) & ~(size_t)3); ++z.n; }
    };
    add(screen, P * kRowFloats);
    add(out.means3D, P * 3);
    add(out.means2D, P * 3);
    add(out.opacities, P);
    if (g.colors_precomp) add(out.colors_precomp, P * 3);
    if (!g.cov3D_precomp) { add(out.scales, P * 3); add(out.rotations, P * 4); }
    if (g.cov3D_precomp) add(out.cov3D_precomp, P * 6);
    const bool split = raw_split_sh(g);
    if (g.shs) add(out.shs, P * 3 * (size_t)(split ? 1 : f.M));
    if (split && f.M > 1) add(out.shs_rest, P * 3 * (size_t)(f.M - 1));
    if (row_valid && valid_bytes) add(reinterpret_cast<float *>(row_valid), (valid_bytes + 3) / 4);     // (a 256-byte aligned, padded block)
    return z;
}

// zero-fill of the backward's outputs in ONE launch: screen-space gradients (optional) + every wanted parameter gradient
int launch_zero_outputs(const FrameK &f, const gsr_gaussians &g, float *screen, const gsr_grads &out, hipStream_t s,
                        uint8_t *row_valid, size_t valid_bytes)
{
    return launch_zero_segments(zero_segments(f, g, screen, out, row_valid, valid_bytes), s);
}

int launch_zero_segments(const ZeroSegs &z, hipStream_t s)
{
    if (z.n == 0) return GSR_OK;
    const size_t total = z.end[z.n - 1];
    size_t blocks = (total / 4 + kGeomBlock - 1) / kGeomBlock / 4 + 1;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_zero_segments, dim3((unsigned)blocks), dim3(kGeomBlock), 0, s, z);
    GSR_LAUNCH_CHECK("zero_outputs", false, s);
    return GSR_OK;
}

// the aux backward's z chain (k_geom_bwd_depth), behind launch_geom_bwd of the same arguments: over the rows it visited
int launch_geom_bwd_depth(const FrameK &f, const gsr_camera &cam, const int32_t *radii, const float *screen_grads, const GeomRows &rows,
                          float *dmeans, bool debug, hipStream_t s)
{
    const int n = rows.count();
    if (!dmeans || n <= 0) return GSR_OK;
    ProfileScope prof("geom_bwd_depth", s);
    const dim3 grid((unsigned)((n + kGeomBlock - 1) / kGeomBlock));
    const float4 *screen = reinterpret_cast<const float4 *>(screen_grads);
    hipLaunchKernelGGL(rows.sparse ? k_geom_bwd_depth<true> : k_geom_bwd_depth<false>, grid, dim3(kGeomBlock), 0, s, rows.sparse ? 0 : rows.g0,
                       n, f.P, rows.rows, rows.cnt_open, cam.viewmatrix, radii, screen, dmeans);
    GSR_LAUNCH_CHECK("geom_bwd_depth", debug, s);
    return GSR_OK;
}

int launch_screen_absgrad(const FrameK &f, const int32_t *radii, const float *screen_grads, const GeomRows &rows, float *out, bool debug,
                          hipStream_t s)
{
    if (f.P <= 0) return GSR_OK;
    ProfileScope prof("screen_absgrad", s);
    if (rows.sparse) GSR_HIP_CHECK(hipMemsetAsync(out, 0, (size_t)f.P * 3 * sizeof(float), s));
    const int n = rows.count();
    if (n > 0) {
        const dim3 grid((unsigned)((n + kGeomBlock - 1) / kGeomBlock));
        const float4 *screen = reinterpret_cast<const float4 *>(screen_grads);
        hipLaunchKernelGGL(rows.sparse ? k_screen_absgrad<true> : k_screen_absgrad<false>, grid, dim3(kGeomBlock), 0, s, n, f.P, rows.rows,
                           rows.cnt_open, radii, screen, out);
    }
    GSR_LAUNCH_CHECK("screen_absgrad", debug, s);
    return GSR_OK;
}

int launch_geom_bwd(const FrameK &f, const gsr_camera &cam, const gsr_gaussians &g, const int32_t *radii, const GeomWS &gw,
                    const float *screen_grads, const GeomRows &rows, const gsr_grads &out, bool debug, hipStream_t s)
{
    const int g0 = rows.g0, g1 = rows.g1, n_ranks = rows.n_ranks;
    if (g1 <= g0) return GSR_OK;
    if (rows.sparse) {
        // depth-complex frame: almost every gradient row is zero -> memset the outputs, then visit the binned prefix only
        ProfileScope prof("geom_bwd", s);
        int rc0;
        if (!out.prezeroed && (rc0 = launch_zero_outputs(f, g, nullptr, out, s))) return rc0;
        if (n_ranks > 0) {
            const int sgrid = (n_ranks + kGeomBlock - 1) / kGeomBlock;
            dispatch_deg_raw<3>(f.D, raw_mode(g), [&](auto deg, auto raw) {
                hipLaunchKernelGGL((k_geom_bwd_sparse<decltype(deg)::value, decltype(raw)::value>), dim3(sgrid), dim3(kGeomBlock), 0, s, f,
                                   n_ranks, rows.rows, cam.viewmatrix, cam.projmatrix, cam.campos, g.means3D, g.scales, g.rotations,
                                   g.cov3D_precomp, g.opacities, g.shs, g.shs_rest, g.colors_precomp ? 1 : 0, radii, gw.clamped,
                                   reinterpret_cast<const float4 *>(screen_grads), out, rows.cnt_open);
            });
        }
        GSR_LAUNCH_CHECK("geom_bwd_sparse", debug, s);
        return GSR_OK;
    }
    const int grid = (g1 - g0 + kGeomBlock - 1) / kGeomBlock;
    ProfileScope prof("geom_bwd", s);
    dispatch_deg_raw<3>(f.D, raw_mode(g), [&](auto deg, auto raw) {
        hipLaunchKernelGGL((k_geom_bwd<decltype(deg)::value, decltype(raw)::value>), dim3(grid), dim3(kGeomBlock), 0, s, f, g0, g1,
                           cam.viewmatrix, cam.projmatrix, cam.campos, g.means3D, g.scales, g.rotations, g.cov3D_precomp, g.opacities,
                           g.shs, g.shs_rest, g.colors_precomp ? 1 : 0, radii, gw.clamped, reinterpret_cast<const float4 *>(screen_grads),
                           out);
    });
    GSR_LAUNCH_CHECK("geom_bwd", debug, s);
    return GSR_OK;
}

__global__ __launch_bounds__(kGeomBlock) void k_mark_visible(int P, const float *__restrict__ means,
                                                             const float *__restrict__ view, uint8_t *__restrict__ present)
{
    const int i = blockIdx.x * kGeomBlock + threadIdx.x;
    if (i >= P) return;
    float V[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) V[k] = view[k];
    const float p[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
    present[i] = in_frustum(p, V) ? 1 : 0;
}

int launch_mark_visible(int P, const float *means3D, const float *view, uint8_t *present, hipStream_t s)
{
    if (P == 0) return GSR_OK;
    hipLaunchKernelGGL(k_mark_visible, dim3((P + kGeomBlock - 1) / kGeomBlock), dim3(kGeomBlock), 0, s, P, means3D, view, present);
    GSR_LAUNCH_CHECK("mark_visible", false, s);
    return GSR_OK;
}

}  // namespace gsr
