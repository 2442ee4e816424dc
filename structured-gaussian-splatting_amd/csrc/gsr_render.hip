// gsr_render.hip — per-tile alpha blending, forward (K6) and backward (K7), plus the deterministic
// per-Gaussian reduction of the backward's instance rows.  Spec: SURVEY A.8 / A.9.
//
// MI355X mapping ("one wave, one tile"):
//   * forward: a 16x16 binning tile is blended by ONE wave64.  Chunks of large splats (k_render_fwd<QuadrantLanes>): lane l owns the pixel
//     (l & 7, l >> 3) of each of the tile's four 8x8 QUADRANTS, so "can this splat reach quadrant k at all" is wave-uniform and
//     clear quadrants are skipped with scalar branches (sub-tile culling); early termination is a wave ballot per quadrant.
//     Chunks of small splats (k_render_fwd<GroupLanes>): the backward's mapping, one 16-lane group per quadrant, each walking its own
//     entries.  Both kernels are one body (render_fwd) over the pixel mapping (QuadrantLanes, GroupLanes), so they render the same
//     bits and leave the checkpoints in one layout (ckpt_word).  No workgroup barrier exists anywhere in the blend loops.
//   * splat records (48 B: xy, conic, opacity, rgb) are gathered 64 at a time, one per lane, staged in
//     LDS and read back as broadcasts (ds_read_b128).
//   * backward: FRONT TO BACK, in independent work units of kSeg list entries (gsr_internal.h: kSeg, UnitLists) that start from the
//     per-pixel state the forward left at the segment boundary.  The wave is four GROUPS of 16 lanes, one per quadrant, each
//     walking the entries that reach ITS quadrant: up to four different splats per pass, one DPP butterfly over the rows of 16
//     lanes for all four (k_render_bwd).  The sums of a batch of 64 entries meet in LDS and leave as whole 48-B rows, one per
//     list entry (no global atomics; one valid byte per row says whether it was written).
//   * workgroup = one wave (64 threads); forward: tile = block (consecutive tiles run on different XCDs).
#include "gsr_internal.h"

namespace gsr {

__device__ __forceinline__ float fast_exp(float x)
{
    // v_exp_f32 computes 2^x; same function in forward and backward (SURVEY 7 "expf accuracy").
    return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
}

__device__ __forceinline__ float fast_rcp(float x) { return __builtin_amdgcn_rcpf(x); }

// Nine sums over each ROW of 16 lanes, all four rows at once (k_render_bwd's quadrant groups): a transposing butterfly.  The first
// two steps fold two values per instruction (bank_mask picks the half / the quads that keep a value), the two steps inside a quad
// run on the three registers that are left: 20 DPP adds for four splats.  On return every lane of a quad holds, with b = the quad's
// number in the row:   a[0]: value (0, 1, 4, 5)[b]     a[2]: value (2, 3, 6, 7)[b]     a[8]: value 8
// DPP hazard (a VALU write followed by a DPP read of the same register needs two wait states) is covered by the order and s_nops.
__device__ __forceinline__ void row_sum9_transpose(float (&a)[9])
{
#define GSR_DPP(d, s_, ctrl, bank) "v_add_f32_dpp %" #d ", %" #s_ ", %" #s_ " " ctrl " row_mask:0xf bank_mask:" bank "\n\t"
    asm volatile("s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_ror:8", "0x3") GSR_DPP(1, 1, "row_ror:8", "0x3") GSR_DPP(2, 2, "row_ror:8", "0x3")
                 GSR_DPP(3, 3, "row_ror:8", "0x3") GSR_DPP(8, 8, "row_ror:8", "0xf")
                 GSR_DPP(0, 4, "row_ror:8", "0xc") GSR_DPP(1, 5, "row_ror:8", "0xc") GSR_DPP(2, 6, "row_ror:8", "0xc")
                 GSR_DPP(3, 7, "row_ror:8", "0xc")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_half_mirror", "0x5") GSR_DPP(2, 2, "row_half_mirror", "0x5") GSR_DPP(8, 8, "row_half_mirror", "0xf")
                 GSR_DPP(0, 1, "row_half_mirror", "0xa") GSR_DPP(2, 3, "row_half_mirror", "0xa")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "quad_perm:[1,0,3,2]", "0xf") GSR_DPP(2, 2, "quad_perm:[1,0,3,2]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[1,0,3,2]", "0xf")
                 "s_nop 0\n\t"
                 GSR_DPP(0, 0, "quad_perm:[2,3,0,1]", "0xf") GSR_DPP(2, 2, "quad_perm:[2,3,0,1]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[2,3,0,1]", "0xf")
                 "s_nop 1"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]));
#undef GSR_DPP
}
// The same butterfly with a tenth value (the aux backward's sum of w dL/ddepth), reduced over the row like value 8 - four more DPP
// adds, each placed right behind value 8's, so the wait states above cover it:   a[9]: value 9 in every lane of the row
__device__ __forceinline__ void row_sum10_transpose(float (&a)[10])
{
#define GSR_DPP(d, s_, ctrl, bank) "v_add_f32_dpp %" #d ", %" #s_ ", %" #s_ " " ctrl " row_mask:0xf bank_mask:" bank "\n\t"
    asm volatile("s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_ror:8", "0x3") GSR_DPP(1, 1, "row_ror:8", "0x3") GSR_DPP(2, 2, "row_ror:8", "0x3")
                 GSR_DPP(3, 3, "row_ror:8", "0x3") GSR_DPP(8, 8, "row_ror:8", "0xf") GSR_DPP(9, 9, "row_ror:8", "0xf")
                 GSR_DPP(0, 4, "row_ror:8", "0xc") GSR_DPP(1, 5, "row_ror:8", "0xc") GSR_DPP(2, 6, "row_ror:8", "0xc")
                 GSR_DPP(3, 7, "row_ror:8", "0xc")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_half_mirror", "0x5") GSR_DPP(2, 2, "row_half_mirror", "0x5") GSR_DPP(8, 8, "row_half_mirror", "0xf")
                 GSR_DPP(9, 9, "row_half_mirror", "0xf")
                 GSR_DPP(0, 1, "row_half_mirror", "0xa") GSR_DPP(2, 3, "row_half_mirror", "0xa")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "quad_perm:[1,0,3,2]", "0xf") GSR_DPP(2, 2, "quad_perm:[1,0,3,2]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[1,0,3,2]", "0xf") GSR_DPP(9, 9, "quad_perm:[1,0,3,2]", "0xf")
                 "s_nop 0\n\t"
                 GSR_DPP(0, 0, "quad_perm:[2,3,0,1]", "0xf") GSR_DPP(2, 2, "quad_perm:[2,3,0,1]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[2,3,0,1]", "0xf") GSR_DPP(9, 9, "quad_perm:[2,3,0,1]", "0xf")
                 "s_nop 1"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]),
                   "+v"(a[9]));
#undef GSR_DPP
}

// The abs backward's butterfly: values 9 and 10 (the sums of |d/dmean2D.x|, |d/dmean2D.y| per pixel) are reduced over the row like
// value 8, each step's adds right behind value 8's (more instructions between a write and its DPP read, never fewer):
//   a[9], a[10]: values 9, 10 in every lane of the row
__device__ __forceinline__ void row_sum11_transpose(float (&a)[11])
{
#define GSR_DPP(d, s_, ctrl, bank) "v_add_f32_dpp %" #d ", %" #s_ ", %" #s_ " " ctrl " row_mask:0xf bank_mask:" bank "\n\t"
    asm volatile("s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_ror:8", "0x3") GSR_DPP(1, 1, "row_ror:8", "0x3") GSR_DPP(2, 2, "row_ror:8", "0x3")
                 GSR_DPP(3, 3, "row_ror:8", "0x3") GSR_DPP(8, 8, "row_ror:8", "0xf") GSR_DPP(9, 9, "row_ror:8", "0xf")
                 GSR_DPP(10, 10, "row_ror:8", "0xf")
                 GSR_DPP(0, 4, "row_ror:8", "0xc") GSR_DPP(1, 5, "row_ror:8", "0xc") GSR_DPP(2, 6, "row_ror:8", "0xc")
                 GSR_DPP(3, 7, "row_ror:8", "0xc")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "row_half_mirror", "0x5") GSR_DPP(2, 2, "row_half_mirror", "0x5") GSR_DPP(8, 8, "row_half_mirror", "0xf")
                 GSR_DPP(9, 9, "row_half_mirror", "0xf") GSR_DPP(10, 10, "row_half_mirror", "0xf")
                 GSR_DPP(0, 1, "row_half_mirror", "0xa") GSR_DPP(2, 3, "row_half_mirror", "0xa")
                 "s_nop 1\n\t"
                 GSR_DPP(0, 0, "quad_perm:[1,0,3,2]", "0xf") GSR_DPP(2, 2, "quad_perm:[1,0,3,2]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[1,0,3,2]", "0xf") GSR_DPP(9, 9, "quad_perm:[1,0,3,2]", "0xf")
                 GSR_DPP(10, 10, "quad_perm:[1,0,3,2]", "0xf")
                 "s_nop 0\n\t"
                 GSR_DPP(0, 0, "quad_perm:[2,3,0,1]", "0xf") GSR_DPP(2, 2, "quad_perm:[2,3,0,1]", "0xf")
                 GSR_DPP(8, 8, "quad_perm:[2,3,0,1]", "0xf") GSR_DPP(9, 9, "quad_perm:[2,3,0,1]", "0xf")
                 GSR_DPP(10, 10, "quad_perm:[2,3,0,1]", "0xf")
                 "s_nop 1"
                 : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]),
                   "+v"(a[9]), "+v"(a[10]));
#undef GSR_DPP
}

// The ext backward's three further values (the sums of w dL/dextra): each reduced over its row of 16 lanes by value 8's four steps, in
// an asm of their own behind row_sum10_transpose - three adds per step and an s_nop 1 between the steps, so every DPP read is at
// least two wait states behind the write of its register:   b[0..2]: the row's totals in every lane of the row
__device__ __forceinline__ void row_sum3_rows(float (&b)[3])
{
#define GSR_DPP(d, ctrl) "v_add_f32_dpp %" #d ", %" #d ", %" #d " " ctrl " row_mask:0xf bank_mask:0xf\n\t"
    asm volatile("s_nop 1\n\t"
                 GSR_DPP(0, "row_ror:8") GSR_DPP(1, "row_ror:8") GSR_DPP(2, "row_ror:8")
                 "s_nop 1\n\t"
                 GSR_DPP(0, "row_half_mirror") GSR_DPP(1, "row_half_mirror") GSR_DPP(2, "row_half_mirror")
                 "s_nop 1\n\t"
                 GSR_DPP(0, "quad_perm:[1,0,3,2]") GSR_DPP(1, "quad_perm:[1,0,3,2]") GSR_DPP(2, "quad_perm:[1,0,3,2]")
                 "s_nop 1\n\t"
                 GSR_DPP(0, "quad_perm:[2,3,0,1]") GSR_DPP(1, "quad_perm:[2,3,0,1]") GSR_DPP(2, "quad_perm:[2,3,0,1]")
                 "s_nop 1"
                 : "+v"(b[0]), "+v"(b[1]), "+v"(b[2]));
#undef GSR_DPP
}

__device__ __forceinline__ int wave_max_uniform(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    return __builtin_amdgcn_readfirstlane(v);
}

constexpr int kFwdWaves = 5;       // resident waves per SIMD the register allocation of the forward kernels aims for
constexpr int kBwdWaves = 4;       // ... and of k_render_bwd
constexpr int kFwdExtWaves = 4;    // ... of the ext forward instantiations (the aux ones' value)
typedef float v2f __attribute__((ext_vector_type(2)));      // packed-fp32 operand: the lane's two pixels of a pair

// lp = log2(opacity exp(power)) of a pair of pixels from the pre-scaled record (qA, qB, qC = a.z, a.w, b.x; log2 opacity = b.y):
//     lp = qA dx^2 + qB dx dy + qC dy^2 + lop = ((qC dy + qB dx) dy) + (qA dx) dx + lop
// ONE definition for the three blend kernels, with every rounding spelled out (no contraction left to the compiler): the forward
// kernels and the backward then agree on every pixel's lp - and with it on alpha, on the accept / stop decisions and on the
// transmittance - bit for bit, whichever kernel rendered the frame.
struct LpTerms { v2f axx, bx; };
__device__ __forceinline__ LpTerms lp_terms(float qA, float qB, float lop, v2f dx)
{
#pragma clang fp contract(off)
    LpTerms t;
    const v2f adx = qA * dx;                                               // rounded
    t.axx = __builtin_elementwise_fma(adx, dx, v2f{lop, lop});             // (qA dx) dx + lop
    t.bx = qB * dx;                                                        // rounded
    return t;
}
__device__ __forceinline__ v2f lp_at(const LpTerms &t, float qC, float dy)
{
#pragma clang fp contract(off)
    const v2f s = __builtin_elementwise_fma(v2f{qC, qC}, v2f{dy, dy}, t.bx);        // qC dy + qB dx
    return __builtin_elementwise_fma(s, v2f{dy, dy}, t.axx);
}

// Stage up to 64 records (one per lane) of a tile's list into LDS; returns the lane's quadrant mask (bits 28..31 of the
// sorted list's entry, put there by the emit kernels: gsr_binning.hip).  entry (optional): the lane's whole list entry (mask and
// Gaussian index) for a caller that needs the index behind the batch; untouched in the lanes behind a short batch's end.
__device__ __forceinline__ unsigned stage_batch(float4 *sh_rec, int lane, int n, const uint32_t *__restrict__ sorted_gid, uint32_t first,
                                                const float4 *__restrict__ records, uint32_t *entry = nullptr)
{
    unsigned m = 0;
    if (lane < n) {
        const uint32_t v = sorted_gid[first + lane];
        if (entry) *entry = v;
        m = v >> kQuadMaskShift;
        const float4 *r = records + 3 * (size_t)(v & kGidMask);
        sh_rec[3 * lane + 0] = r[0];
        sh_rec[3 * lane + 1] = r[1];
        sh_rec[3 * lane + 2] = r[2];
    }
    return m;
}
// stage_batch of the ext kernels: the same lanes also gather their Gaussian's row of the extra table, by the entry's index, into a
// second LDS array beside sh_rec.  (A function of its own: stage_batch, and with it every other instantiation, stays as it is.)
__device__ __forceinline__ unsigned stage_batch_ext(float4 *sh_rec, float4 *sh_ext, int lane, int n, const uint32_t *__restrict__ sorted_gid,
                                                    uint32_t first, const float4 *__restrict__ records, const float4 *__restrict__ ext_table)
{
    uint32_t entry = 0;
    const unsigned m = stage_batch(sh_rec, lane, n, sorted_gid, first, records, &entry);
    if (lane < n) sh_ext[lane] = ext_table[entry & kGidMask];
    return m;
}

// ------------------------------------------------------------------------------------------- K6
// One launch per depth chunk.  A tile's wave resumes the pixels' state (T, colour, last contributor) where
// the previous chunk left it, blends the chunk's range, and closes the tile once all 256 pixels have
// taken the cut-off.  State lives in the image workspace: T_state (negative = done), last_enc, and the
// un-finalised colour in out_color itself; the background term is added exactly once, when the tile
// closes or after the last chunk.
//
// The alpha >= 1/255 test (A.8) is taken on the exponent: lp = log2(opacity exp(power)) < log2(1/255).  Forward and backward use
// the same constant on the same lp, so they agree on every pixel; against alpha = opacity * exp(power) < 1/255 in exact
// arithmetic the two rules differ only where alpha sits within rounding of the threshold (the oracle's fragile band).
constexpr float kLog2AlphaMin = -7.99435343685886f;      // log2(1 / 255)

// Per pixel: T (signed, see FwdPair), colour, last contributor.  A rejected splat runs the same arithmetic with alpha = 0, which leaves
// everything unchanged, so the only selects are on alpha, on the stop decision and on the contributor index.
struct FwdPair {             // state of a lane's two pixels in one pair (elements 0, 1 or 2, 3)
    v2f T, Cr, Cg, Cb;       // T > 0: live transmittance; T < 0: the pixel has taken the cut-off (or lies outside the image), |T| = the
    int last0, last1;        // transmittance to report (frozen in front of the stopping splat): exactly what T_state holds
};

// One register per pixel carries both "live transmittance" and "final transmittance of a done pixel": for a done pixel
// test_T = T (1 - alpha) is negative, so the stop test fires by itself, nothing is composited and T keeps its value.
// ONE definition for both forward kernels (active: the lane's group has a splat in this pass - always, in the lock-step kernel).
// Returns the pair's blend weights w = alpha T (0 where nothing was composited): the aux instantiations blend the depth with them.
__device__ __forceinline__ v2f fwd_pair(bool active, v2f lp, float lop, float cr, float cg, float cb, int contributor, FwdPair &P)
{
    const bool keep0 = active && !(lp[0] > lop) && !(lp[0] < kLog2AlphaMin);      // power > 0  <=>  lp > lop;  alpha < 1/255  <=>  lp < log2(1/255)
    const bool keep1 = active && !(lp[1] > lop) && !(lp[1] < kLog2AlphaMin);
    // a rejected pixel gets lp = -inf: exp2 gives alpha = 0 by itself (one select per pixel, in front of the exponential)
    const v2f ae = {fminf((float)GSR_ALPHA_MAX, __builtin_amdgcn_exp2f(keep0 ? lp[0] : -INFINITY)),
                    fminf((float)GSR_ALPHA_MAX, __builtin_amdgcn_exp2f(keep1 ? lp[1] : -INFINITY))};
    const v2f test_T = P.T * (1.f - ae);                       // == T when rejected, negative when already done
    const v2f aT = ae * P.T;
    const bool stop0 = test_T[0] < (float)GSR_T_CUTOFF;        // live + accepted + below the cut-off, or done
    const bool stop1 = test_T[1] < (float)GSR_T_CUTOFF;
    const v2f w = {stop0 ? 0.f : aT[0], stop1 ? 0.f : aT[1]};  // the stopping splat is NOT composited (A.8)
    P.Cr = __builtin_elementwise_fma(v2f{cr, cr}, w, P.Cr);
    P.Cg = __builtin_elementwise_fma(v2f{cg, cg}, w, P.Cg);
    P.Cb = __builtin_elementwise_fma(v2f{cb, cb}, w, P.Cb);
    P.T = v2f{stop0 ? -fabsf(P.T[0]) : test_T[0], stop1 ? -fabsf(P.T[1]) : test_T[1]};
    P.last0 = (keep0 && !stop0) ? contributor : P.last0;
    P.last1 = (keep1 && !stop1) ? contributor : P.last1;
    return w;
}

// ---- Which four pixels of a tile a lane owns, and where their state sits in a checkpoint.  A lane owns two PAIRS of pixels (elements
// e = 0, 1 and 2, 3): the two pixels of a pair share dy and lie kPair apart in x, and run as packed fp32 (v_pk_fma_f32 issues two FMAs
// in the cycles of 1.2 plain ones on gfx950: profiles/valu_microbench); the second pair lies kPair below the first.
//
// The checkpoint (kCkptFloats: the pixels' state in front of a list position, which the forward writes and the backward reads) holds
// the tile's 256 pixels as [quadrant][T, r, g, b][y << 3 | x inside the 8x8 quadrant]; this is its one definition.  The parts of a
// word take disjoint bits, so a word is also the sum of the words of its parts (a lane's base plus a constant per element and field).
__device__ __forceinline__ int ckpt_word(int quadrant, int field, int qx, int qy) { return (4 * quadrant + field) * kWave + (qy << 3 | qx); }
// The aux checkpoint (kAuxCkptFloats: the depth so far in front of the same list positions) is one plane of the tile's 256 pixels,
// [quadrant][y << 3 | x]: ckpt_word's layout with one field.
__device__ __forceinline__ int aux_word(int quadrant, int qx, int qy) { return quadrant * kWave + (qy << 3 | qx); }
template <int P> struct LanePairs {
    static constexpr int kPair = P;
    __device__ static int ex(int e) { return (e & 1) * kPair; }      // element e's pixel, from the lane's first (element 0)
    __device__ static int ey(int e) { return (e >> 1) * kPair; }
};

// k_render_fwd<QuadrantLanes> ("one wave, one tile", QUADRANT-major): lane l owns the pixel (l & 7, l >> 3) of each of the tile's four 8x8 quadrants
// (element e = quadrant e).  Whether a splat can reach a quadrant at all (quadrant_mask_q: the exact alpha >= 1/255 bound on the 8x8
// pixel rectangle) is then WAVE-UNIFORM: the 4-bit mask travels with the tile list's entry, and the blend loop skips clear quadrants
// with scalar branches.  A 2-3 px splat reaches one or two quadrants of a tile, not four.
struct QuadrantLanes : LanePairs<8> {
    static constexpr bool kLockStep = true;
    int lx, ly;                                          // the lane's pixel inside each quadrant
    __device__ explicit QuadrantLanes(int lane) : lx(lane & 7), ly(lane >> 3) {}
    __device__ int x0(int tx) const { return tx * GSR_TILE + lx; }      // the lane's first pixel (element 0) in the tile (tx, ty)
    __device__ int y0(int ty) const { return ty * GSR_TILE + ly; }
    __device__ int ckpt(int e, int field) const { return ckpt_word(0, 0, lx, ly) + ckpt_word(e, field, 0, 0); }
    __device__ int aux(int e) const { return aux_word(0, lx, ly) + aux_word(e, 0, 0); }
    // wave-uniform 4-bit mask: quadrant k still has a live pixel
    __device__ unsigned live(const FwdPair &A, const FwdPair &B) const
    {
        unsigned m = 0;
        if (__ballot(A.T[0] > 0.f) != 0ull) m |= 1u;
        if (__ballot(A.T[1] > 0.f) != 0ull) m |= 2u;
        if (__ballot(B.T[0] > 0.f) != 0ull) m |= 4u;
        if (__ballot(B.T[1] > 0.f) != 0ull) m |= 8u;
        return m;
    }
};

// k_render_bwd and k_render_fwd<GroupLanes>: the wave is four GROUPS of 16 lanes, one per quadrant; lane l belongs to quadrant g = l >> 4
// and owns the pixels (i & 3 [+ 4], i >> 2 [+ 4]), i = l & 15, of it.  Each group walks its own entries (GroupWalk).
struct GroupLanes : LanePairs<4> {
    static constexpr bool kLockStep = false;
    int grp, lx, ly;                                     // the lane's quadrant, and its first pixel inside it
    __device__ explicit GroupLanes(int lane) : grp(lane >> 4), lx(lane & 3), ly((lane & 15) >> 2) {}
    __device__ int x0(int tx) const { return tx * GSR_TILE + (grp & 1) * 8 + lx; }
    __device__ int y0(int ty) const { return ty * GSR_TILE + (grp >> 1) * 8 + ly; }
    __device__ int ckpt(int e, int field) const { return ckpt_word(grp, 0, lx, ly) + ckpt_word(0, field, ex(e), ey(e)); }
    __device__ int aux(int e) const { return aux_word(grp, lx, ly) + aux_word(0, ex(e), ey(e)); }
    // bit g: group (= quadrant) g still has a live pixel.  One ballot
    __device__ unsigned live(const FwdPair &A, const FwdPair &B) const
    {
        const unsigned long long bal = __ballot(A.T[0] > 0.f || A.T[1] > 0.f || B.T[0] > 0.f || B.T[1] > 0.f);
        return ((bal & 0xFFFFull) ? 1u : 0u) | ((bal & 0xFFFF0000ull) ? 2u : 0u) | ((bal & 0xFFFF00000000ull) ? 4u : 0u) |
               ((bal & 0xFFFF000000000000ull) ? 8u : 0u);
    }
};

// The four groups' walk of a batch: per group, the batch's entries it still has to walk (wave-uniform bit sets: scalar registers).
struct GroupWalk {
    unsigned long long act0, act1, act2, act3;
    // the entries whose quadrant mask has the group's bit, for the groups whose bit is set in `live`
    __device__ GroupWalk(unsigned mymask, unsigned live)
        : act0((live & 1u) ? __ballot((mymask & 1u) != 0u) : 0ull), act1((live & 2u) ? __ballot((mymask & 2u) != 0u) : 0ull),
          act2((live & 4u) ? __ballot((mymask & 4u) != 0u) : 0ull), act3((live & 8u) ? __ballot((mymask & 8u) != 0u) : 0ull) {}
    __device__ bool more() const { return (act0 | act1 | act2 | act3) != 0ull; }
    // each group's next entry (255: it is through with the batch), one byte per group in a scalar register; returns the lane's group's,
    // and in jj the entry to read: an idle group reads the batch's first record, staged for sure, where the slots behind a short
    // batch's end hold whatever LDS held
    __device__ unsigned next(unsigned grp_shift, unsigned &jj)
    {
        const unsigned j0 = act0 ? (unsigned)__ffsll((long long)act0) - 1u : 255u, j1 = act1 ? (unsigned)__ffsll((long long)act1) - 1u : 255u,
                       j2 = act2 ? (unsigned)__ffsll((long long)act2) - 1u : 255u, j3 = act3 ? (unsigned)__ffsll((long long)act3) - 1u : 255u;
        act0 &= act0 - 1ull; act1 &= act1 - 1ull; act2 &= act2 - 1ull; act3 &= act3 - 1ull;      // (0 & anything = 0)
        const unsigned j = __builtin_amdgcn_ubfe(j0 | j1 << 8 | j2 << 16 | j3 << 24, grp_shift, 8u);
        jj = j < (unsigned)kWave ? j : 0u;
        return j;
    }
    __device__ void keep(unsigned live)      // groups whose quadrant is done stop
    {
        if (!(live & 1u)) act0 = 0ull;
        if (!(live & 2u)) act1 = 0ull;
        if (!(live & 4u)) act2 = 0ull;
        if (!(live & 8u)) act3 = 0ull;
    }
};

#if defined(GSR_BWD_TRACE) || defined(GSR_FWD_TRACE)
// debug builds only (tools/bwd_trace.sh): per block {start, end (100 MHz clock), HW_ID, XCC_ID} of the last launch of the
// traced kernel
__device__ unsigned long long g_bwd_trace[4 * 65536];
extern "C" int gsr_debug_bwd_trace(unsigned long long *host_out, int n_blocks)
{
    return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_bwd_trace), sizeof(unsigned long long) * 4 * (size_t)n_blocks);
}
struct TraceEnd {
    unsigned long long t0; int b;
    __device__ ~TraceEnd() {
        if (threadIdx.x == 0 && b < 65536) {
            g_bwd_trace[4 * b] = t0; g_bwd_trace[4 * b + 1] = wall_clock64();
            g_bwd_trace[4 * b + 2] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);
            g_bwd_trace[4 * b + 3] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 20);
        }
    }
};
#endif

// the end of a (tile, chunk)'s blend: the tile's open flag, how deep the backward will walk, and the backward's work units
__device__ __forceinline__ void fwd_tile_epilogue(int t, int tile, int c, int lane, bool closing, bool stuck, int walked, uint32_t *__restrict__ open,
                                                  uint32_t *__restrict__ tile_walk_c, const UnitLists &units, uint32_t *__restrict__ unit_count)
{
    if (lane == 0) {
        open[tile] = closing ? 0u : (stuck ? 2u : 1u);
        tile_walk_c[tile] = (uint32_t)walked;
    }
    // the blend backward's work units of this (tile, chunk): one per kSeg walked entries, appended to the lists of the tile's shard
    // (full segments; the last, partial one by its length class)
    const uint32_t n_full = (uint32_t)walked / kSeg, rest = (uint32_t)walked - n_full * kSeg;
    if (walked > 0) {
        const int shard = t & (kUnitShards - 1);
        const uint32_t head = (uint32_t)tile | ((uint32_t)c << kUnitTileBits);
        const int cls = unit_class(rest);
        uint32_t at_full = 0, at_part = 0;
        if (lane == 0) {
            if (n_full) at_full = atomicAdd(&unit_count[shard * kUnitClasses], n_full);
            if (rest) at_part = atomicAdd(&unit_count[shard * kUnitClasses + cls], 1u);
        }
        at_full = (uint32_t)__builtin_amdgcn_readfirstlane((int)at_full);
        uint2 *full = units.units + units.list_begin(shard, 0);
        for (uint32_t sgm = (uint32_t)lane; sgm < n_full; sgm += kWave)
            if (at_full + sgm < units.cap_full) full[at_full + sgm] = make_uint2(head, sgm);
        if (lane == 0 && rest && at_part < units.cap_part) units.units[units.list_begin(shard, cls) + at_part] = make_uint2(head, n_full);
    }
}

// One blend forward of a (tile, chunk) for both pixel mappings; only the batch walk differs.  Lock step (QuadrantLanes): the wave walks
// the batch's splats that reach a live quadrant together.  Groups (GroupLanes): each group walks the entries that reach ITS quadrant -
// the mapping and the walk of k_render_bwd - for chunks of SMALL splats (launch_render_fwd's `groups`: fewer than 4.5 tiles per
// Gaussian).  A splat that reaches one or two quadrants costs the lock-step walk a pass of the whole wave; with groups up to four
// different splats share a pass.  Where splats reach most quadrants lock step is faster (wave-uniform records, whole pairs skipped):
// cfg3n 258 -> 230 us with groups, but cfg3 105 -> 116, cfg5n 696 -> 706 - hence two kernels.  The checkpoints and every per-pixel
// array are the same either way, and so are the bits.
//
// kAux (gsr_forward_render_aux): the same blend also renders the expected depth, one more packed accumulator per pair,
// Z = fma(z, w, Z) with the record's view depth z - the colour channels' own operation, so depth is bit for bit a colour channel fed
// z - and alpha = 1 - |T| when the tile stores its pixels.  Between chunks Z lives in the depth map (as the unfinished colour lives in
// out_color); in front of every checkpoint it goes into the aux checkpoint plane of the same slot (AuxFwdK).
struct AuxFwdK {
    static constexpr int kPlanes = 1;  // planes of kAuxCkptFloats per aux checkpoint
    static constexpr bool kMedian = false;      // MedFwdK: the blend also selects the median depth
    float *depth, *alpha;              // [H, W]
    float *ckpt;                       // [R / kSeg + 2][kAuxCkptFloats]: Z in front of the checkpoint of the same slot (BinningWS::ckpt)
    float *ckpt_start_c;               // [Tn][kAuxCkptFloats]: Z when this chunk (>= 1) starts on a tile (ImageWS::ckpt_start)
};
// kExt (gsr_forward_render_extra; the aux kernels handed an ExtFwdK): the same blend also renders three more linear channels from a
// per-Gaussian table, staged by stage_batch into a second LDS array beside sh_rec: three more packed accumulators per pair,
// X = fma(e, w, X) - again the colour channels' own operation on fwd_pair's w, so each is bit for bit a colour channel fed e over a zero
// background.  Between chunks they live in the map [3, H, W]; in front of every checkpoint they go into planes 1..3 of the aux
// checkpoint, which has kPlanes = 4 planes in these instantiations (plane 0: Z).
struct ExtFwdK : AuxFwdK {
    static constexpr int kPlanes = kExtCkptPlanes;
    const float4 *table;               // [P] (e0, e1, e2, unused)
    float *map;                        // [3, H, W]
};
// kMed (gsr_forward_render_median; the aux kernels handed a MedFwdK): the same blend also selects the pixel's median depth - the view
// depth of the last composited splat whose front transmittance is above one half.  Per pair: T in front of the
// splat is taken before fwd_pair, w behind it, and M = (T > 0.5 && w > 0) ? z : M, likewise the entry's last_enc encoding - two compares
// and two selects per pixel, no arithmetic, so every other value of the frame is the aux frame's.  A done pixel has T < 0 and a pixel whose T
// has fallen to one half or below never passes the test again, so a later chunk cannot move it.  Between chunks the two values live in
// their maps, as Z lives in the depth map; the backward does not re-derive the median, so no checkpoint plane holds it.
struct MedFwdK : AuxFwdK {
    static constexpr bool kMedian = true;
    float *median;                     // [H, W]
    int32_t *median_enc;               // [H, W] the median's list entry, encoded as last_enc (0: none)
};
// kStats (gsr_forward_render_contrib; lock step only): the same blend also takes, per blended splat, three totals over the wave's 256
// pixels of the weights w that fwd_pair returns - n = the pixels with w > 0 (ballots: scalar), s = their sum (the lane's four in a
// fixed order, then wave_sum's fixed tree), m = their maximum (wave_max).  The splat is wave-uniform, so each is a whole-wave
// reduction; lane j keeps the totals of entry j of the staged batch, and behind the batch the lanes whose n > 0 add them to the
// caller's per-Gaussian accumulators: three wave instructions per batch of 64 entries, every one an INTEGER add or max (ContribK), so
// the accumulators do not depend on the order in which tiles, chunks or launches arrive.  Everything else is written as by the plain
// kernel: a statistics frame is a complete frame.
struct ContribK {
    unsigned long long *count;         // [P] += n
    unsigned long long *sum_q32;       // [P] += (uint64)(s 2^32): s < 256, the product is below 2^40 and exact but for what lies under 2^-32
    uint32_t *max_bits;                // [P] = max(., bits of m): w >= 0, so the bit patterns order like the values
};
// kErr (gsr_forward_render_contrib_error; with kStats): a fourth total per blended splat, e = the sum over the wave's 256 pixels of
// w E(pixel), with E the caller's per-pixel error map.  Each lane loads the error of its four pixels once per launch (load_px's
// addressing; 0 outside the image; clamped to [0, 1] on load, which also reads a NaN as 0) and keeps them in registers for the walk.
// The lane's four products are added in the association of `s` (err_dot4), so that E = 1 gives the bits of `s`; lane j
// keeps e beside n, s, m and the batch's fourth atomic is a 64-bit integer add in units of 2^-32 (E <= 1: the bound of sum_q32).
struct ErrK {
    const float *pixel_error;          // [H, W]
    unsigned long long *frame_q32;     // [P] += (uint64)(e 2^32): this frame's total, folded and cleared by k_contrib_error_fold
};
// ((a0 e0 + a1 e1) + a2 e2) + a3 e3 with every product and sum rounded on its own: the file is built with -ffp-contract=fast, which
// would fuse three of the products into the adds.  The association is what makes E = 1 reproduce `s` (a product with 1 is exact, fused
// or not); the pragma only fixes which roundings a general E sees, so that they do not move with the compiler's choice.
__device__ __forceinline__ float err_dot4(float a0, float a1, float a2, float a3, float e0, float e1, float e2, float e3)
{
#pragma clang fp contract(off)
    return ((a0 * e0 + a1 * e1) + a2 * e2) + a3 * e3;
}
template <class Map, bool kAux, bool kStats = false, bool kErr = false, class AX = AuxFwdK>
__device__ __forceinline__ void render_fwd(FrameK f, int c, int finalize_all, const uint2 *__restrict__ ranges_c, uint32_t *__restrict__ open,
                                           const uint32_t *__restrict__ sorted_gid, const float4 *__restrict__ records,
                                           const float *__restrict__ bg, float *__restrict__ out_color, float *__restrict__ T_state,
                                           int32_t *__restrict__ last_enc, uint32_t *__restrict__ tile_walk_c, float *__restrict__ ckpt,
                                           float *__restrict__ ckpt_start_c, const UnitLists &units, uint32_t *__restrict__ unit_count,
                                           const AX &ax, const ContribK &cs = ContribK{}, const ErrK &er = ErrK{})
{
    constexpr bool kExt = AX::kPlanes > 1;
    constexpr bool kMed = AX::kMedian;
    static_assert(!kMed || (kAux && !kExt), "the median rides on the aux kernels; ext x median is not built");
    constexpr int kAuxStride = AX::kPlanes * kAuxCkptFloats;      // floats per aux checkpoint
    static_assert(!kExt || kAux, "the extra channels ride on the aux kernels");
    static_assert(!kStats || (Map::kLockStep && !kAux), "the statistics are built for the lock-step colour kernel");
    static_assert(!kErr || kStats, "the error-weighted total rides on the statistics");
    __shared__ float4 sh_rec[kWave * 3];
    float4 *sh_ext = nullptr;                              // kExt: the batch's rows of the extra table
    if constexpr (kExt) {
        __shared__ float4 sh_ext_rows[kWave];
        sh_ext = sh_ext_rows;
    }
#ifdef GSR_FWD_TRACE
    TraceEnd trace_end{(unsigned long long)wall_clock64(), (int)blockIdx.x};
#endif
    // tile = block: consecutive tiles run on different XCDs (block b -> XCD b % 8), which balances them; contiguous bands
    // per XCD (round 1) finished up to 20 % apart at cfg3 and bought nothing measurable in L2 hits
    const int t = (int)blockIdx.x;
    const int tx = t % f.Gx, ty = f.ty0 + t / f.Gx;
    const int tile = ty * f.Gx + tx;
    if (open[tile] == 0u) return;                       // closed by an earlier chunk: pixels are final
    const uint2 rng = ranges_c[tile];
    const int lane = threadIdx.x;
    const Map map(lane);
    const int px0 = map.x0(tx), py0 = map.y0(ty);
    const float fy0 = (float)py0, fy1 = fy0 + (float)Map::kPair;
    const v2f fxv = {(float)px0, (float)(px0 + Map::kPair)};
    const size_t N = (size_t)f.W * f.H;

    FwdPair P0, P1;
    auto load_px = [&](int e, float &t_, float &r_, float &g_, float &b_, int &last) {
        const int px = px0 + map.ex(e), py = py0 + map.ey(e);
        const bool inside = px < f.W && py < f.H;
        t_ = inside ? 1.f : -1.f; r_ = g_ = b_ = 0.f; last = 0;
        if (c > 0 && inside) {
            const size_t pix = (size_t)py * f.W + px;
            t_ = T_state[pix];
            r_ = out_color[pix]; g_ = out_color[N + pix]; b_ = out_color[2 * N + pix];
            last = last_enc[pix];
        }
    };
    {
        float t0, r0, g0, b0, t1, r1, g1, b1;
        load_px(0, t0, r0, g0, b0, P0.last0); load_px(1, t1, r1, g1, b1, P0.last1);
        P0.T = v2f{t0, t1}; P0.Cr = v2f{r0, r1}; P0.Cg = v2f{g0, g1}; P0.Cb = v2f{b0, b1};
        load_px(2, t0, r0, g0, b0, P1.last0); load_px(3, t1, r1, g1, b1, P1.last1);
        P1.T = v2f{t0, t1}; P1.Cr = v2f{r0, r1}; P1.Cg = v2f{g0, g1}; P1.Cb = v2f{b0, b1};
    }
    float e00 = 0.f, e01 = 0.f, e10 = 0.f, e11 = 0.f;      // kErr: the error of the lane's four pixels (P0's two, P1's two)
    if constexpr (kErr) {
        auto load_e = [&](int e) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            const float x = (px < f.W && py < f.H) ? er.pixel_error[(size_t)py * f.W + px] : 0.f;
            return fminf(fmaxf(x, 0.f), 1.f);               // (fmaxf(NaN, 0) = 0)
        };
        e00 = load_e(0); e01 = load_e(1); e10 = load_e(2); e11 = load_e(3);
    }
    v2f Z0 = {0.f, 0.f}, Z1 = {0.f, 0.f};                  // kAux: the depth so far of the two pairs
    if constexpr (kAux) {
        auto load_z = [&](int e) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            return (c > 0 && px < f.W && py < f.H) ? ax.depth[(size_t)py * f.W + px] : 0.f;
        };
        Z0 = v2f{load_z(0), load_z(1)}; Z1 = v2f{load_z(2), load_z(3)};
    }
    v2f M0 = {0.f, 0.f}, M1 = {0.f, 0.f};                  // kMed: the median depth so far of the two pairs, and its list entry
    int me00 = 0, me01 = 0, me10 = 0, me11 = 0;
    if constexpr (kMed) {
        auto load_m = [&](int e, float &m_, int &enc) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            m_ = 0.f; enc = 0;
            if (c > 0 && px < f.W && py < f.H) { m_ = ax.median[(size_t)py * f.W + px]; enc = ax.median_enc[(size_t)py * f.W + px]; }
        };
        float m0, m1;
        load_m(0, m0, me00); load_m(1, m1, me01); M0 = v2f{m0, m1};
        load_m(2, m0, me10); load_m(3, m1, me11); M1 = v2f{m0, m1};
    }
    v2f X0[3] = {}, X1[3] = {};                            // kExt: the three extra channels so far of the two pairs
    if constexpr (kExt) {
        auto load_x = [&](int e, int k) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            return (c > 0 && px < f.W && py < f.H) ? ax.map[(size_t)k * N + (size_t)py * f.W + px] : 0.f;
        };
#pragma unroll
        for (int k = 0; k < 3; ++k) { X0[k] = v2f{load_x(0, k), load_x(1, k)}; X1[k] = v2f{load_x(2, k), load_x(3, k)}; }
    }

    const int n_total = (int)(rng.y - rng.x);
    const int enc_base = (c + 1) << kLastShift;
    // The blend backward walks this list front to back in independent segments of kSeg entries (gsr_internal.h): it starts a
    // segment from the pixels' state (live transmittance, colour so far) in front of the segment's first entry, kept here.
    auto checkpoint = [&](float *dst, float *zdst) {
        auto put = [&](int e, const FwdPair &P, int h) {
            dst[map.ckpt(e, 0)] = P.T[h]; dst[map.ckpt(e, 1)] = P.Cr[h]; dst[map.ckpt(e, 2)] = P.Cg[h]; dst[map.ckpt(e, 3)] = P.Cb[h];
        };
        put(0, P0, 0); put(1, P0, 1); put(2, P1, 0); put(3, P1, 1);
        if constexpr (kAux) {
            zdst[map.aux(0)] = Z0[0]; zdst[map.aux(1)] = Z0[1]; zdst[map.aux(2)] = Z1[0]; zdst[map.aux(3)] = Z1[1];
        }
        if constexpr (kExt) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float *xdst = zdst + (k + 1) * kAuxCkptFloats;
                xdst[map.aux(0)] = X0[k][0]; xdst[map.aux(1)] = X0[k][1]; xdst[map.aux(2)] = X1[k][0]; xdst[map.aux(3)] = X1[k][1];
            }
        }
    };
    v2f sw0 = {0.f, 0.f}, sw1 = {0.f, 0.f};              // kStats: the weights of the splat blended last (0 for a pair it skipped)
    // blend entry j of the batch into the pairs m names (bits 0-1: P0, 2-3: P1; active: the lane's group has an entry in this pass)
    auto blend = [&](int base, unsigned j, bool active, unsigned m) {
        if constexpr (kStats) sw0 = sw1 = v2f{0.f, 0.f};
        const float4 a = sh_rec[3u * j], b = sh_rec[3u * j + 1u];
        const float cbl = sh_rec[3u * j + 2u].x;
        const int contributor = enc_base | (int)((unsigned)base + j + 1u);
        const v2f dx = a.x - fxv;                                 // one subtraction from the pixel's x (all three blend kernels)
        const LpTerms lt = lp_terms(a.z, a.w, b.y, dx);
        if (m & 3u) {
            const float dy = a.y - fy0;
            v2f Tf = {0.f, 0.f};                                  // kMed: T in front of the splat
            if constexpr (kMed) Tf = P0.T;
            const v2f w = fwd_pair(active, lp_at(lt, b.x, dy), b.y, b.z, b.w, cbl, contributor, P0);
            if constexpr (kMed) {
                const float z = sh_rec[3u * j + 2u].y;
                const bool s0 = Tf[0] > 0.5f && w[0] > 0.f, s1 = Tf[1] > 0.5f && w[1] > 0.f;
                M0 = v2f{s0 ? z : M0[0], s1 ? z : M0[1]};
                me00 = s0 ? contributor : me00; me01 = s1 ? contributor : me01;
            }
            if constexpr (kAux) { const float z = sh_rec[3u * j + 2u].y; Z0 = __builtin_elementwise_fma(v2f{z, z}, w, Z0); }
            if constexpr (kExt) {
                const float4 x = sh_ext[j];
                X0[0] = __builtin_elementwise_fma(v2f{x.x, x.x}, w, X0[0]);
                X0[1] = __builtin_elementwise_fma(v2f{x.y, x.y}, w, X0[1]);
                X0[2] = __builtin_elementwise_fma(v2f{x.z, x.z}, w, X0[2]);
            }
            if constexpr (kStats) sw0 = w;
        }
        if (m & 12u) {
            const float dy = a.y - fy1;
            v2f Tf = {0.f, 0.f};
            if constexpr (kMed) Tf = P1.T;
            const v2f w = fwd_pair(active, lp_at(lt, b.x, dy), b.y, b.z, b.w, cbl, contributor, P1);
            if constexpr (kMed) {
                const float z = sh_rec[3u * j + 2u].y;
                const bool s0 = Tf[0] > 0.5f && w[0] > 0.f, s1 = Tf[1] > 0.5f && w[1] > 0.f;
                M1 = v2f{s0 ? z : M1[0], s1 ? z : M1[1]};
                me10 = s0 ? contributor : me10; me11 = s1 ? contributor : me11;
            }
            if constexpr (kAux) { const float z = sh_rec[3u * j + 2u].y; Z1 = __builtin_elementwise_fma(v2f{z, z}, w, Z1); }
            if constexpr (kExt) {
                const float4 x = sh_ext[j];
                X1[0] = __builtin_elementwise_fma(v2f{x.x, x.x}, w, X1[0]);
                X1[1] = __builtin_elementwise_fma(v2f{x.y, x.y}, w, X1[1]);
                X1[2] = __builtin_elementwise_fma(v2f{x.z, x.z}, w, X1[2]);
            }
            if constexpr (kStats) sw1 = w;
        }
    };
    if (c > 0 && n_total > 0)
        checkpoint(ckpt_start_c + (size_t)tile * kCkptFloats, kAux ? ax.ckpt_start_c + (size_t)tile * kAuxStride : nullptr);
    for (int base = 0; base < n_total; base += kWave) {
        unsigned live = map.live(P0, P1);
        if (live == 0u) break;
        if (base > 0 && base % kSeg == 0) {
            const size_t slot = (rng.x + (uint32_t)base) / kSeg;
            checkpoint(ckpt + slot * kCkptFloats, kAux ? ax.ckpt + slot * kAuxStride : nullptr);
        }
        const int n = min(kWave, n_total - base);
        __syncthreads();
        uint32_t entry = 0;                                // kStats: the lane's list entry, and its totals over the wave's pixels
        uint32_t st_n = 0;
        float st_s = 0.f, st_m = 0.f, st_e = 0.f;
        unsigned mymask;
        if constexpr (kExt) mymask = stage_batch_ext(sh_rec, sh_ext, lane, n, sorted_gid, rng.x + base, records, ax.table);
        else mymask = stage_batch(sh_rec, lane, n, sorted_gid, rng.x + base, records, kStats ? &entry : nullptr);
        __syncthreads();
        // every 8 blended splats (passes, with groups) the live mask is refreshed: quadrants (and tiles) that saturate mid-batch stop there
        int since_refresh = 0;
        if constexpr (Map::kLockStep) {
            // splats of the batch that can reach a live quadrant, front to back (bit j = splat j): the others cost nothing
            unsigned long long act = __ballot((mymask & live) != 0u);
            while (act != 0ull) {
                const int j = __ffsll((long long)act) - 1;
                act &= act - 1ull;
                blend(base, (unsigned)j, true, (unsigned)__builtin_amdgcn_readlane((int)mymask, j) & live);
                if constexpr (kStats) {
                    const uint32_t cnt = (uint32_t)(__popcll(__ballot(sw0[0] > 0.f)) + __popcll(__ballot(sw0[1] > 0.f)) +
                                                    __popcll(__ballot(sw1[0] > 0.f)) + __popcll(__ballot(sw1[1] > 0.f)));
                    if (cnt != 0u) {                       // (wave-uniform: a splat no pixel composited costs the ballots only)
                        const float sum = wave_sum(((sw0[0] + sw0[1]) + sw1[0]) + sw1[1]);
                        const float top = wave_max(fmaxf(fmaxf(sw0[0], sw0[1]), fmaxf(sw1[0], sw1[1])));
                        if (lane == j) { st_n = cnt; st_s = sum; st_m = top; }      // an entry is blended at most once
                        if constexpr (kErr) {
                            const float err = wave_sum(err_dot4(sw0[0], sw0[1], sw1[0], sw1[1], e00, e01, e10, e11));
                            if (lane == j) st_e = err;
                        }
                    }
                }
                if (++since_refresh == 8) {
                    since_refresh = 0;
                    live = map.live(P0, P1);
                    act &= __ballot((mymask & live) != 0u);
                }
            }
        } else {
            // each group walks the batch's entries that reach ITS quadrant, front to back, while the quadrant holds a live pixel
            GroupWalk walk(mymask, live);
            while (walk.more()) {
                unsigned jj;
                const unsigned j = walk.next(8u * (unsigned)map.grp, jj);
                blend(base, jj, j < (unsigned)kWave, 15u);
                if (++since_refresh == 8) {
                    since_refresh = 0;
                    live = map.live(P0, P1);
                    walk.keep(live);
                }
            }
        }
        if constexpr (kStats) {
            if (st_n != 0u) {
                const uint32_t gid = entry & kGidMask;
                atomicAdd(cs.count + gid, (unsigned long long)st_n);
                atomicAdd(cs.sum_q32 + gid, (unsigned long long)(st_s * 4294967296.f));
                atomicMax(cs.max_bits + gid, __float_as_uint(st_m));
                if constexpr (kErr) atomicAdd(er.frame_q32 + gid, (unsigned long long)(st_e * 4294967296.f));
            }
        }
    }
    const bool closing = map.live(P0, P1) == 0u;
    const bool finalize = closing || finalize_all != 0;
    const float bg0 = finalize ? bg[0] : 0.f, bg1 = finalize ? bg[1] : 0.f, bg2 = finalize ? bg[2] : 0.f;
    auto store_px = [&](int e, float t_, float r_, float g_, float b_, int last) {
        const int px = px0 + map.ex(e), py = py0 + map.ey(e);
        if (px < f.W && py < f.H) {
            const size_t pix = (size_t)py * f.W + px;
            const float tf = fabsf(t_);
            out_color[pix] = r_ + tf * bg0;
            out_color[N + pix] = g_ + tf * bg1;
            out_color[2 * N + pix] = b_ + tf * bg2;
            T_state[pix] = t_;
            last_enc[pix] = last;
        }
    };
    store_px(0, P0.T[0], P0.Cr[0], P0.Cg[0], P0.Cb[0], P0.last0);
    store_px(1, P0.T[1], P0.Cr[1], P0.Cg[1], P0.Cb[1], P0.last1);
    store_px(2, P1.T[0], P1.Cr[0], P1.Cg[0], P1.Cb[0], P1.last0);
    store_px(3, P1.T[1], P1.Cr[1], P1.Cg[1], P1.Cb[1], P1.last1);
    if constexpr (kAux) {
        auto store_aux = [&](int e, float t_, float z_) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            if (px < f.W && py < f.H) {
                const size_t pix = (size_t)py * f.W + px;
                ax.depth[pix] = z_;                             // no background term
                ax.alpha[pix] = 1.f - fabsf(t_);
            }
        };
        store_aux(0, P0.T[0], Z0[0]); store_aux(1, P0.T[1], Z0[1]); store_aux(2, P1.T[0], Z1[0]); store_aux(3, P1.T[1], Z1[1]);
    }
    if constexpr (kMed) {
        auto store_m = [&](int e, float m_, int enc) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            if (px < f.W && py < f.H) { ax.median[(size_t)py * f.W + px] = m_; ax.median_enc[(size_t)py * f.W + px] = enc; }
        };
        store_m(0, M0[0], me00); store_m(1, M0[1], me01); store_m(2, M1[0], me10); store_m(3, M1[1], me11);
    }
    if constexpr (kExt) {
        auto store_x = [&](int e, int k, float x_) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            if (px < f.W && py < f.H) ax.map[(size_t)k * N + (size_t)py * f.W + px] = x_;      // no background term
        };
#pragma unroll
        for (int k = 0; k < 3; ++k) { store_x(0, k, X0[k][0]); store_x(1, k, X0[k][1]); store_x(2, k, X1[k][0]); store_x(3, k, X1[k][1]); }
    }
    // 2 = open AND some pixel is still more than half transparent after everything so far: a tile no splat has covered yet
    // (the chunk plan merges the remaining chunks when such tiles exist: the frame is not going to close, gsr_api.hip)
    auto clear_px = [&](int e, float t_) { return px0 + map.ex(e) < f.W && py0 + map.ey(e) < f.H && t_ > 0.5f; };
    const bool stuck = __ballot(clear_px(0, P0.T[0]) || clear_px(1, P0.T[1]) || clear_px(2, P1.T[0]) || clear_px(3, P1.T[1])) != 0ull;
    // what the backward's wave will walk of this chunk's range: up to the tile's deepest contributor (launch order of K7)
    auto depth_here = [&](int last) { return (last >> kLastShift) == c + 1 ? (last & ((1 << kLastShift) - 1)) : 0; };
    const int walked = wave_max_uniform(max(max(depth_here(P0.last0), depth_here(P0.last1)), max(depth_here(P1.last0), depth_here(P1.last1))));
    fwd_tile_epilogue(t, tile, c, lane, closing, stuck, walked, open, tile_walk_c, units, unit_count);
}

// Every variant of the blend forward is an instantiation of this one kernel.  X: the variant's own kernel arguments - AuxFwdK for the aux
// instantiations of both pixel mappings (colour, radii and every array as the plain kernels, plus depth and alpha), ExtFwdK in its
// place for the ext instantiations (every array as the aux kernels, plus the extra map), MedFwdK for the median ones (plus the median maps); ContribK, then
// ErrK, for the statistics instantiations (lock step, whatever the chunk's splats are like: both mappings render the same bits)
template <class Map, bool kAux, bool kStats, bool kErr, int kMinWaves, class... X>
__global__ __launch_bounds__(kWave, kMinWaves) void k_render_fwd(FrameK f, int n_tiles, int c, int finalize_all,
                                                                 const uint2 *__restrict__ ranges_c, uint32_t *__restrict__ open,
                                                                 const uint32_t *__restrict__ sorted_gid,
                                                                 const float4 *__restrict__ records, const float *__restrict__ bg,
                                                                 float *__restrict__ out_color, float *__restrict__ T_state,
                                                                 int32_t *__restrict__ last_enc, uint32_t *__restrict__ tile_walk_c,
                                                                 float *__restrict__ ckpt, float *__restrict__ ckpt_start_c,
                                                                 UnitLists units, uint32_t *__restrict__ unit_count, X... x)
{
    if constexpr (kAux)
        render_fwd<Map, true>(f, c, finalize_all, ranges_c, open, sorted_gid, records, bg, out_color, T_state, last_enc, tile_walk_c, ckpt, ckpt_start_c, units, unit_count, x...);
    else
        render_fwd<Map, false, kStats, kErr>(f, c, finalize_all, ranges_c, open, sorted_gid, records, bg, out_color, T_state, last_enc, tile_walk_c, ckpt, ckpt_start_c, units,
                                             unit_count, AuxFwdK{}, x...);
}

// Behind a frame's last chunk: fold the frame's error totals into the running sum and the running maximum, and clear them for the next
// frame.  One thread per Gaussian; no row is touched by two threads.
__global__ __launch_bounds__(256) void k_contrib_error_fold(long long P, unsigned long long *__restrict__ frame_q32,
                                                            unsigned long long *__restrict__ sum_q32, float *__restrict__ error_max)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= P) return;
    const unsigned long long q = frame_q32[g];
    sum_q32[g] += q;
    error_max[g] = fmaxf(error_max[g], (float)((double)q * 0x1p-32));
    frame_q32[g] = 0ull;
}

int launch_contrib_error_fold(long long P, uint64_t *frame_q32, uint64_t *sum_q32, float *error_max, bool debug, hipStream_t s)
{
    if (P <= 0) return GSR_OK;
    ProfileScope prof("contrib_error_fold", s);
    hipLaunchKernelGGL(k_contrib_error_fold, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, P, (unsigned long long *)frame_q32,
                       (unsigned long long *)sum_q32, error_max);
    GSR_LAUNCH_CHECK("contrib_error_fold", debug, s);
    return GSR_OK;
}

int launch_render_fwd(const FrameK &f, const gsr_camera &cam, int c, bool last_chunk, int sort_result, const GeomWS &gw, const BinningWS &bw,
                      ImageWS &iw, float *out_color, bool debug, hipStream_t s, bool groups, const FwdVariant &v)
{
    const int n_tiles = (f.ty1 - f.ty0) * f.Gx;
    if (n_tiles <= 0) return GSR_OK;
    const size_t Tn = (size_t)f.Gx * f.Gy;
    const auto launch = [&](auto kernel, const char *name, auto... x) -> int {
        ProfileScope prof(name, s);
        hipLaunchKernelGGL(kernel, dim3(n_tiles), dim3(kWave), 0, s, f, n_tiles, c, last_chunk ? 1 : 0, iw.ranges + (size_t)c * Tn, iw.open,
                           bw.gids[1], gw.records, cam.bg, out_color, iw.T_state, iw.last_enc, iw.tile_walk + (size_t)c * Tn, bw.ckpt,
                           c > 0 ? iw.ckpt_start + (size_t)(c - 1) * Tn * kCkptFloats : nullptr, bw.units, iw.unit_count, x...);
        GSR_LAUNCH_CHECK(name, debug, s);
        return GSR_OK;
    };
    if (v.stats) {
        const ContribK cs{(unsigned long long *)v.stats->count, (unsigned long long *)v.stats->weight_sum_q32, v.stats->weight_max_bits};
        if (!v.err) return launch(k_render_fwd<QuadrantLanes, false, true, false, 4, ContribK>, "render_fwd_contrib", cs);
        const ErrK er{v.err->pixel_error, (unsigned long long *)v.err->error_frame_q32};
        return launch(k_render_fwd<QuadrantLanes, false, true, true, 4, ContribK, ErrK>, "render_fwd_contrib_error", cs, er);
    }
    if (v.aux && v.ext) {
        ExtFwdK ex;
        ex.depth = v.aux->depth; ex.alpha = v.aux->alpha; ex.ckpt = v.aux->ckpt;
        ex.ckpt_start_c = c > 0 ? v.aux->ckpt_start + (size_t)(c - 1) * Tn * (kExtCkptPlanes * kAuxCkptFloats) : nullptr;
        ex.table = v.ext->table; ex.map = v.ext->map;
        return launch(groups ? k_render_fwd<GroupLanes, true, false, false, kFwdExtWaves, ExtFwdK> : k_render_fwd<QuadrantLanes, true, false, false, kFwdExtWaves, ExtFwdK>,
                      "render_fwd_ext", ex);
    }
    if (v.aux && v.med) {
        MedFwdK mx;
        mx.depth = v.aux->depth; mx.alpha = v.aux->alpha; mx.ckpt = v.aux->ckpt;
        mx.ckpt_start_c = c > 0 ? v.aux->ckpt_start + (size_t)(c - 1) * Tn * kAuxCkptFloats : nullptr;
        mx.median = v.med->median; mx.median_enc = v.med->median_enc;
        return launch(groups ? k_render_fwd<GroupLanes, true, false, false, 4, MedFwdK> : k_render_fwd<QuadrantLanes, true, false, false, 4, MedFwdK>,
                      "render_fwd_median", mx);
    }
    if (v.aux) {
        const AuxFwdK ax{v.aux->depth, v.aux->alpha, v.aux->ckpt, c > 0 ? v.aux->ckpt_start + (size_t)(c - 1) * Tn * kAuxCkptFloats : nullptr};
        return launch(groups ? k_render_fwd<GroupLanes, true, false, false, 4, AuxFwdK> : k_render_fwd<QuadrantLanes, true, false, false, 4, AuxFwdK>,
                      "render_fwd_aux", ax);
    }
    return launch(groups ? k_render_fwd<GroupLanes, false, false, false, kFwdWaves> : k_render_fwd<QuadrantLanes, false, false, false, kFwdWaves>,
                  "render_fwd");
}

// ------------------------------------------------------------------------------------------- K7
// One launch for the whole frame, one wave per WORK UNIT (tile, chunk, segment of kSeg list entries), FRONT TO BACK.
//
// A.9 walks a pixel's list back to front with the colour behind the current splat as its state.  The same derivative in
// front-to-back form: with w_j = alpha_j T_j (T_j = transmittance in front of splat j), D_i = sum_{j <= i} w_j <c_j, dL/dpix>
// (the prefix of the pixel's colour, dotted with the upstream gradient) and Q = <out_color, dL/dpix> (the FINAL pixel,
// background term T_final bg included),
//     dL/dalpha_i = T_i <c_i, dL/dpix> - (Q - D_i) / (1 - alpha_i)
// since (Q - D_i) is what all splats behind i and the background contribute.  The state per pixel is (T, D): T is
// advanced by the multiplication the forward used (no division by 1 - alpha to recover it), and a walk may start anywhere
// the forward left (T, colour): a checkpoint every kSeg entries, D = <colour so far, dL/dpix>.  So the segments of a tile
// are independent units — 21 k units of <= 128 entries instead of 8 160 tiles of ~400 at cfg3n, where the launch used to end
// with a third of its time draining.
//
// Per pixel and splat, written so that a rejected pixel runs the same arithmetic with alpha = 0 and G = 0: T, D and every
// partial sum then stay exactly unchanged, and only alpha and G need a select.
//
// Algebra: with ga = opacity * G (the alpha before its 0.99 clamp; 0 where the pixel rejects the splat) every term of A.9
// that carries G * dL/dG = G * opacity * dL/dalpha is dL/dalpha * ga, so neither the opacity nor its reciprocal is needed
// per pixel (dL/dopacity = sum(G dL/dalpha) = sum(ga dL/dalpha) / opacity: one division per splat, after the reduction), and
// the conic enters through the pre-scaled record fields directly: cA = -2 ln2 qA, cB = -ln2 qB, cC = -2 ln2 qC, so
// -(tx cA + ty cB) = ln2 (2 qA tx + qB ty): the factor ln2 goes into the row store.
//
// The aux backward (k_render_bwd<true>) adds the depth and alpha maps' upstream gradients g_z, g_a.  Depth is one more linear channel
// (colour z_i, no background): <c_i, dL/dpix> gains z_i g_z, E's starting value g_z (depth_final - Z at the checkpoint), and
// dL/dz_i = sum w_i g_z is a tenth per-splat sum.  alpha = 1 - T_final adds g_a T_final / (1 - alpha_i) to dL/dalpha_i: a constant
// per pixel (GA = g_a T_final) times the 1 / (1 - alpha) the colour term already has, one FMA - not through E, where it would be a
// difference of near-equal numbers once T is small.
struct BwdSplat {            // per-splat values (uniform over a 16-lane group)
    float lop, cr, cg, cb;
    float z;                           // aux: the view depth
};
struct BwdPair {             // state of a lane's pair of pixels (4 apart in x, the same row)
    v2f T, E, dpr, dpg, dpb;           // transmittance in front of the current splat; E = Q - D: what everything behind the current
                                       // splat (and the background) still adds to <pixel, dL/dpix>; dL/dpix
    int limit0, limit1;                // contributors of the current chunk each pixel takes part in
};
struct BwdPairAux {          // aux: the same pair's dL/ddepth and dL/dalpha T_final
    v2f dpz, GA;
};
struct BwdExt {              // ext: the splat's extra triple, and a pair's dL/dextra
    float e0, e1, e2;
};
struct BwdPairExt {
    v2f dpe0, dpe1, dpe2;
};
struct BwdAccExt { v2f S10, S11, S12; };      // ext: the lane's sums of w dL/dextra
struct BwdPairMed {          // median: the same pair's dL/dmedian, and each pixel's median as a position + 1 in this unit's chunk (0: none here)
    v2f gm;
    int mpos0, mpos1;
};
// The median's share of the tenth sum: g_m where this entry is the pixel's median, and -0.0 - the one value whose addition changes no
// float, -0.0 and +0.0 included - elsewhere.  An add of its own, never contracted into the product in front of it: with a zero (or
// NULL) dL/dmedian the sum keeps the aux backward's roundings, and at most a zero's sign differs (which the row's first add absorbs).
__device__ __forceinline__ v2f add_median_share(v2f s9, int mabs, const BwdPairMed &PM)
{
#pragma clang fp contract(off)
    return s9 + v2f{mabs == PM.mpos0 ? PM.gm[0] : -0.f, mabs == PM.mpos1 ? PM.gm[1] : -0.f};
}
// the lane's partial sums of one splat, per pair element: X = sum tA dx, Y = sum tA dy (dL/dmean2D = ln2 (2 qA X + qB Y, 2 qC Y + qB X):
// formed once per splat by the lane that stores the row), S2..S4 the conic's, S5 the opacity's, S6..S8 the colour's, S9 (aux) the depth's
struct BwdAcc { v2f X, Y, S2, S3, S4, S5, S6, S7, S8; };
// abs (k_render_bwd<false, true>): the same expression PER PIXEL, u = (2 qA tx + qB ty, 2 qC ty + qB tx), and the lane's sums of |u|:
// what the signed sums lose when a splat's pixels pull in opposite directions.  A rejected pixel has tA = 0 and adds exactly 0.
struct BwdAbsQ { float qA2, qB, qC2; };        // 2 qA, qB, 2 qC of the staged record
struct BwdAbs { v2f AX, AY; };
__device__ __forceinline__ float add_halves(v2f v)
{
    float r;
    asm("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(v[0]), "v"(v[1]));
    return r;
}

// kMed (with kAux): mabs = the entry's position + 1 in the chunk's list (-1 for an idle group's pass), PM the pair's median
template <bool INIT, bool kAux = false, bool kAbs = false, bool kExt = false, bool kMed = false>         // INIT: the splat's first pair, the sums start here (A comes in undefined)
__device__ __forceinline__ void bwd_pair(const BwdSplat sp, v2f lp, v2f dx, float dy, int pos, BwdPair &P, BwdAcc &A,
                                         const BwdPairAux &PA = BwdPairAux{}, v2f *S9 = nullptr, const BwdAbsQ &Q = BwdAbsQ{},
                                         BwdAbs *AB = nullptr, const BwdExt *se = nullptr, const BwdPairExt *PE = nullptr,
                                         BwdAccExt *AE = nullptr, int mabs = -1, const BwdPairMed *PM = nullptr)
{
    const bool valid0 = (pos < P.limit0) && !(lp[0] > sp.lop) && !(lp[0] < kLog2AlphaMin);      // power > 0 <=> lp > lop
    const bool valid1 = (pos < P.limit1) && !(lp[1] > sp.lop) && !(lp[1] < kLog2AlphaMin);
    // a rejected pixel gets lp = -inf: ga = opacity * G and alpha come out 0 by themselves
    const v2f ga = {__builtin_amdgcn_exp2f(valid0 ? lp[0] : -INFINITY), __builtin_amdgcn_exp2f(valid1 ? lp[1] : -INFINITY)};
    const v2f ae = {fminf((float)GSR_ALPHA_MAX, ga[0]), fminf((float)GSR_ALPHA_MAX, ga[1])};
    const v2f one_m = 1.f - ae;
    const v2f inv1ma = {fast_rcp(one_m[0]), fast_rcp(one_m[1])};
    v2f cdp = sp.cr * P.dpr + sp.cg * P.dpg + sp.cb * P.dpb;            // <c_i, dL/dpix>
    if constexpr (kAux) cdp = __builtin_elementwise_fma(v2f{sp.z, sp.z}, PA.dpz, cdp);      // + z_i dL/ddepth
    if constexpr (kExt) {                                                                   // + <e_i, dL/dextra>
        cdp = __builtin_elementwise_fma(v2f{se->e0, se->e0}, PE->dpe0, cdp);
        cdp = __builtin_elementwise_fma(v2f{se->e1, se->e1}, PE->dpe1, cdp);
        cdp = __builtin_elementwise_fma(v2f{se->e2, se->e2}, PE->dpe2, cdp);
    }
    const v2f w = ae * P.T;                                              // d colour / d rgb
    P.E -= w * cdp;                                                      // this splat's own share leaves the remainder
    v2f dL_dalpha = P.T * cdp - P.E * inv1ma;
    if constexpr (kAux) dL_dalpha = __builtin_elementwise_fma(PA.GA, inv1ma, dL_dalpha);      // + dL/dalpha T_final / (1 - alpha_i)
    P.T = P.T * one_m;                                                   // exactly the forward's update
    const v2f tA = dL_dalpha * ga;
    const v2f tx = tA * dx, ty = tA * dy;
    if constexpr (INIT) {
        A.X = tx; A.Y = ty;
        A.S2 = tx * dx;
        A.S3 = tx * dy;
        A.S4 = ty * dy;
        A.S5 = tA;
        A.S6 = w * P.dpr; A.S7 = w * P.dpg; A.S8 = w * P.dpb;
        if constexpr (kAux) *S9 = w * PA.dpz;
        if constexpr (kExt) { AE->S10 = w * PE->dpe0; AE->S11 = w * PE->dpe1; AE->S12 = w * PE->dpe2; }
        if constexpr (kAbs) {
            AB->AX = __builtin_elementwise_abs(Q.qA2 * tx + Q.qB * ty);
            AB->AY = __builtin_elementwise_abs(Q.qC2 * ty + Q.qB * tx);
        }
    } else {
        A.X += tx; A.Y += ty;
        A.S2 += tx * dx;
        A.S3 += tx * dy;
        A.S4 += ty * dy;
        A.S5 += tA;
        A.S6 += w * P.dpr; A.S7 += w * P.dpg; A.S8 += w * P.dpb;
        if constexpr (kAux) *S9 += w * PA.dpz;
        if constexpr (kExt) { AE->S10 += w * PE->dpe0; AE->S11 += w * PE->dpe1; AE->S12 += w * PE->dpe2; }
        if constexpr (kAbs) {
            AB->AX += __builtin_elementwise_abs(Q.qA2 * tx + Q.qB * ty);
            AB->AY += __builtin_elementwise_abs(Q.qC2 * ty + Q.qB * tx);
        }
    }
    if constexpr (kMed) *S9 = add_median_share(*S9, mabs, *PM);
}

// The kernel: one wave per work unit, front to back from the forward's checkpoint, with the wave split into four GROUPS of 16 lanes,
// one per 8x8 quadrant of the tile (GroupLanes).  A small splat reaches one or two quadrants; walked in lock step the whole wave spends
// a pass (and a wave-wide reduction) on it.  Here each group walks (GroupWalk)
// only the batch's entries whose mask has ITS bit: in one pass the wave works on up to four different splats, and one transposing
// butterfly over the rows of 16 lanes (row_sum9_transpose) reduces all four.  The order inside a quadrant is the list's, which is
// all the blend needs.  A group's totals are added to the entry's nine sums in LDS; when the batch is through, lane j forms entry
// j's gradient row and stores it whole (48 B) - rows are written for every entry some group attempted (row_valid).
// A batch ends when its slowest group does (measured imbalance over a frame: 1.01 .. 1.14, tools/quad_stats.py).
// kAux (k_render_bwd<true>): a tenth sum per entry (dL/dz, row slot 9); the LDS stride goes to 11 words, odd, still conflict-free.
// kAbs (k_render_bwd<false, true>): eleven sums per entry, the last two the per-pixel absolute sums (BwdAbs) -> row slots 10, 11 with
// the W/2, H/2 of slots 0, 1; stride 11.  Every other value is computed exactly as in k_render_bwd<false>.
// kExt (k_render_bwd<true, false, kBwdExtWaves, ExtBwdK>; gsr_backward_render_extra): the aux backward plus the three extra channels
// of an ext frame, each one more linear channel like the depth: <c_i, dL/dpix> gains <e_i, g_e>, E's starting value
// <extra_final - extra at the checkpoint, g_e> (planes 1..3 of the four-plane aux checkpoint), and the sums of w g_e are three more
// per-entry sums - 13 with an LDS stride of 13 words, odd, conflict-free - reduced over the rows by row_sum3_rows and stored to a
// row plane of their own ([R] float4, by slot): the 48-B rows keep their layout.
struct AuxBwdK {
    const float *depth;                // [H, W] the forward's depth map (final)
    const float *dL_ddepth, *dL_dalpha;      // [H, W] each, NULL = zero
    const float *ckpt, *ckpt_start;    // the aux checkpoints (AuxWS)
};
// kMed (k_render_bwd<true, false, kBwdWaves, MedBwdK>; gsr_backward_render_median): the aux backward of a median frame.  The selection
// is piecewise constant, so the median map's upstream gradient g_m goes to dL/dz of the pixel's median splat and nowhere else: per pixel
// g_m and the median's position in this unit's chunk (decoded from median_enc as `limit` is from last_enc; 0 when it lies in another
// chunk), and in bwd_pair S9 += (position == the pixel's ? g_m : 0) behind the aux backward's own add.  Every other value is the aux
// backward's; the sum leaves in row slot 9 and the aux row reduction and depth chain follow unchanged.
struct MedBwdK {
    const int32_t *median_enc;         // [H, W] the forward's
    const float *dL_dmedian;           // [H, W], NULL = zero
};
struct ExtBwdK {
    const float4 *table;               // [P] (e0, e1, e2, unused)
    const float *map;                  // [3, H, W] the forward's extra map (final)
    const float *dL_dmap;              // [3, H, W], NULL = zero
    float4 *rows;                      // [instances emitted] by slot
};
constexpr int kBwdExtWaves = 3;        // minimum waves per SIMD of the ext instantiation: at kBwdWaves = 4 (128 VGPRs) it spills three registers
template <class K, class... X> struct HasArg { static constexpr bool value = (... || __is_same(K, X)); };
// X: nothing, ExtBwdK (the ext instantiation: kAux, and an aux checkpoint of kExtCkptPlanes planes) or MedBwdK (the median one: kAux)
template <bool kAux, bool kAbs, int kMinWaves, class... X>
__global__ __launch_bounds__(kWave, kMinWaves) void k_render_bwd(FrameK f, const uint2 *__restrict__ ranges,
                                                      const uint32_t *__restrict__ tile_walk,
                                                      const uint32_t *__restrict__ sorted_gid, const uint32_t *__restrict__ sorted_slot,
                                                      const float4 *__restrict__ records, const float *__restrict__ out_color,
                                                      const float *__restrict__ T_state, const int32_t *__restrict__ last_enc,
                                                      const float *__restrict__ dL_dpix, const float *__restrict__ ckpt,
                                                      const float *__restrict__ ckpt_start, float4 *__restrict__ grad_rows,
                                                      uint8_t *__restrict__ row_valid, UnitLists units,
                                                      const uint32_t *__restrict__ unit_count, AuxBwdK ax, X... x)
{
    static_assert(!(kAux && kAbs), "the aux x abs blend backward is not built");
    constexpr bool kExt = HasArg<ExtBwdK, X...>::value, kMed = HasArg<MedBwdK, X...>::value;
    static_assert(sizeof...(X) <= 1 && ((!kExt && !kMed) || kAux), "the extra channels and the median ride on the aux backward");
    constexpr int kSums = kExt ? 13 : kAux ? 10 : kAbs ? 11 : 9;         // per-entry sums
    constexpr int kAccStride = kExt ? 13 : (kAux || kAbs) ? 11 : 9;
    constexpr int kAuxStride = (kExt ? kExtCkptPlanes : 1) * kAuxCkptFloats;      // floats per aux checkpoint
    __shared__ float4 sh_rec[kWave * 3];
    float4 *sh_ext = nullptr;                         // kExt: the batch's rows of the extra table
    ExtBwdK ex{};
    if constexpr (kExt) {
        __shared__ float4 sh_ext_rows[kWave];
        sh_ext = sh_ext_rows;
        ex = ExtBwdK{x...};
    }
    MedBwdK md{};
    if constexpr (kMed) md = MedBwdK{x...};
    __shared__ float sh_acc[kWave * kAccStride];      // the batch's sums, [entry][value]: stride 9 (11) words, conflict-free by lane
#ifdef GSR_BWD_TRACE
    TraceEnd trace_end{(unsigned long long)wall_clock64(), (int)blockIdx.x};
#endif
    const int shard = (int)(blockIdx.x & (kUnitShards - 1));
    uint32_t list_end[kUnitClasses];
    {
        uint32_t run = 0;
#pragma unroll
        for (int k = 0; k < kUnitClasses; ++k) { run += min(unit_count[shard * kUnitClasses + k], units.list_cap(k)); list_end[k] = run; }
    }
    const uint32_t n_units = list_end[kUnitClasses - 1];
    const size_t Tn = (size_t)f.Gx * f.Gy;
    const int lane = threadIdx.x;
    const GroupLanes map(lane);
    const size_t N = (size_t)f.W * f.H;
    const float half_w = 0.5f * (float)f.W, half_h = 0.5f * (float)f.H;
    // where the butterfly leaves this lane's share of a group's totals: which value (of which register), if any
    const int quad = (lane >> 2) & 3, in_quad = lane & 3;
    unsigned acc_idx = (unsigned)(in_quad == 0 ? (quad < 2 ? quad : quad + 2) : in_quad == 1 ? (quad < 2 ? quad + 2 : quad + 4) : ((kAux || kAbs) ? 8 + quad : 8));
    const unsigned grp_shift = 8u * (unsigned)map.grp;
    bool acc_on = in_quad < 2 || (in_quad == 2 && (kAbs ? quad < 3 : kAux ? quad < 2 : quad == 0));
    if constexpr (kExt) {      // values 8 .. 11 with the four quads' third lanes, value 12 with the first quad's fourth
        if (in_quad == 3) acc_idx = 12u;
        acc_on = in_quad < 3 || quad == 0;
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) sh_acc[lane * kAccStride + k] = 0.f;
    for (uint32_t u = blockIdx.x / kUnitShards; u < n_units; u += gridDim.x / kUnitShards) {
        int cls = 0;
        for (int k = 0; k < kUnitClasses - 1; ++k) cls += u >= list_end[k] ? 1 : 0;
        const uint2 unit = units.units[units.list_begin(shard, cls) + (u - (cls ? list_end[cls - 1] : 0u))];
        const int tile = (int)(unit.x & ((1u << kUnitTileBits) - 1u)), c = (int)(unit.x >> kUnitTileBits);
        const int sgm = (int)unit.y;
        const int ty = tile / f.Gx, tx = tile - ty * f.Gx;
        const int px0 = map.x0(tx), py0 = map.y0(ty);
        // dx and dy are one subtraction from the pixel's coordinate, as in the forward kernels: every pixel's lp, alpha and transmittance
        // are the forward's, bit for bit
        const v2f fxv = {(float)px0, (float)(px0 + GroupLanes::kPair)};
        const float fy0 = (float)py0, fy1 = fy0 + (float)GroupLanes::kPair;
        const uint2 rng = ranges[(size_t)c * Tn + tile];
        const int n_total = (int)(rng.y - rng.x);
        const int seg_begin = sgm * kSeg, seg_end = min(n_total, seg_begin + kSeg);
        const int walk_end = min(seg_end, (int)tile_walk[(size_t)c * Tn + tile]);

        BwdPair P0, P1;
        const float *chk = (sgm > 0) ? ckpt + (size_t)((rng.x + (uint32_t)seg_begin) / kSeg) * kCkptFloats
                                     : (c > 0 ? ckpt_start + ((size_t)(c - 1) * Tn + tile) * kCkptFloats : nullptr);
        auto load_px = [&](int e, float &Tk, float &Ek, float &r_, float &g_, float &b_, int &limit) {
            const int px = px0 + map.ex(e), py = py0 + map.ey(e);
            const bool inside = px < f.W && py < f.H;
            const size_t pix = inside ? (size_t)py * f.W + px : 0;
            const int enc = inside ? last_enc[pix] : 0;
            const int c_last = (enc >> kLastShift) - 1;
            limit = c < c_last ? n_total : (c == c_last ? (enc & ((1 << kLastShift) - 1)) : 0);
            const bool has_c = !kAux || dL_dpix != nullptr;      // (the aux kernel takes a NULL colour gradient)
            r_ = inside && has_c ? dL_dpix[pix] : 0.f; g_ = inside && has_c ? dL_dpix[N + pix] : 0.f; b_ = inside && has_c ? dL_dpix[2 * N + pix] : 0.f;
            float er = inside ? out_color[pix] : 0.f, eg = inside ? out_color[N + pix] : 0.f, eb = inside ? out_color[2 * N + pix] : 0.f;
            Tk = 1.f;
            if (chk) {
                // read from one pointer per element: with -ffp-contract=fast the shape of these loads has decided which product of E's
                // sum below the compiler contracts, i.e. its rounding
                const float *q = chk + map.ckpt(e, 0);
                Tk = q[0];
                er -= q[ckpt_word(0, 1, 0, 0)]; eg -= q[ckpt_word(0, 2, 0, 0)]; eb -= q[ckpt_word(0, 3, 0, 0)];
            }
            Ek = er * r_ + eg * g_ + eb * b_;
        };
        {
            float Ta, Ea, ra, ga, bla, Tb, Eb, rb, gb, blb;
            load_px(0, Ta, Ea, ra, ga, bla, P0.limit0); load_px(1, Tb, Eb, rb, gb, blb, P0.limit1);
            P0.T = v2f{Ta, Tb}; P0.E = v2f{Ea, Eb}; P0.dpr = v2f{ra, rb}; P0.dpg = v2f{ga, gb}; P0.dpb = v2f{bla, blb};
            load_px(2, Ta, Ea, ra, ga, bla, P1.limit0); load_px(3, Tb, Eb, rb, gb, blb, P1.limit1);
            P1.T = v2f{Ta, Tb}; P1.E = v2f{Ea, Eb}; P1.dpr = v2f{ra, rb}; P1.dpg = v2f{ga, gb}; P1.dpb = v2f{bla, blb};
        }
        BwdPairAux PA0, PA1;
        if constexpr (kAux) {
            // E gains g_z (depth_final - Z in front of the segment); GA = g_a T_final, T_final = |T_state| (frozen at the stop)
            const float *zchk = (sgm > 0) ? ax.ckpt + (size_t)((rng.x + (uint32_t)seg_begin) / kSeg) * kAuxStride
                                          : (c > 0 ? ax.ckpt_start + ((size_t)(c - 1) * Tn + tile) * kAuxStride : nullptr);
            auto load_aux = [&](int e, float &E, float &gz, float &gaT) {
                const int px = px0 + map.ex(e), py = py0 + map.ey(e);
                const bool inside = px < f.W && py < f.H;
                const size_t pix = inside ? (size_t)py * f.W + px : 0;
                gz = inside && ax.dL_ddepth ? ax.dL_ddepth[pix] : 0.f;
                gaT = inside && ax.dL_dalpha ? ax.dL_dalpha[pix] * fabsf(T_state[pix]) : 0.f;
                const float zf = inside ? ax.depth[pix] : 0.f, zc = zchk ? zchk[map.aux(e)] : 0.f;
                E += gz * (zf - zc);
            };
            float E0 = P0.E[0], E1 = P0.E[1], E2 = P1.E[0], E3 = P1.E[1], z0, z1, z2, z3, a0, a1, a2, a3;
            load_aux(0, E0, z0, a0); load_aux(1, E1, z1, a1); load_aux(2, E2, z2, a2); load_aux(3, E3, z3, a3);
            P0.E = v2f{E0, E1}; PA0.dpz = v2f{z0, z1}; PA0.GA = v2f{a0, a1};
            P1.E = v2f{E2, E3}; PA1.dpz = v2f{z2, z3}; PA1.GA = v2f{a2, a3};
        }
        BwdPairMed PM0{}, PM1{};
        if constexpr (kMed) {
            auto load_med = [&](int e, float &gm, int &mpos) {
                const int px = px0 + map.ex(e), py = py0 + map.ey(e);
                const bool inside = px < f.W && py < f.H;
                const size_t pix = inside ? (size_t)py * f.W + px : 0;
                gm = inside && md.dL_dmedian ? md.dL_dmedian[pix] : 0.f;
                const int enc = inside ? md.median_enc[pix] : 0;
                mpos = (enc >> kLastShift) - 1 == c ? (enc & ((1 << kLastShift) - 1)) : 0;
            };
            float g0, g1, g2, g3;
            load_med(0, g0, PM0.mpos0); load_med(1, g1, PM0.mpos1); load_med(2, g2, PM1.mpos0); load_med(3, g3, PM1.mpos1);
            PM0.gm = v2f{g0, g1}; PM1.gm = v2f{g2, g3};
        }
        BwdPairExt PE0{}, PE1{};
        if constexpr (kExt) {
            // E gains <extra_final - extra in front of the segment, g_e>
            const float *zchk = (sgm > 0) ? ax.ckpt + (size_t)((rng.x + (uint32_t)seg_begin) / kSeg) * kAuxStride
                                          : (c > 0 ? ax.ckpt_start + ((size_t)(c - 1) * Tn + tile) * kAuxStride : nullptr);
            auto load_ext = [&](int e, float &E, float &g0, float &g1, float &g2) {
                const int px = px0 + map.ex(e), py = py0 + map.ey(e);
                const bool inside = px < f.W && py < f.H;
                const size_t pix = inside ? (size_t)py * f.W + px : 0;
                const bool has = inside && ex.dL_dmap != nullptr;
                g0 = has ? ex.dL_dmap[pix] : 0.f; g1 = has ? ex.dL_dmap[N + pix] : 0.f; g2 = has ? ex.dL_dmap[2 * N + pix] : 0.f;
                float d0 = inside ? ex.map[pix] : 0.f, d1 = inside ? ex.map[N + pix] : 0.f, d2 = inside ? ex.map[2 * N + pix] : 0.f;
                if (zchk) {
                    const float *q = zchk + map.aux(e);
                    d0 -= q[kAuxCkptFloats]; d1 -= q[2 * kAuxCkptFloats]; d2 -= q[3 * kAuxCkptFloats];
                }
                E += g0 * d0 + g1 * d1 + g2 * d2;
            };
            float E0 = P0.E[0], E1 = P0.E[1], E2 = P1.E[0], E3 = P1.E[1], g[4][3];
            load_ext(0, E0, g[0][0], g[0][1], g[0][2]); load_ext(1, E1, g[1][0], g[1][1], g[1][2]);
            load_ext(2, E2, g[2][0], g[2][1], g[2][2]); load_ext(3, E3, g[3][0], g[3][1], g[3][2]);
            P0.E = v2f{E0, E1}; PE0.dpe0 = v2f{g[0][0], g[1][0]}; PE0.dpe1 = v2f{g[0][1], g[1][1]}; PE0.dpe2 = v2f{g[0][2], g[1][2]};
            P1.E = v2f{E2, E3}; PE1.dpe0 = v2f{g[2][0], g[3][0]}; PE1.dpe1 = v2f{g[2][1], g[3][1]}; PE1.dpe2 = v2f{g[2][2], g[3][2]};
        }
        // per quadrant (= per group): its last participating contributor
        int gmax = max(max(P0.limit0, P0.limit1), max(P1.limit0, P1.limit1));
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) gmax = max(gmax, __shfl_xor(gmax, off));
        const int qmax0 = min(walk_end, __builtin_amdgcn_readlane(gmax, 0)), qmax1 = min(walk_end, __builtin_amdgcn_readlane(gmax, 16)),
                  qmax2 = min(walk_end, __builtin_amdgcn_readlane(gmax, 32)), qmax3 = min(walk_end, __builtin_amdgcn_readlane(gmax, 48));
        const int max_contrib = max(max(qmax0, qmax1), max(qmax2, qmax3));

        for (int base = seg_begin; base < seg_end; base += kWave) {
            if (base >= max_contrib) break;
            const int n = min(kWave, seg_end - base);
            const uint32_t slot = lane < n ? sorted_slot[rng.x + base + lane] : 0u;
            __syncthreads();
            unsigned mymask;
            if constexpr (kExt) mymask = stage_batch_ext(sh_rec, sh_ext, lane, n, sorted_gid, rng.x + base, records, ex.table);
            else mymask = stage_batch(sh_rec, lane, n, sorted_gid, rng.x + base, records);
            __syncthreads();
            const int mypos = base + lane;
            mymask &= (mypos < qmax0 ? 1u : 0u) | (mypos < qmax1 ? 2u : 0u) | (mypos < qmax2 ? 4u : 0u) | (mypos < qmax3 ? 8u : 0u);
            GroupWalk walk(mymask, 15u);
            // a pixel's limit relative to the batch, clamped to [0, 64]: an idle group's entry number (255) fails it by itself
            const int L00 = P0.limit0, L01 = P0.limit1, L10 = P1.limit0, L11 = P1.limit1;
            P0.limit0 = min(max(L00 - base, 0), kWave); P0.limit1 = min(max(L01 - base, 0), kWave);
            P1.limit0 = min(max(L10 - base, 0), kWave); P1.limit1 = min(max(L11 - base, 0), kWave);
            while (walk.more()) {
                unsigned jj;
                const unsigned j = walk.next(grp_shift, jj);
                const float4 a = sh_rec[3u * jj], b = sh_rec[3u * jj + 1u];
                const BwdSplat sp{b.y, b.z, b.w, sh_rec[3u * jj + 2u].x, kAux ? sh_rec[3u * jj + 2u].y : 0.f};
                const v2f dx = a.x - fxv;
                const LpTerms lt = lp_terms(a.z, a.w, b.y, dx);
                BwdAcc A;
                v2f S9;                                  // aux: the lane's sum of w dL/ddepth
                BwdAbs AB;                               // abs: the lane's sums of |u|
                const BwdAbsQ Q{2.f * a.z, a.w, 2.f * b.x};
                BwdAccExt AE;                            // ext: the lane's sums of w dL/dextra
                // median: the entry's position + 1 in the chunk's list, as median_enc counts it (an idle group's pass: never a median)
                const int mabs = kMed && j < (unsigned)kWave ? base + (int)j + 1 : -1;
                if constexpr (kExt) {
                    const float4 xe = sh_ext[jj];        // the splat's extra triple
                    float xe1 = xe.y;
                    // (an opaque copy, no instruction: without it the compiler pairs (e1, e2) out of the 96-bit LDS read as an unaligned
                    // register pair and legalises that through 16 bytes of scratch)
                    asm volatile("" : "+v"(xe1));
                    const BwdExt se{xe.x, xe1, xe.z};
                    const float dy0 = a.y - fy0, dy1 = a.y - fy1;
                    bwd_pair<true, true, false, true>(sp, lp_at(lt, b.x, dy0), dx, dy0, (int)j, P0, A, PA0, &S9, Q, nullptr, &se, &PE0, &AE);
                    bwd_pair<false, true, false, true>(sp, lp_at(lt, b.x, dy1), dx, dy1, (int)j, P1, A, PA1, &S9, Q, nullptr, &se, &PE1, &AE);
                } else {
                    {
                        const float dy = a.y - fy0;
                        if constexpr (kAbs) bwd_pair<true, false, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P0, A, PA0, nullptr, Q, &AB);
                        else if constexpr (kMed) bwd_pair<true, true, false, false, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P0, A, PA0, &S9, Q, nullptr, nullptr, nullptr, nullptr, mabs, &PM0);
                        else if constexpr (kAux) bwd_pair<true, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P0, A, PA0, &S9);
                        else bwd_pair<true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P0, A);
                    }
                    {
                        const float dy = a.y - fy1;
                        if constexpr (kAbs) bwd_pair<false, false, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P1, A, PA1, nullptr, Q, &AB);
                        else if constexpr (kMed) bwd_pair<false, true, false, false, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P1, A, PA1, &S9, Q, nullptr, nullptr, nullptr, nullptr, mabs, &PM1);
                        else if constexpr (kAux) bwd_pair<false, true>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P1, A, PA1, &S9);
                        else bwd_pair<false>(sp, lp_at(lt, b.x, dy), dx, dy, (int)j, P1, A);
                    }
                }
                float mine;
                if constexpr (kExt) {
                    float s[10] = {add_halves(A.X), add_halves(A.Y), add_halves(A.S2), add_halves(A.S3), add_halves(A.S4), add_halves(A.S5),
                                   add_halves(A.S6), add_halves(A.S7), add_halves(A.S8), add_halves(S9)};
                    float t[3] = {add_halves(AE.S10), add_halves(AE.S11), add_halves(AE.S12)};
                    row_sum10_transpose(s);
                    row_sum3_rows(t);
                    mine = in_quad == 0 ? s[0] : in_quad == 1 ? s[2] : in_quad == 3 ? t[2] : (quad == 0 ? s[8] : quad == 1 ? s[9] : quad == 2 ? t[0] : t[1]);
                } else if constexpr (kAbs) {
                    float s[11] = {add_halves(A.X), add_halves(A.Y), add_halves(A.S2), add_halves(A.S3), add_halves(A.S4), add_halves(A.S5),
                                   add_halves(A.S6), add_halves(A.S7), add_halves(A.S8), add_halves(AB.AX), add_halves(AB.AY)};
                    row_sum11_transpose(s);
                    mine = in_quad == 0 ? s[0] : in_quad == 1 ? s[2] : (quad == 0 ? s[8] : quad == 1 ? s[9] : s[10]);
                } else if constexpr (kAux) {
                    float s[10] = {add_halves(A.X), add_halves(A.Y), add_halves(A.S2), add_halves(A.S3), add_halves(A.S4), add_halves(A.S5),
                                   add_halves(A.S6), add_halves(A.S7), add_halves(A.S8), add_halves(S9)};
                    row_sum10_transpose(s);
                    mine = in_quad == 0 ? s[0] : in_quad == 1 ? s[2] : (quad == 0 ? s[8] : s[9]);
                } else {
                    float s[9] = {add_halves(A.X), add_halves(A.Y), add_halves(A.S2), add_halves(A.S3), add_halves(A.S4), add_halves(A.S5),
                                  add_halves(A.S6), add_halves(A.S7), add_halves(A.S8)};
                    row_sum9_transpose(s);
                    mine = in_quad == 0 ? s[0] : in_quad == 1 ? s[2] : s[8];
                }
                // groups that meet on an entry in the same pass add in group order, one LDS instruction per group: the order of every
                // floating-point sum is fixed by the program
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (acc_on && j < (unsigned)kWave && map.grp == k) atomicAdd(&sh_acc[jj * (unsigned)kAccStride + acc_idx], mine);
            }
            P0.limit0 = L00; P0.limit1 = L01; P1.limit0 = L10; P1.limit1 = L11;
            __syncthreads();
            if (mymask != 0u) {
                float v[kSums];
#pragma unroll
                for (int k = 0; k < kSums; ++k) { v[k] = sh_acc[lane * kAccStride + k]; sh_acc[lane * kAccStride + k] = 0.f; }
                const float4 a = sh_rec[3 * lane], b = sh_rec[3 * lane + 1];
                // -(X cA + Y cB) = ln2 (2 qA X + qB Y), likewise for y; gA, gB, gC carry the -1/2 of A.9; dL/dopacity = sum / opacity
                const float gx = 2.f * a.z * v[0] + a.w * v[1], gy = 2.f * b.x * v[1] + a.w * v[0];
                float4 *row = grad_rows + 3 * (size_t)slot;
                row[0] = make_float4(gx * (0.69314718f * half_w), gy * (0.69314718f * half_h), v[2] * -0.5f, v[3] * -0.5f);
                row[1] = make_float4(v[4] * -0.5f, v[5] * __builtin_amdgcn_exp2f(-b.y), v[6], v[7]);
                if constexpr (kAbs) row[2] = make_float4(v[8], 0.f, v[9] * (0.69314718f * half_w), v[10] * (0.69314718f * half_h));
                else row[2] = make_float4(v[8], kAux ? v[kExt ? 9 : kSums - 1] : 0.f, 0.f, 0.f);
                if constexpr (kExt) ex.rows[slot] = make_float4(v[10 < kSums ? 10 : 0], v[11 < kSums ? 11 : 0], v[12 < kSums ? 12 : 0], 0.f);
                row_valid[slot] = 1;
            }
        }
    }
}

int launch_render_bwd(const FrameK &f, int chunks_run, int sort_result, long long rows_upper, const GeomWS &gw, BinningWS &bw,
                      const ImageWS &iw, const float *out_color, const float *dL_dcolor, bool debug, hipStream_t s, const BwdVariant &v)
{
    const int n_tiles = (f.ty1 - f.ty0) * f.Gx;
    if (n_tiles <= 0 || chunks_run <= 0) return GSR_OK;
    // one block per unit while they fit the grid; the counts are the device's (the forward appended the units), the bound the
    // host's: a (tile, chunk) pair has at most n / kSeg + 1 units.  Blocks are dealt to the shards round-robin.
    long long per_shard = (rows_upper / kSeg + (long long)n_tiles * chunks_run) / kUnitShards + 1;
    if (per_shard > (long long)bw.units.shard_stride()) per_shard = (long long)bw.units.shard_stride();
    if (per_shard > (1 << 13)) per_shard = 1 << 13;
    // by BwdKind: the instantiations take the same arguments; only the aux one reads the aux block
    static const decltype(&k_render_bwd<false, false, kBwdWaves>) kernels[] = {k_render_bwd<false, false, kBwdWaves>, k_render_bwd<true, false, kBwdWaves>,
                                                                               k_render_bwd<false, true, kBwdWaves>};
    static const char *const names[] = {"render_bwd", "render_bwd_aux", "render_bwd_abs", "render_bwd_ext", "render_bwd_median"};
    const char *name = names[(int)v.kind];
    const bool with_aux = v.kind == BwdKind::kAux || v.kind == BwdKind::kExt || v.kind == BwdKind::kMed;
    const AuxBwdK ax = with_aux ? AuxBwdK{v.aux->depth, v.dL_ddepth, v.dL_dalpha, v.aux->ckpt, v.aux->ckpt_start} : AuxBwdK{};
    ProfileScope prof(name, s);
    if (v.kind == BwdKind::kExt) {
        const ExtBwdK ex{v.ext->table, v.ext->map, v.ext->dL_dmap, v.ext->rows};
        hipLaunchKernelGGL((k_render_bwd<true, false, kBwdExtWaves, ExtBwdK>), dim3((unsigned)(per_shard * kUnitShards)), dim3(kWave), 0, s, f,
                           iw.ranges, iw.tile_walk, bw.gids[1], bw.vals[sort_result], gw.records, out_color, iw.T_state, iw.last_enc, dL_dcolor,
                           bw.ckpt, iw.ckpt_start, reinterpret_cast<float4 *>(bw.grad_rows), bw.row_valid, bw.units, iw.unit_count, ax, ex);
        GSR_LAUNCH_CHECK(name, debug, s);
        return GSR_OK;
    }
    if (v.kind == BwdKind::kMed) {
        const MedBwdK md{v.med->median_enc, v.med->dL_dmedian};
        hipLaunchKernelGGL((k_render_bwd<true, false, kBwdWaves, MedBwdK>), dim3((unsigned)(per_shard * kUnitShards)), dim3(kWave), 0, s, f,
                           iw.ranges, iw.tile_walk, bw.gids[1], bw.vals[sort_result], gw.records, out_color, iw.T_state, iw.last_enc, dL_dcolor,
                           bw.ckpt, iw.ckpt_start, reinterpret_cast<float4 *>(bw.grad_rows), bw.row_valid, bw.units, iw.unit_count, ax, md);
        GSR_LAUNCH_CHECK(name, debug, s);
        return GSR_OK;
    }
    hipLaunchKernelGGL(kernels[(int)v.kind], dim3((unsigned)(per_shard * kUnitShards)), dim3(kWave), 0, s, f,
                       iw.ranges, iw.tile_walk, bw.gids[1], bw.vals[sort_result], gw.records, out_color, iw.T_state, iw.last_enc, dL_dcolor,
                       bw.ckpt, iw.ckpt_start, reinterpret_cast<float4 *>(bw.grad_rows), bw.row_valid, bw.units, iw.unit_count, ax);
    GSR_LAUNCH_CHECK(name, debug, s);
    return GSR_OK;
}

// ---- per-Gaussian reduction of the instance rows (bitwise reproducible: fixed lane assignment and a fixed
// shuffle tree).  EIGHT lanes cooperate on one depth rank (8 ranks per wave): lane i of the group sums rows
// i, i+8, ... and three xor-shuffles combine the group.  The near, screen-filling Gaussians own hundreds of
// rows each; one thread per Gaussian left a tail of a few thousand threads walking them serially.
// Only ranks of chunks that actually ran can own rows; every other Gaussian's gradient row is zero (memset).
// kAux: rows of the aux backward - slot 9 (dL/dz) is summed too, in the same order as the others.
// kAbs: rows of the abs backward - slots 10, 11 likewise, into screen[3 g + 2].zw.
// kExt (X = the ext backward's row plane [R] float4 and dL_dextra [P, 3]; with kAux): the plane's three sums are added beside the
// row's, trip for trip and in the same tree, and the group's fourth lane writes them to dL_dextra[g].
constexpr int kRedBlock = 256;
template <int kRedGroup, bool kAux = false, bool kAbs = false, class... X>
__global__ __launch_bounds__(kRedBlock) void k_reduce_rows(int r_begin, int n_ranks, const uint32_t *__restrict__ order,
                                                           const uint32_t *__restrict__ cnt_open,
                                                           const uint32_t *__restrict__ row_begin,
                                                           const uint8_t *__restrict__ row_valid,
                                                           const float4 *__restrict__ grad_rows, float4 *__restrict__ screen,
                                                           int write_empty, int plain, X... x)
{
    constexpr bool kExt = sizeof...(X) == 2;
    static_assert(sizeof...(X) == 0 || (kExt && kAux && kRedGroup >= 4), "the ext reduction rides on the aux one");
    const float4 *ext_rows = nullptr;
    float *dL_dextra = nullptr;
    if constexpr (kExt) {
        auto take = [&](const float4 *r, float *d) { ext_rows = r; dL_dextra = d; };
        take(x...);
    }
    float ax0 = 0.f, ax1 = 0.f, ax2 = 0.f;             // kExt: the three sums
    const int sub = threadIdx.x & (kRedGroup - 1);
    const int r = r_begin + (blockIdx.x * kRedBlock + threadIdx.x) / kRedGroup;
    const bool live = r < n_ranks;
    // the rank's three words in one round trip (the chain was count -> first row -> rows -> Gaussian: four)
    const uint32_t cnt = live ? cnt_open[r] : 0u, begin = live ? row_begin[r] : 0u, g = live ? order[r] : 0u;
    float4 a0 = make_float4(0.f, 0.f, 0.f, 0.f), a1 = a0;
    float a8 = 0.f, a9 = 0.f, a10 = 0.f, a11 = 0.f;
    bool batched = false;
    if constexpr (kRedGroup >= 64) batched = !plain;
    if (cnt && batched) {
        // Wide groups, kRedBatch trips of a lane at a time: the rows of the batch's valid trips are loaded together, and with them
        // the valid bytes of the NEXT batch (clamped to the lane's last row, masked after), then the rows are added in ascending
        // row order - the adds of the plain loop below in its order, so the same bits, with ceil(trips / kRedBatch) + 1 dependent
        // round trips on a lane's chain instead of 2 trips
        constexpr int kRedBatch = 8;
        const size_t end = (size_t)begin + cnt, first = (size_t)begin + (size_t)sub;
        uint32_t ok[kRedBatch], nx[kRedBatch];
        if (first < end) {
#pragma unroll
            for (int u = 0; u < kRedBatch; ++u) {
                const size_t su = first + (size_t)(u * kRedGroup);
                ok[u] = row_valid[su < end ? su : first];
                if (su >= end) ok[u] = 0u;
            }
        }
        for (size_t sl = first; sl < end; sl += kRedBatch * kRedGroup) {
            float4 r0[kRedBatch], r1[kRedBatch], r2[kRedBatch];
            float4 r3[kExt ? kRedBatch : 1];
            const size_t sn = sl + kRedBatch * kRedGroup;
#pragma unroll
            for (int u = 0; u < kRedBatch; ++u) {
                const size_t su = sn + (size_t)(u * kRedGroup);
                nx[u] = row_valid[su < end ? su : sl];
                if (su >= end) nx[u] = 0u;
            }
#pragma unroll
            for (int u = 0; u < kRedBatch; ++u) {
                const size_t su = sl + (size_t)(u * kRedGroup);
                if (ok[u]) {
                    r0[u] = grad_rows[3 * su]; r1[u] = grad_rows[3 * su + 1];
                    if constexpr (kAux || kAbs) r2[u] = grad_rows[3 * su + 2];
                    else r2[u].x = grad_rows[3 * su + 2].x;
                    if constexpr (kExt) r3[u] = ext_rows[su];
                }
            }
#pragma unroll
            for (int u = 0; u < kRedBatch; ++u) {
                if (ok[u]) {
                    a0.x += r0[u].x; a0.y += r0[u].y; a0.z += r0[u].z; a0.w += r0[u].w;
                    a1.x += r1[u].x; a1.y += r1[u].y; a1.z += r1[u].z; a1.w += r1[u].w;
                    a8 += r2[u].x;
                    if constexpr (kAux) a9 += r2[u].y;
                    if constexpr (kExt) { ax0 += r3[u].x; ax1 += r3[u].y; ax2 += r3[u].z; }
                    if constexpr (kAbs) { a10 += r2[u].z; a11 += r2[u].w; }
                }
                ok[u] = nx[u];
            }
        }
    } else if (cnt) {
        for (uint32_t sl = begin + sub; sl < begin + cnt; sl += kRedGroup) {
            // a clear valid byte: nobody walked that far into the tile's list, or no pixel accepted the splat — the row was never
            // written.  Wide groups (big splats: most rows of a saturating frame are invalid) test the byte first; narrow ones (small
            // splats, nearly every row valid) load the row beside its byte — one memory round trip instead of two — and drop it after
            float4 r0, r1;
            float4 r3 = make_float4(0.f, 0.f, 0.f, 0.f);
            float r2, r9 = 0.f, r10 = 0.f, r11 = 0.f;
            if constexpr (kRedGroup >= 64) {
                if (!row_valid[sl]) continue;
                r0 = grad_rows[3 * (size_t)sl]; r1 = grad_rows[3 * (size_t)sl + 1]; r2 = grad_rows[3 * (size_t)sl + 2].x;
                if constexpr (kAux) r9 = grad_rows[3 * (size_t)sl + 2].y;
                if constexpr (kAbs) { r10 = grad_rows[3 * (size_t)sl + 2].z; r11 = grad_rows[3 * (size_t)sl + 2].w; }
                if constexpr (kExt) r3 = ext_rows[sl];
            } else {
                const uint8_t ok = row_valid[sl];
                r0 = grad_rows[3 * (size_t)sl]; r1 = grad_rows[3 * (size_t)sl + 1]; r2 = grad_rows[3 * (size_t)sl + 2].x;
                if constexpr (kAux) r9 = grad_rows[3 * (size_t)sl + 2].y;
                if constexpr (kAbs) { r10 = grad_rows[3 * (size_t)sl + 2].z; r11 = grad_rows[3 * (size_t)sl + 2].w; }
                if constexpr (kExt) r3 = ext_rows[sl];
                if (!ok) continue;                      // (whatever the unwritten row holds — NaN patterns included — is never added)
            }
            a0.x += r0.x; a0.y += r0.y; a0.z += r0.z; a0.w += r0.w;
            a1.x += r1.x; a1.y += r1.y; a1.z += r1.z; a1.w += r1.w;
            a8 += r2;
            if constexpr (kAux) a9 += r9;
            if constexpr (kAbs) { a10 += r10; a11 += r11; }
            if constexpr (kExt) { ax0 += r3.x; ax1 += r3.y; ax2 += r3.z; }
        }
    }
#pragma unroll
    for (int off = kRedGroup / 2; off >= 1; off >>= 1) {
        a0.x += __shfl_xor(a0.x, off); a0.y += __shfl_xor(a0.y, off); a0.z += __shfl_xor(a0.z, off); a0.w += __shfl_xor(a0.w, off);
        a1.x += __shfl_xor(a1.x, off); a1.y += __shfl_xor(a1.y, off); a1.z += __shfl_xor(a1.z, off); a1.w += __shfl_xor(a1.w, off);
        a8 += __shfl_xor(a8, off);
        if constexpr (kAux) a9 += __shfl_xor(a9, off);
        if constexpr (kAbs) { a10 += __shfl_xor(a10, off); a11 += __shfl_xor(a11, off); }
        if constexpr (kExt) { ax0 += __shfl_xor(ax0, off); ax1 += __shfl_xor(ax1, off); ax2 += __shfl_xor(ax2, off); }
    }
    if (live && (cnt || write_empty) && sub < 3)
        screen[3 * (size_t)g + sub] = sub == 0 ? a0 : (sub == 1 ? a1 : make_float4(a8, a9, a10, a11));
    if constexpr (kExt) {
        if (live && (cnt || write_empty) && sub == 3) {
            dL_dextra[3 * (size_t)g] = ax0; dL_dextra[3 * (size_t)g + 1] = ax1; dL_dextra[3 * (size_t)g + 2] = ax2;
        }
    }
}

// One launch per depth chunk that ran, each with its own lanes-per-Gaussian: a whole wave or eight (gsr_dispatch.h reduce_wide)
int launch_reduce_rows(const FrameK &f, const gsr_frame_plan &plan, const GeomWS &gw, const BinningWS &bw, float *screen_grads,
                       int prezeroed, bool debug, hipStream_t s, BwdKind kind, const ExtWS *ext)
{
    // prezeroed: 0 = clear the whole tensor first; 1 = the caller already has; 2 = only the rows of the binned prefix will ever
    // be read (the sparse geometry backward of the same frame): every prefix row is written, zeros included, nothing else
    if (f.P == 0) return GSR_OK;
    // by BwdKind, then narrow / wide groups
    static const decltype(&k_reduce_rows<8>) kernels[][2] = {{k_reduce_rows<8>, k_reduce_rows<64>},
                                                             {k_reduce_rows<8, true>, k_reduce_rows<64, true>},
                                                             {k_reduce_rows<8, false, true>, k_reduce_rows<64, false, true>}};
    static const char *const names[] = {"reduce_rows", "reduce_rows_aux", "reduce_rows_abs", "reduce_rows_ext"};
    ProfileScope prof(names[(int)kind], s);
    // a Gaussian without a row - outside the chunks that ran, or never emitted - gets exactly 0
    if (kind == BwdKind::kExt) GSR_HIP_CHECK(hipMemsetAsync(ext->dL_dtable, 0, (size_t)f.P * 3 * sizeof(float), s));
    if (prezeroed == 0) GSR_HIP_CHECK(hipMemsetAsync(screen_grads, 0, (size_t)f.P * kRowFloats * sizeof(float), s));
    const int write_empty = prezeroed == 2 ? 1 : 0;
    const int plain = switches().reduce_rows_plain ? 1 : 0;
    const int chunks = (plan.num_rendered > 0 && plan.chunks_run > 0) ? plan.chunks_run : 0;
    for (int c = 0; c < chunks && c < GSR_MAX_CHUNKS; ++c) {
        const int r0 = plan.chunk_rank_begin[c], r1 = plan.chunk_rank_begin[c + 1];
        if (r1 <= r0) continue;
        const bool wide = reduce_wide(r1 - r0, plan.chunk_instances_max[c], (plan.chunks_filtered >> c) & 1);
        const long long threads = (long long)(r1 - r0) * (wide ? 64 : 8);
        const dim3 grid((unsigned)((threads + kRedBlock - 1) / kRedBlock));
        if (kind == BwdKind::kExt) {
            const auto kernel = wide ? k_reduce_rows<64, true, false, const float4 *, float *> : k_reduce_rows<8, true, false, const float4 *, float *>;
            hipLaunchKernelGGL(kernel, grid, dim3(kRedBlock), 0, s, r0, r1, gw.order, gw.cnt_open, gw.row_begin, bw.row_valid,
                               reinterpret_cast<const float4 *>(bw.grad_rows), reinterpret_cast<float4 *>(screen_grads), write_empty, plain,
                               (const float4 *)ext->rows, ext->dL_dtable);
            continue;
        }
        hipLaunchKernelGGL(kernels[(int)kind][wide], grid, dim3(kRedBlock), 0, s, r0, r1, gw.order, gw.cnt_open, gw.row_begin,
                           bw.row_valid, reinterpret_cast<const float4 *>(bw.grad_rows), reinterpret_cast<float4 *>(screen_grads), write_empty, plain);
    }
    GSR_LAUNCH_CHECK("reduce_rows", debug, s);
    return GSR_OK;
}

}  // namespace gsr
