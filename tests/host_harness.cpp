// host_harness.cpp — TEST INFRASTRUCTURE.  Compiles the product's per-Gaussian maths header
// (structured-gaussian-splatting_amd/csrc/gsr_math.h, the functions the HIP kernels wrap) with g++
// so tests/test_host_math.py can check the formulas against the oracle without a GPU.
// Nothing in the product loads this library.
#include <cstdint>
#include <cstring>

#include "../structured-gaussian-splatting_amd/csrc/gsr_math.h"

using namespace gsr;

static FrameK make_frame(int P, int D, int M, int W, int H, float tanfovx, float tanfovy, float mod, int ty0, int ty1)
{
    FrameK f;
    f.P = P; f.D = D; f.M = M; f.W = W; f.H = H;
    f.Gx = (W + GSR_TILE - 1) / GSR_TILE; f.Gy = (H + GSR_TILE - 1) / GSR_TILE;
    f.ty0 = ty0 < 0 ? 0 : ty0;
    f.ty1 = (ty1 <= 0 || ty1 > f.Gy) ? f.Gy : ty1;
    f.tanfovx = tanfovx; f.tanfovy = tanfovy;
    f.focal_x = (float)W / (2.f * tanfovx); f.focal_y = (float)H / (2.f * tanfovy);
    f.scale_modifier = mod;
    return f;
}

extern "C" void hh_preprocess(int P, int D, int M, int W, int H, float tanfovx, float tanfovy, float mod, int ty0, int ty1,
                              const float *V, const float *PV, const float *campos, const float *means, const float *scales,
                              const float *rots, const float *covpre, const float *opac, const float *shs,
                              const float *colpre, int32_t *radii, uint32_t *tiles, uint8_t *clamped, float *records)
{
    FrameK f = make_frame(P, D, M, W, H, tanfovx, tanfovy, mod, ty0, ty1);
    for (int i = 0; i < P; ++i) {
        PreOut o;
        preprocess_one(f, V, PV, campos, means + 3 * i, scales ? scales + 3 * i : nullptr, rots ? rots + 4 * i : nullptr,
                       covpre ? covpre + 6 * i : nullptr, opac[i], shs ? shs + (size_t)i * M * 3 : nullptr,
                       colpre ? colpre + 3 * i : nullptr, o);
        radii[i] = o.radius; tiles[i] = o.tiles; clamped[i] = (uint8_t)o.clamped;
        std::memcpy(records + 12 * i, &o.s, sizeof(Splat));
    }
}

extern "C" void hh_geom_backward(int P, int D, int M, int W, int H, float tanfovx, float tanfovy, float mod,
                                 const float *V, const float *PV, const float *campos, const float *means,
                                 const float *scales, const float *rots, const float *covpre, const float *shs,
                                 int has_colpre, const int32_t *radii, const uint8_t *clamped, const float *screen9,
                                 float *dmeans3D, float *dmeans2D, float *dsh, float *dcolors, float *dopac,
                                 float *dscales, float *drots, float *dcov)
{
    FrameK f = make_frame(P, D, M, W, H, tanfovx, tanfovy, mod, 0, 0);
    for (int i = 0; i < P; ++i) {
        if (radii[i] <= 0) continue;
        GeomGrad g;
        geom_backward_one(f, V, PV, campos, means + 3 * i, scales ? scales + 3 * i : nullptr, rots ? rots + 4 * i : nullptr,
                          covpre ? covpre + 6 * i : nullptr, shs ? shs + (size_t)i * M * 3 : nullptr, has_colpre != 0,
                          clamped[i], screen9 + 9 * i, g, (shs && dsh) ? dsh + (size_t)i * M * 3 : nullptr, shs && dsh);
        for (int k = 0; k < 3; ++k) { dmeans3D[3 * i + k] = g.dmean[k]; dcolors[3 * i + k] = g.dcolor[k]; dscales[3 * i + k] = g.dscale[k]; }
        dmeans2D[3 * i] = g.dmean2D[0]; dmeans2D[3 * i + 1] = g.dmean2D[1]; dmeans2D[3 * i + 2] = 0.f;
        dopac[i] = g.dopacity;
        for (int k = 0; k < 4; ++k) drots[4 * i + k] = g.drot[k];
        for (int k = 0; k < 6; ++k) dcov[6 * i + k] = g.dcov[k];
    }
}

extern "C" void hh_tile_may_contribute(int n, const float *sx, const float *sy, const float *A, const float *B, const float *C,
                                       const float *op, const int32_t *tx, const int32_t *ty, uint8_t *out)
{
    for (int i = 0; i < n; ++i) out[i] = tile_may_contribute(sx[i], sy[i], A[i], B[i], C[i], op[i], tx[i], ty[i]) ? 1 : 0;
}

// A.3: packed covariance from scale * modifier and a (normalised) quaternion
extern "C" void hh_cov3d(int n, const float *scales, const float *quats, float mod, float *cov6)
{
    for (int i = 0; i < n; ++i) cov3d_from_scale_rot(scales + 3 * i, mod, quats + 4 * i, cov6 + 6 * i);
}

// sub-tile culling on the pre-scaled record: 4-bit quadrant mask per (splat, tile)
extern "C" void hh_quadrant_mask(int n, const float *rec12, const int32_t *tx, const int32_t *ty, uint8_t *out)
{
    for (int i = 0; i < n; ++i) {
        const float *r = rec12 + 12 * (size_t)i;
        out[i] = (uint8_t)quadrant_mask_q(r[0], r[1], r[2], r[3], r[4], r[5], (float)(tx[i] * GSR_TILE), (float)(ty[i] * GSR_TILE));
    }
}

extern "C" void hh_quadrant_mask_bbox(int n, const float *rec12, const int32_t *tx, const int32_t *ty, uint8_t *out)
{
    for (int i = 0; i < n; ++i) {
        const float *r = rec12 + 12 * (size_t)i;
        float xe, ye;
        splat_extent_q(r[2], r[3], r[4], r[5], xe, ye);
        out[i] = (uint8_t)quadrant_mask_bbox(r[0], r[1], xe, ye, (float)(tx[i] * GSR_TILE), (float)(ty[i] * GSR_TILE));
    }
}

// a14: activations of the raw parameters and their chain rule (gsr_math.h activate_raw / activate_raw_backward).
// in: log_scales[n,3], raw_q[n,4], logits[n]; upstream d_scale[n,3], d_q[n,4], d_op[n]
// out: scale[n,3], q[n,4], op[n] and the gradients w.r.t. the raw values in g_ls[n,3], g_rq[n,4], g_logit[n]
extern "C" void hh_activate_raw(int n, const float *log_scales, const float *raw_q, const float *logits, const float *d_scale,
                                const float *d_q, const float *d_op, float *scale, float *q, float *op, float *g_ls,
                                float *g_rq, float *g_logit)
{
    for (int i = 0; i < n; ++i) {
        RawAct a;
        activate_raw(log_scales + 3 * i, raw_q + 4 * i, logits[i], a);
        for (int k = 0; k < 3; ++k) scale[3 * i + k] = a.scale[k];
        for (int k = 0; k < 4; ++k) q[4 * i + k] = a.q[k];
        op[i] = a.opacity;
        GeomGrad g;
        for (int k = 0; k < 3; ++k) g.dscale[k] = d_scale[3 * i + k];
        for (int k = 0; k < 4; ++k) g.drot[k] = d_q[4 * i + k];
        g.dopacity = d_op[i];
        activate_raw_backward(a, g);
        for (int k = 0; k < 3; ++k) g_ls[3 * i + k] = g.dscale[k];
        for (int k = 0; k < 4; ++k) g_rq[4 * i + k] = g.drot[k];
        g_logit[i] = g.dopacity;
    }
}

// f1: one Adam step over n elements by the kernels' own rule (gsr_math.h adam_update, adam_step_size), with the scalars the host side
// of gsr_adam_step_multi derives (tests/training_ref.py adam_scalars).  row_len = 0: one step size, else columns below `split` take
// step_head and the others step_tail.
extern "C" void hh_adam_step(int64_t n, float *p, const float *g, float *m, float *v, float one_minus_b1, float b2, float one_minus_b2,
                             float eps, float step_head, float step_tail, float inv_bc2_sqrt, int32_t row_len, int32_t split)
{
    const AdamConsts c = {one_minus_b1, b2, one_minus_b2, eps};
    for (int64_t i = 0; i < n; ++i) {
        const float st = row_len ? adam_step_size((uint32_t)(i % row_len), (uint32_t)row_len, (uint32_t)split, step_head, step_tail, true) : step_head;
        adam_update(p[i], m[i], v[i], g[i], st, inv_bc2_sqrt, c);
    }
}

// ---- exact host reference of the progressive binning (tests/binning_ref.py).  Input: the device's own records, depth order and
// chunk plan.  For every chunk c and tile t: the Gaussians of chunk c whose rectangle holds t (inside the slab) and which
// tile_may_contribute accepts, in (binary32 depth key, index) order, each with the quadrant mask of the chunk's path (quadrant_mask_q
// for flat chunks, quadrant_mask_bbox for team / gather chunks).  The device contracts to FMA and this file is built without, so
// every decision also reports its margin: a decision closer to its cut-off than `tol` (relative to the magnitudes that enter it)
// is flagged, and the checker lets the device decide it either way.
#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr uint8_t kRefMaybe = 0x10;        // inclusion decided within tol of its cut-off
constexpr uint8_t kRefHostIn = 0x20;       // the host's own inclusion decision (entries flagged kRefMaybe may be host-rejected)

struct Decision { bool v; float margin; };     // margin: distance to the cut-off relative to the decision's magnitude

inline Decision rel(float diff, float scale) { return {diff >= 0.f, std::fabs(diff) / (scale > 0.f ? scale : 1.f)}; }
inline Decision lower(Decision a, Decision b) { return a.margin <= b.margin ? a : b; }

// tile_may_contribute (gsr_math.h) with the margin of the decision that settled it
Decision tmc_margin(float sx, float sy, float A, float B, float C, float op, int tx, int ty)
{
    const bool v = tile_may_contribute(sx, sy, A, B, C, op, tx, ty);
    const float amin = (float)GSR_ALPHA_MIN;
    float m = std::fabs(op - amin) / amin;
    if (op < amin) return {v, m};
    const float det = A * C - B * B;
    m = std::fmin(m, std::fabs(det) / (A * C + B * B + 1e-30f));
    if (!(A > 0.f) || !(C > 0.f) || !(det > 0.f)) return {v, m};
    const float dx0 = sx - (float)(tx * GSR_TILE + GSR_TILE - 1), dx1 = sx - (float)(tx * GSR_TILE);
    const float dy0 = sy - (float)(ty * GSR_TILE + GSR_TILE - 1), dy1 = sy - (float)(ty * GSR_TILE);
    if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) return {v, m};
    float qmax = -3.0e38f;
    for (int e = 0; e < 2; ++e) {
        const float ex = e ? dx1 : dx0;
        float dy = std::fmin(dy1, std::fmax(dy0, -B * ex / C));
        qmax = std::fmax(qmax, -0.5f * (A * ex * ex + C * dy * dy) - B * ex * dy);
        const float ey = e ? dy1 : dy0;
        float dx = std::fmin(dx1, std::fmax(dx0, -B * ey / A));
        qmax = std::fmax(qmax, -0.5f * (A * dx * dx + C * ey * ey) - B * dx * ey);
    }
    const float mx = std::fmax(std::fabs(dx0), std::fabs(dx1)), my = std::fmax(std::fabs(dy0), std::fabs(dy1));
    const float S = 0.5f * A * mx * mx + 0.5f * C * my * my + std::fabs(B) * mx * my;
    const float need = -logf(255.f * op);
    const Decision d = rel(qmax - (need - (0.01f + 1e-5f * S)), S + std::fabs(need) + 1.f);
    return {v, std::fmin(m, d.margin)};
}

// rect_may_contribute_q's margin (the quadrant decision of flat chunks)
float rmc_q_margin(float sx, float sy, float qA, float qB, float qC, float lop, float x0, float x1, float y0, float y1)
{
    const float kLog2AlphaMin = -7.994353437f;
    float m = std::fabs(lop - kLog2AlphaMin) / -kLog2AlphaMin;
    if (lop < kLog2AlphaMin) return m;
    const float det = 4.f * qA * qC - qB * qB;
    m = std::fmin(m, std::fabs(det) / (std::fabs(4.f * qA * qC) + qB * qB + 1e-30f));
    if (!(qA < 0.f) || !(qC < 0.f) || !(det > 0.f)) return m;
    const float dx0 = sx - x1, dx1 = sx - x0, dy0 = sy - y1, dy1 = sy - y0;
    if (dx0 <= 0.f && dx1 >= 0.f && dy0 <= 0.f && dy1 >= 0.f) return m;
    const float hC = -0.5f * qB / qC, hA = -0.5f * qB / qA;
    float qmax = -3.0e38f;
    for (int e = 0; e < 2; ++e) {
        const float ex = e ? dx1 : dx0;
        const float dy = std::fmin(dy1, std::fmax(dy0, hC * ex));
        qmax = std::fmax(qmax, (qA * ex + qB * dy) * ex + qC * dy * dy);
        const float ey = e ? dy1 : dy0;
        const float dx = std::fmin(dx1, std::fmax(dx0, hA * ey));
        qmax = std::fmax(qmax, (qC * ey + qB * dx) * ey + qA * dx * dx);
    }
    const float mx = std::fmax(std::fabs(dx0), std::fabs(dx1)), my = std::fmax(std::fabs(dy0), std::fabs(dy1));
    const float S = -qA * mx * mx - qC * my * my + std::fabs(qB) * mx * my;
    const float need = (kLog2AlphaMin - lop) - (0.0145f + 1e-5f * S);
    return std::fmin(m, rel(qmax - need, S + std::fabs(kLog2AlphaMin - lop) + 1.f).margin);
}

struct RefEntry { uint32_t tile, gid; uint8_t quad, flags; float margin; };

struct RefState {
    int n_chunks = 0, Tn = 0;
    std::vector<int64_t> offs;            // [n_chunks * Tn + 1]
    std::vector<RefEntry> entries;        // grouped by (chunk, tile)
    double max_margin_flagged = 0.0;
};
RefState g_ref;

}  // namespace

// Builds the reference (kept in this library until the next call).  rec: [P, 12] device records; order: the depth order;
// rank_begin[n_chunks + 1]; bbox[c] != 0: chunk c takes quadrant_mask_bbox.  Returns the number of entries (flagged ones included).
extern "C" int64_t hh_bin_reference(int Gx, int Gy, int ty0, int ty1, int P, const float *rec, const int32_t *order, int n_chunks,
                                    const int32_t *rank_begin, const uint8_t *bbox, float tol)
{
    const int Tn = Gx * Gy;
    g_ref = RefState();
    g_ref.n_chunks = n_chunks; g_ref.Tn = Tn;
    std::vector<RefEntry> all;
    std::vector<int64_t> cnt((size_t)n_chunks * Tn + 1, 0);
    std::vector<uint32_t> members;
    for (int c = 0; c < n_chunks; ++c) {
        members.assign(order + rank_begin[c], order + rank_begin[c + 1]);
        auto key = [&](uint32_t g) { uint32_t k; std::memcpy(&k, rec + 12 * (size_t)g + 9, 4); return k; };
        std::sort(members.begin(), members.end(), [&](uint32_t a, uint32_t b) {
            const uint32_t ka = key(a), kb = key(b);
            return ka != kb ? ka < kb : a < b;
        });
        for (uint32_t g : members) {
            if ((int)g < 0 || (int)g >= P) continue;
            const float *r = rec + 12 * (size_t)g;
            uint32_t rx, ry;
            std::memcpy(&rx, r + 10, 4); std::memcpy(&ry, r + 11, 4);
            const int x0 = (int)(rx & 0xFFFFu), x1 = (int)(rx >> 16), y0 = std::max((int)(ry & 0xFFFFu), ty0), y1 = std::min((int)(ry >> 16), ty1);
            float A, B, Cc, op;
            unscale_conic(r[2], r[3], r[4], r[5], A, B, Cc, op);
            float xe = 0.f, ye = 0.f;
            if (bbox[c]) splat_extent_q(r[2], r[3], r[4], r[5], xe, ye);
            for (int ty = y0; ty < y1; ++ty)
                for (int tx = x0; tx < x1 && tx < Gx; ++tx) {
                    const Decision d = tmc_margin(r[0], r[1], A, B, Cc, op, tx, ty);
                    const bool maybe = d.margin <= tol;
                    if (!d.v && !maybe) continue;
                    RefEntry e;
                    e.tile = (uint32_t)(ty * Gx + tx); e.gid = g; e.flags = (uint8_t)((maybe ? kRefMaybe : 0) | (d.v ? kRefHostIn : 0));
                    e.margin = d.margin;
                    const float px0 = (float)(tx * GSR_TILE), py0 = (float)(ty * GSR_TILE);
                    if (bbox[c]) {
                        e.quad = (uint8_t)quadrant_mask_bbox(r[0], r[1], xe, ye, px0, py0);
                        // the four compares of each axis: a bound within tol of a quadrant edge may go either way
                        const float h = (float)(GSR_TILE / 2), sx = r[0], sy = r[1];
                        const float ex[4] = {sx - xe - (px0 + h - 1.f), sx + xe - px0, sx - xe - (px0 + 2.f * h - 1.f), sx + xe - (px0 + h)};
                        const float ey[4] = {sy - ye - (py0 + h - 1.f), sy + ye - py0, sy - ye - (py0 + 2.f * h - 1.f), sy + ye - (py0 + h)};
                        const float sxs = std::fabs(sx) + std::fabs(xe) + 16.f, sys = std::fabs(sy) + std::fabs(ye) + 16.f;
                        unsigned ux = 0, uy = 0;
                        for (int i = 0; i < 4; ++i) {
                            if (std::fabs(ex[i]) <= tol * sxs) ux |= i < 2 ? 1u : 2u;
                            if (std::fabs(ey[i]) <= tol * sys) uy |= i < 2 ? 1u : 2u;
                        }
                        const float L = (r[5] + 7.994353437f) * 1.001f + 0.02f, det = 4.f * r[2] * r[4] - r[3] * r[3];
                        const bool shaky = std::fabs(L) <= tol * 8.f || std::fabs(det) <= tol * (std::fabs(4.f * r[2] * r[4]) + r[3] * r[3]);
                        unsigned u = 0;
                        for (int k = 0; k < 4; ++k)
                            if (shaky || ((ux >> (k & 1)) & 1u) || ((uy >> (k >> 1)) & 1u)) u |= 1u << k;
                        e.flags |= (uint8_t)u;
                    } else {
                        e.quad = (uint8_t)quadrant_mask_q(r[0], r[1], r[2], r[3], r[4], r[5], px0, py0);
                        for (int k = 0; k < 4; ++k) {
                            const float qx0 = px0 + (float)((k & 1) * (GSR_TILE / 2)), qy0 = py0 + (float)((k >> 1) * (GSR_TILE / 2));
                            if (rmc_q_margin(r[0], r[1], r[2], r[3], r[4], r[5], qx0, qx0 + (float)(GSR_TILE / 2 - 1), qy0,
                                             qy0 + (float)(GSR_TILE / 2 - 1)) <= tol)
                                e.flags |= (uint8_t)(1u << k);
                        }
                    }
                    all.push_back(e);
                    ++cnt[(size_t)c * Tn + e.tile + 1];
                }
        }
    }
    for (size_t i = 1; i < cnt.size(); ++i) cnt[i] += cnt[i - 1];      // stable counting sort by (chunk, tile): depth order stays
    g_ref.offs = cnt;
    g_ref.entries.resize(all.size());
    std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
    size_t i = 0;
    for (int c = 0; c < n_chunks; ++c) {
        const size_t end = (size_t)(cnt[(size_t)(c + 1) * Tn]);
        for (; i < end; ++i) g_ref.entries[pos[(size_t)c * Tn + all[i].tile]++] = all[i];
    }
    return (int64_t)all.size();
}

// copies the reference out: offs[n_chunks * Tn + 1], gid / quad / flags / margin per entry
extern "C" void hh_bin_reference_get(int64_t *offs, uint32_t *gid, uint8_t *quad, uint8_t *flags, float *margin)
{
    std::memcpy(offs, g_ref.offs.data(), g_ref.offs.size() * sizeof(int64_t));
    for (size_t i = 0; i < g_ref.entries.size(); ++i) {
        const RefEntry &e = g_ref.entries[i];
        gid[i] = e.gid; quad[i] = e.quad; flags[i] = e.flags; margin[i] = e.margin;
    }
}

// Compares device lists with the reference held by hh_bin_reference.
//   ranges[n_chunks][Tn] (begin, end) into words[n_words] (Gaussian | quadrant mask << 28); slab tiles [t_begin, t_end);
//   last_chunk[Tn]: the largest chunk that holds the last contributor of a pixel of the tile (-1: none).
// stats (int64[12]): 0 entries compared, 1 list faults, 2 quadrant faults, 3 range faults, 4 closed-tile faults,
//   5 boundary mismatches (inclusion), 6 boundary mismatches (quadrant bits), 7 closed tiles, 8 lists compared, 9 emitted total,
//   10 first faulty chunk * Tn + tile (-1: none), 11 fault kind of that one (1 list, 2 quad, 3 range, 4 closed).
// *max_margin: the largest margin among the boundary mismatches.
extern "C" void hh_bin_check(const uint32_t *ranges, const uint32_t *words, int64_t n_words, int t_begin, int t_end,
                             const int32_t *last_chunk, int64_t *stats, float *max_margin)
{
    const int n_chunks = g_ref.n_chunks, Tn = g_ref.Tn;
    for (int i = 0; i < 12; ++i) stats[i] = 0;
    stats[10] = -1;
    *max_margin = 0.f;
    auto fault = [&](int kind, int c, int t) {
        stats[kind] += 1;
        if (stats[10] < 0) { stats[10] = (int64_t)c * Tn + t; stats[11] = kind; }
    };
    std::vector<int> closed_at(Tn, -1);
    int64_t base = -1;                                   // start of chunk c's segment: where chunk c - 1 ended
    for (int c = 0; c < n_chunks; ++c) {
        const uint32_t *rc = ranges + (size_t)c * Tn * 2;
        int64_t cursor = base;
        for (int t = 0; t < Tn; ++t) {
            const int64_t a = rc[2 * t], b = rc[2 * t + 1];
            if (t < t_begin || t >= t_end) { if (a != b) fault(3, c, t); continue; }
            if (b < a || b > n_words) { fault(3, c, t); continue; }
            if (b > a) {                                 // ranges follow tile order, back to back (both the sort and the gather)
                if (cursor < 0) cursor = a;
                if (a != cursor) fault(3, c, t);
                cursor = b;
            }
        }
        // a chunk's segment starts where the previous one ended (chunk 0's at 0)
        if (cursor >= 0) {
            int64_t first = -1;
            for (int t = t_begin; t < t_end && first < 0; ++t) if (rc[2 * t + 1] > rc[2 * t]) first = rc[2 * t];
            if (base >= 0 && first != base) fault(3, c, 0);
            if (c == 0 && first != 0) fault(3, c, 0);
            base = cursor;
        }
        stats[9] = base < 0 ? 0 : base;
        for (int t = t_begin; t < t_end; ++t) {
            const int64_t a = rc[2 * t], b = rc[2 * t + 1];
            if (b < a || b > n_words) continue;
            const int64_t e0 = g_ref.offs[(size_t)c * Tn + t], e1 = g_ref.offs[(size_t)c * Tn + t + 1];
            bool definite = false;
            for (int64_t i = e0; i < e1; ++i) definite |= !(g_ref.entries[i].flags & kRefMaybe);
            if (a == b) {                                // empty: a closed tile, or nothing (definite) to take
                if (definite) {
                    if (c == 0) fault(4, c, t);
                    if (closed_at[t] < 0) {
                        closed_at[t] = c; ++stats[7];
                        if (last_chunk && last_chunk[t] >= c) fault(4, c, t);
                    }
                }
                continue;
            }
            ++stats[8];
            if (closed_at[t] >= 0) { fault(4, c, t); continue; }      // closing is for good
            int64_t i = e0, j = a;
            bool bad = false;
            while (j < b) {
                const uint32_t w = words[j], g = w & 0x0FFFFFFFu, q = w >> 28;
                if (i < e1 && g_ref.entries[i].gid == g) {
                    const RefEntry &e = g_ref.entries[i];
                    if (!(e.flags & kRefHostIn)) { ++stats[5]; *max_margin = std::fmax(*max_margin, e.margin); }
                    const unsigned diff = (q ^ e.quad) & 0xFu;
                    if (diff & ~(unsigned)(e.flags & 0xFu)) fault(2, c, t);
                    else if (diff) ++stats[6];
                    ++stats[0]; ++i; ++j;
                } else if (i < e1 && (g_ref.entries[i].flags & kRefMaybe)) {
                    if (g_ref.entries[i].flags & kRefHostIn) { ++stats[5]; *max_margin = std::fmax(*max_margin, g_ref.entries[i].margin); }
                    ++i;
                } else { bad = true; break; }
            }
            for (; !bad && i < e1; ++i) {
                if (!(g_ref.entries[i].flags & kRefMaybe)) bad = true;
                else if (g_ref.entries[i].flags & kRefHostIn) { ++stats[5]; *max_margin = std::fmax(*max_margin, g_ref.entries[i].margin); }
            }
            if (bad) fault(1, c, t);
        }
    }
}
