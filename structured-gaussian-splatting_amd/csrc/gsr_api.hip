// gsr_api.hip — the extern "C" entry points of libgsrast.so (include/gsrast.h).
// Host-side only: argument validation, workspace carving, kernel sequencing on the caller's stream.
#include <stdarg.h>
#include <string.h>

#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "gsr_internal.h"

namespace gsr {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// ---- per-kernel timing: process-wide (the backward runs on the autograd worker thread) list of
// (name, start, stop) event pairs behind a mutex; events pooled.  Opt-in, off by default.
struct ProfEntry { char name[GSR_PROFILE_NAME_LEN]; hipEvent_t a, b; };
struct ProfState {
    bool on = false;
    std::vector<ProfEntry> pending;
    std::vector<hipEvent_t> pool;
    struct Acc { char name[GSR_PROFILE_NAME_LEN]; double ms; int n; };
    std::vector<Acc> acc;
};
static ProfState g_prof;
static std::mutex g_prof_mu;

bool profile_on() { return g_prof.on; }

static hipEvent_t prof_event()
{
    if (!g_prof.pool.empty()) { hipEvent_t e = g_prof.pool.back(); g_prof.pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int profile_begin(const char *name, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    ProfEntry e;
    strncpy(e.name, name, GSR_PROFILE_NAME_LEN - 1);
    e.name[GSR_PROFILE_NAME_LEN - 1] = 0;
    e.a = prof_event(); e.b = prof_event();
    (void)hipEventRecord(e.a, s);
    g_prof.pending.push_back(e);
    return (int)g_prof.pending.size() - 1;
}

void profile_end(int idx, hipStream_t s)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    if (idx >= 0 && idx < (int)g_prof.pending.size()) (void)hipEventRecord(g_prof.pending[idx].b, s);
}

static void profile_drain()
{
    for (auto &e : g_prof.pending) {
        float ms = 0.f;
        if (hipEventSynchronize(e.b) == hipSuccess && hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
            bool found = false;
            for (auto &a : g_prof.acc)
                if (!strcmp(a.name, e.name)) { a.ms += ms; a.n += 1; found = true; break; }
            if (!found) { ProfState::Acc a; strcpy(a.name, e.name); a.ms = ms; a.n = 1; g_prof.acc.push_back(a); }
        }
        g_prof.pool.push_back(e.a); g_prof.pool.push_back(e.b);
    }
    g_prof.pending.clear();
}

static int validate(const gsr_frame_desc *d)
{
    if (!d) { set_error("frame descriptor is NULL"); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->P >= (1 << kQuadMaskShift)) {
        set_error("P = %d: at most 2^%d - 1 Gaussians per frame (the sorted instance list packs a 4-bit quadrant mask above the index)",
                  d->P, kQuadMaskShift);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (d->P < 0 || d->width <= 0 || d->height <= 0) {
        set_error("bad frame: P=%d width=%d height=%d", d->P, d->width, d->height);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (((long long)(d->width + GSR_TILE - 1) / GSR_TILE) * ((long long)(d->height + GSR_TILE - 1) / GSR_TILE) >= (1ll << kUnitTileBits)) {
        set_error("%d x %d pixels: at most 2^%d - 1 tiles per frame (the blend backward's work units pack the tile index)", d->width,
                  d->height, kUnitTileBits);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (d->sh_degree < 0 || d->sh_degree > 3) { set_error("sh_degree %d outside 0..3", d->sh_degree); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->sh_coeffs < 0 || d->sh_coeffs > 16) { set_error("sh_coeffs %d outside 0..16", d->sh_coeffs); return GSR_ERR_INVALID_ARGUMENT; }
    if (!(d->tanfovx > 0.f) || !(d->tanfovy > 0.f)) { set_error("tanfov must be positive"); return GSR_ERR_INVALID_ARGUMENT; }
    return GSR_OK;
}

static int validate_inputs(const gsr_frame_desc *d, const gsr_camera *c, const gsr_gaussians *g)
{
    if (!c || !c->bg || !c->viewmatrix || !c->projmatrix || !c->campos) { set_error("camera tensors missing"); return GSR_ERR_INVALID_ARGUMENT; }
    if (!g) { set_error("gaussians missing"); return GSR_ERR_INVALID_ARGUMENT; }
    if (d->P == 0) return GSR_OK;
    if (!g->means3D || !g->opacities) { set_error("means3D / opacities missing"); return GSR_ERR_INVALID_ARGUMENT; }
    if (g->raw) {
        // raw-parameter mode (a14): log-scales, raw quaternions, opacity logits; SH as _features_dc + _features_rest (raw == 1) or
        // as one interleaved table (raw == 2)
        const bool common = g->shs && g->scales && g->rotations && !g->colors_precomp && !g->cov3D_precomp && d->sh_coeffs >= 1;
        if (g->raw == 1 && (!common || ((g->shs_rest == nullptr) != (d->sh_coeffs == 1)))) {
            set_error("raw mode needs shs (features_dc), shs_rest (features_rest, NULL iff sh_coeffs == 1), scales and rotations, "
                      "and neither colors_precomp nor cov3D_precomp");
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (g->raw == 2 && (!common || g->shs_rest)) {
            set_error("raw mode 2 needs shs (the interleaved [P,sh_coeffs,3] table), no shs_rest, scales and rotations, and neither "
                      "colors_precomp nor cov3D_precomp");
            return GSR_ERR_INVALID_ARGUMENT;
        }
        if (g->raw != 1 && g->raw != 2) { set_error("raw must be 0, 1 or 2"); return GSR_ERR_INVALID_ARGUMENT; }
    } else if (g->shs_rest) {
        set_error("shs_rest is only meaningful with raw != 0");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((g->shs == nullptr) == (g->colors_precomp == nullptr)) {
        set_error("provide exactly one of shs / colors_precomp");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const bool sr = g->scales && g->rotations;
    if (sr == (g->cov3D_precomp != nullptr) || (!sr && (g->scales || g->rotations))) {
        set_error("provide exactly one of (scales, rotations) / cov3D_precomp");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (g->shs && (d->sh_degree + 1) * (d->sh_degree + 1) > d->sh_coeffs) {
        set_error("active SH degree %d needs %d coefficients, shs holds %d", d->sh_degree,
                  (d->sh_degree + 1) * (d->sh_degree + 1), d->sh_coeffs);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

// Control-block readback: the two host decisions of a frame (R / chunk plan, open-tile count) wait for 250 bytes.  The kernel
// in front of each decision (k_open_count) writes the block straight into host-coherent pinned memory and releases a sequence
// number behind it (CtrlMirror); the host polls that word.  (Round 1 copied the block with hipMemcpyAsync and polled an event:
// the copy is a 5 us kernel of its own and the event another packet, both on the critical path of a 0.8 ms step.)  A frame
// whose geometry workspace is absent, or a stream that drains without the word arriving, falls back to the copy.
constexpr double kReadbackTimeoutS = 30.0;

// the one reader of the environment (gsr_internal.h Switches): the experiments when the library is loaded, the test hooks per call
static const Switches g_loaded = {getenv("GSR_NO_LIVE_FILTER") != nullptr, getenv("GSR_NO_CHUNK_MERGE") != nullptr,
                                  getenv("GSR_NO_GATHER") != nullptr, getenv("GSR_FWD_GROUPS") ? atoi(getenv("GSR_FWD_GROUPS")) : -1,
                                  false, false};
Switches switches()
{
    Switches sw = g_loaded;
    sw.sort_force_radix = getenv("GSR_SORT_FORCE_RADIX") != nullptr;
    sw.reduce_rows_plain = getenv("GSR_REDUCE_ROWS_PLAIN") != nullptr;
    return sw;
}

static inline void cpu_pause()
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#elif defined(__aarch64__)
    asm volatile("yield");
#endif
}

struct Readback {            // one per host thread, never freed (pinned words + an event; the HIP runtime may already be gone
    uint32_t *words = nullptr;   // when thread-local destructors run).  words: Ctrl, then the sequence word
    uint32_t *words_dev = nullptr;
    uint32_t seq = 0;
    hipEvent_t ev = nullptr;
};
static thread_local Readback tl_readback;
constexpr int kCtrlWords = (int)(sizeof(Ctrl) / 4);

static int readback_init(Readback &rb)
{
    if (rb.words) return GSR_OK;
    void *p = nullptr;
    GSR_HIP_CHECK(hipHostMalloc(&p, sizeof(Ctrl) + 64, hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent));
    memset(p, 0, sizeof(Ctrl) + 64);
    void *d = nullptr;
    GSR_HIP_CHECK(hipHostGetDevicePointer(&d, p, 0));
    GSR_HIP_CHECK(hipEventCreateWithFlags(&rb.ev, hipEventDisableTiming));
    rb.words = static_cast<uint32_t *>(p);
    rb.words_dev = static_cast<uint32_t *>(d);
    return GSR_OK;
}

// the mirror to hand to the kernel in front of the next wait_ctrl() of this thread
static int next_mirror(CtrlMirror *m)
{
    Readback &rb = tl_readback;
    int rc = readback_init(rb);
    if (rc) return rc;
    if (++rb.seq == 0) rb.seq = 1;
    m->words = rb.words_dev; m->seq = rb.seq;
    return GSR_OK;
}

static int read_ctrl_by_copy(const Ctrl *dev, Ctrl *out, hipStream_t s)
{
    Readback &rb = tl_readback;
    int rc = readback_init(rb);
    if (rc) return rc;
    GSR_HIP_CHECK(hipMemcpyAsync(rb.words, dev, sizeof(Ctrl), hipMemcpyDeviceToHost, s));
    GSR_HIP_CHECK(hipStreamSynchronize(s));
    memcpy(out, rb.words, sizeof(Ctrl));
    return GSR_OK;
}

// Wait for the block the kernel given next_mirror()'s mirror publishes.  Polls, politely and not for ever: a few thousand
// loads back to back (the word normally lands within microseconds of the kernel's end), then with a pause instruction, now and
// then a look at the stream (an error, or a drained stream without the word, ends the wait), and after kReadbackTimeoutS an
// error instead of hanging the host on a wedged stream.
static int wait_ctrl(const Ctrl *dev, Ctrl *out, hipStream_t s)
{
    Readback &rb = tl_readback;
    const uint32_t want = rb.seq;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long long spins = 0;; ++spins) {
        if (__atomic_load_n(&rb.words[kCtrlWords], __ATOMIC_ACQUIRE) == want) break;
        if (spins > 4096) {
            cpu_pause();
            if ((spins & 4095) == 0) {
                const hipError_t e = hipStreamQuery(s);
                if (e == hipSuccess) {                               // drained: the word is there now, or it is not coming
                    if (__atomic_load_n(&rb.words[kCtrlWords], __ATOMIC_ACQUIRE) == want) break;
                    return read_ctrl_by_copy(dev, out, s);
                }
                if (e != hipErrorNotReady) { set_error("control-block readback: %s", hipGetErrorString(e)); return GSR_ERR_HIP; }
                if (spins > (1ull << 20)) std::this_thread::yield();         // a long wait (debugger, huge frame): give the core away
                const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (waited > kReadbackTimeoutS) {
                    set_error("control-block readback did not complete within %.0f s: the stream is stuck (a kernel of this frame "
                              "hangs or the device was lost)", kReadbackTimeoutS);
                    return GSR_ERR_HIP;
                }
            }
        }
    }
    memcpy(out, rb.words, sizeof(Ctrl));
    return GSR_OK;
}

}  // namespace gsr

using namespace gsr;

extern "C" {

int gsr_version(void) { return GSR_VERSION; }

const char *gsr_last_error(void) { return g_err; }

int gsr_workspace_sizes(const gsr_frame_desc *desc, size_t *geom_bytes, size_t *image_bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    const FrameK f = make_frame(*desc);
    if (geom_bytes) *geom_bytes = carve_geom(nullptr, f.P).total;
    if (image_bytes) *image_bytes = carve_image(nullptr, f).total;
    return GSR_OK;
}

int gsr_binning_size(const gsr_frame_desc *desc, int64_t num_rendered, size_t *binning_bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (num_rendered < 0 || !binning_bytes) { set_error("bad num_rendered / NULL out"); return GSR_ERR_INVALID_ARGUMENT; }
    *binning_bytes = carve_binning(nullptr, num_rendered, make_frame(*desc)).total;
    return GSR_OK;
}

int gsr_binning_first_chunk_capacity(const gsr_frame_plan *plan, int64_t *instances)
{
    if (!plan || !instances) { set_error("gsr_binning_first_chunk_capacity: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    *instances = first_chunk_capacity(*plan);
    return GSR_OK;
}

int gsr_forward_preprocess(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws,
                           void *image_ws, int32_t *radii, gsr_frame_plan *plan, void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if ((rc = validate_inputs(desc, cam, g))) return rc;
    if (!plan || (desc->P > 0 && (!geom_ws || !radii))) { set_error("NULL output"); return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    const bool dbg = desc->debug != 0;
    const FrameK f = make_frame(*desc);
    memset(plan, 0, sizeof *plan);
    plan->num_chunks = 1;
    if (f.P == 0) return GSR_OK;
    GeomWS gw = carve_geom(geom_ws, f.P);
    // (the selection's histograms are cleared by the preprocess kernel, the tile ranges by the partition's scatter kernel)
    if ((rc = launch_preprocess(f, *cam, *g, gw, radii, desc->prefiltered != 0, dbg, s))) return rc;
    if (image_ws) {                                  // stage 2's reset of ranges / open flags, in the shadow of the readback
        ImageWS iw = carve_image(image_ws, f);
        if ((rc = launch_depth_select(f, gw, dbg, s, iw.ranges, binning_clear_bytes(iw) / 16))) return rc;      // chunk plan + partition by chunk
        CtrlMirror mirror;
        if ((rc = next_mirror(&mirror))) return rc;
        if ((rc = launch_binning_init(f, gw, iw, dbg, s, true, mirror))) return rc;
        plan->binning_initialised = 1;
    } else if ((rc = launch_depth_select(f, gw, dbg, s))) return rc;
    // The one host synchronisation of this stage: the plan (R sizes the binning workspace).
    Ctrl h;
    if ((rc = image_ws ? wait_ctrl(gw.ctrl, &h, s) : read_ctrl_by_copy(gw.ctrl, &h, s))) return rc;
    if (desc->prefiltered && h.prefilter_violation) {
        set_error("prefiltered is set but at least one Gaussian fails the frustum test (view depth <= 0.2): the caller's "
                  "pre-filter and the rasterizer disagree");
        return GSR_ERR_PREFILTERED;
    }
    if (h.overflow) {
        set_error("the frame's tile instances (sum of tiles touched over %d visible Gaussians) exceed 2^32 - 1: "
                  "split the frame into tile-row slabs (gsr_frame_desc.tile_row_begin/end)", (int)h.V);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    plan->num_rendered = (int64_t)h.R_total;
    plan->num_visible = (int32_t)h.V;
    plan->num_chunks = h.num_chunks > 0 ? (int32_t)h.num_chunks : 1;
    for (int c = 0; c <= GSR_MAX_CHUNKS; ++c) plan->chunk_rank_begin[c] = (int32_t)h.bnd[c];
    for (int c = 0; c < GSR_MAX_CHUNKS; ++c) plan->chunk_instances_max[c] = (int64_t)h.chunk_full[c];
    for (int c = 0; c < GSR_MAX_CHUNKS; ++c) plan->chunk_key_end[c] = h.key_end[c];
    plan->key_max = h.key_max;
    if (h.num_chunks == 0)
        for (int c = 0; c <= GSR_MAX_CHUNKS; ++c) plan->chunk_rank_begin[c] = 0;
    return GSR_OK;
}

// What the _contrib and _contrib_error calls ask of their arguments beyond the plain calls (stats and err NULL: nothing), checked on the
// host alone.  who: the _contrib entry point; with err it is the _contrib_error one
static int validate_contrib(const gsr_frame_desc *desc, const gsr_contrib_stats *stats, const gsr_contrib_error *err, const char *who)
{
    int rc = validate(desc);
    if (rc || (!stats && !err)) return rc;
    const char *sfx = err ? "_error" : "";
    if (!stats) {
        set_error("%s%s: err without stats: the error-weighted total is taken beside the blend statistics (stats is required)", who, sfx);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const FrameK f = make_frame(*desc);
    if (f.ty0 != 0 || f.ty1 != f.Gy) {
        set_error("%s%s: the %s statistics are taken over whole images only (tile_row_begin = tile_row_end = 0)", who, sfx,
                  err ? "error-weighted" : "blend");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (desc->P > 0 && err && !err->pixel_error) {
        set_error("%s%s: err->pixel_error is required ([H*W])", who, sfx);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (desc->P > 0 && err && !err->error_frame_q32) {
        set_error("%s%s: err->error_frame_q32 is required ([P])", who, sfx);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (desc->P > 0 && (!stats->count || !stats->weight_sum_q32 || !stats->weight_max_bits)) {
        set_error("%s%s: stats->count, ->weight_sum_q32 and ->weight_max_bits are required ([P] each)", who, sfx);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

// The aux workspace of a frame: the caller's maps, and the checkpoints carved from its ckpt_ws (binned = false: the frame has no list
// entries, the checkpoints are never touched)
static AuxWS aux_workspace(const gsr_aux_outputs *aux_out, bool binned, int64_t capacity, const FrameK &f, int planes = 1)
{
    AuxWS ax = carve_aux(aux_out && binned ? aux_out->ckpt_ws : nullptr, capacity, f, planes);
    if (aux_out) { ax.depth = aux_out->depth; ax.alpha = aux_out->alpha; }
    return ax;
}

// The variant of a frame as the _aux, _contrib and _contrib_error entry points receive it (FwdVariant once the aux workspace is carved)
// extra / extra_map (gsr_forward_extra: `ext` set, with aux): the table and the map of the three extra channels
struct FwdArgs {
    const gsr_aux_outputs *aux = nullptr; const gsr_contrib_stats *stats = nullptr; const gsr_contrib_error *err = nullptr;
    bool ext = false; const float *extra = nullptr; float *extra_map = nullptr;
    bool med = false; float *median = nullptr; int32_t *median_enc = nullptr;      // (gsr_forward_median: `med` set, with aux, without ext)
};

// A median frame's arguments (include/gsrast_median.h): refused with a message before anything is launched
static int validate_median(const gsr_frame_desc *desc, const gsr_aux_outputs *aux, const void *median, const int32_t *median_enc, bool backward,
                           const char *who)
{
    if (!desc) { set_error("%s: NULL frame description", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!aux) { set_error("%s: aux is required (a median frame is an aux frame: depth, alpha and ckpt_ws)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!backward && !median) { set_error("%s: median is NULL ([H,W] float)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!median_enc) { set_error("%s: median_enc is NULL ([H,W] int32)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if ((((uintptr_t)median | (uintptr_t)median_enc) & 3u) != 0) { set_error("%s: median / median_enc are not 4-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!median_frame_allowed(true, false, false, desc->tile_row_begin == 0 && desc->tile_row_end <= 0)) {
        set_error("%s: whole images only (tile_row_begin = tile_row_end = 0)", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

// An extra frame's arguments (include/gsrast_extra.h): refused with a message before anything is launched
static int validate_extra(const gsr_frame_desc *desc, const gsr_aux_outputs *aux, const float *extra, const float *extra_map, const char *who)
{
    if (!desc) { set_error("%s: NULL frame description", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!aux) { set_error("%s: aux is required (an extra frame is an aux frame: depth, alpha and a four-plane ckpt_ws)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->P > 0 && !extra) { set_error("%s: the extra table is NULL ([P] rows of four floats)", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (((uintptr_t)extra & 15u) != 0) { set_error("%s: the extra table is not 16-byte aligned", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (!extra_map) { set_error("%s: extra_map is NULL ([3,H,W])", who); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->tile_row_begin != 0 || desc->tile_row_end > 0) {
        set_error("%s: whole images only (tile_row_begin = tile_row_end = 0)", who);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return GSR_OK;
}

// fill (optional): a zero fill to enqueue behind the FIRST chunk's blend and readback kernels, ahead of the wait for that readback
// (gsr_forward's early fill); *fill_done reports whether it was enqueued
static int forward_render_impl(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                               void *image_ws, gsr_frame_plan *plan, float *out_color, void *stream, const ZeroSegs *fill, bool *fill_done,
                               const FwdArgs &v)
{
    int rc = validate_contrib(desc, v.stats, v.err, "gsr_forward_render_contrib");
    if (rc) return rc;
    if (v.ext && (rc = validate_extra(desc, v.aux, v.extra, v.extra_map, "gsr_forward_render_extra"))) return rc;
    if (v.med && (rc = validate_median(desc, v.aux, v.median, v.median_enc, false, "gsr_forward_render_median"))) return rc;
    if ((rc = validate_inputs(desc, cam, g))) return rc;
    if (!cam || !cam->bg || !image_ws || !out_color || !plan || plan->num_rendered < 0 ||
        (desc->P > 0 && !geom_ws) || (plan->num_rendered > 0 && !binning_ws)) {
        set_error("gsr_forward_render: NULL argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (plan->num_chunks < 1 || plan->num_chunks > GSR_MAX_CHUNKS) { set_error("bad plan (num_chunks %d)", plan->num_chunks); return GSR_ERR_INVALID_ARGUMENT; }
    hipStream_t s = (hipStream_t)stream;
    const bool dbg = desc->debug != 0;
    const FrameK f = make_frame(*desc);
    ImageWS iw = carve_image(image_ws, f);
    if (v.aux && (!v.aux->depth || !v.aux->alpha || (plan->num_rendered > 0 && !v.aux->ckpt_ws) || f.ty0 != 0 || f.ty1 != f.Gy)) {
        set_error("gsr_forward_render_aux: depth, alpha and (for a frame that bins anything) ckpt_ws are required; whole images only");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    plan->chunks_run = 0; plan->instances_emitted = 0; plan->sort_result = 0; plan->tile_order_ready = 0;
    if (f.P == 0 || plan->num_rendered == 0) {
        // nothing to bin: one blend pass over empty ranges writes the background
        GeomWS gw0 = carve_geom(geom_ws, f.P);
        BinningWS bw0 = carve_binning(binning_ws, 0, f);
        if (f.P == 0 || !geom_ws) gw0.ctrl = iw.ctrl_scratch;   // no geometry workspace at all
        if ((rc = launch_binning_init(f, gw0, iw, dbg, s))) return rc;
        const AuxWS ax0 = aux_workspace(v.aux, false, 0, f);
        const ExtWS ex0{reinterpret_cast<const float4 *>(v.extra), v.extra_map, nullptr, nullptr, nullptr};
        // (err is not handed on: nothing is blended, every error total is zero, and with P == 0 the caller may have passed no map -
        // the error kernel would load it at tile start whatever the ranges hold)
        const MedWS md0{v.median, v.median_enc, nullptr};
        if ((rc = launch_render_fwd(f, *cam, 0, true, 0, gw0, bw0, iw, out_color, dbg, s, false,
                                    {v.aux ? &ax0 : nullptr, v.stats, nullptr, v.ext ? &ex0 : nullptr, v.med ? &md0 : nullptr})))
            return rc;
        plan->chunks_run = 1;
        return GSR_OK;
    }
    GeomWS gw = carve_geom(geom_ws, f.P);
    // The binning workspace holds `binning_capacity` instances (0: the upper bound R, as the reference sizes its
    // binningBuffer).  A frame whose tiles saturate runs one small depth chunk and touches a few per cent of R, so
    // callers may size it for the first chunk only; a later chunk that does not fit stops the frame with
    // GSR_ERR_WORKSPACE before anything of that chunk is written (re-run this stage with a workspace for R instances).
    const int64_t capacity = plan_capacity(plan);
    BinningWS bw = carve_binning(binning_ws, capacity, f);
    const AuxWS ax = aux_workspace(v.aux, true, capacity, f, v.ext ? kExtCkptPlanes : 1);
    const ExtWS ex{reinterpret_cast<const float4 *>(v.extra), v.extra_map, nullptr, nullptr, nullptr};
    const MedWS md{v.median, v.median_enc, nullptr};
    const FwdVariant variant{v.aux ? &ax : nullptr, v.stats, v.err, v.ext ? &ex : nullptr, v.med ? &md : nullptr};
    if (!plan->binning_initialised && (rc = launch_binning_init(f, gw, iw, dbg, s))) return rc;
    plan->binning_initialised = 0;                  // a re-run of this stage must reset the tile ranges / open flags itself
    int sort_result = 0;
    const Switches sw = switches();
    const long long slab_tiles = (long long)(f.ty1 - f.ty0) * f.Gx;
    Progress now;                                   // what the chunks so far left behind (each readback below)
    // Early stop: one control-block readback per chunk (~10 us of stream idle, measured); the chunk plan keeps
    // the number of chunks at three or fewer.  Which path each step takes: gsr_dispatch.h.
    for (int c = 0; c < plan->num_chunks; ++c) {
        // plan step: a frame that is not going to close runs all remaining chunks as one
        LiveParts parts;
        uint64_t need = 0;
        if (merge_rest(plan, c, now, slab_tiles, capacity, !sw.no_live_filter && !sw.no_chunk_merge, &parts, &need) == Merge::kShort) {
            set_error("binning workspace holds %lld instances, the remaining depth chunks may need %llu: re-run "
                      "gsr_forward_render with binning_capacity = num_rendered (%lld)", (long long)capacity,
                      (unsigned long long)need, (long long)plan->num_rendered);
            return GSR_ERR_WORKSPACE;
        }
        const bool last = c == plan->num_chunks - 1;
        const int r0 = plan->chunk_rank_begin[c], r1 = plan->chunk_rank_begin[c + 1];
        const uint64_t chunk_n = (uint64_t)(r1 - r0), chunk_max = (uint64_t)plan->chunk_instances_max[c];
        // capacity check
        if (capacity_short(now.emitted, chunk_max, capacity)) {
            set_error("binning workspace holds %lld instances, depth chunk %d may need %llu: re-run gsr_forward_render with "
                      "binning_capacity = num_rendered (%lld)", (long long)capacity, c,
                      (unsigned long long)(now.emitted + chunk_max), (long long)plan->num_rendered);
            return GSR_ERR_WORKSPACE;
        }
        // filter, order: the chunk's Gaussians were selected by depth; now that it is needed, put them in (depth, index) order - a
        // late, large chunk only those that can still reach an open tile
        // (once: a re-run of this stage after GSR_ERR_WORKSPACE finds the earlier chunks sorted, and the sort's inputs consumed)
        const bool filtered = chunk_filtered(c, r1 - r0, chunk_max, now, slab_tiles, sw.no_live_filter);
        if (filtered) plan->chunks_filtered |= 1 << c;
        if (c >= plan->chunks_sorted) {
            if (filtered && (rc = launch_live_filter(f, c, r0, r1, parts, gw, iw, dbg, s))) return rc;
            // (the sort's key span: up to the chunk's end, and never beyond the frame's largest key — the last chunk's end is "everything")
            const uint32_t key_hi = plan->key_max != 0u && plan->key_max < plan->chunk_key_end[c] ? plan->key_max : plan->chunk_key_end[c];
            if ((rc = launch_chunk_order(f, r0, r1, c > 0 ? plan->chunk_key_end[c - 1] : 0u, key_hi, c == 0, gw, dbg, s,
                                         filtered ? &gw.ctrl->chunk_live[c] : nullptr)))
                return rc;
            plan->chunks_sorted = c + 1;
        }
        // bin, colours, blend.  From here on the PLAN's filtered bit decides, not the local one: a re-run of this stage after
        // GSR_ERR_WORKSPACE must take the decisions of the first run
        const bool plan_filtered = (plan->chunks_filtered >> c) & 1;
        if ((rc = launch_chunk_binning(f, c, r0, r1, chunk_max, now.emitted, gw, bw, iw, &sort_result, dbg, s, plan_filtered))) return rc;
        if ((rc = launch_chunk_colors(f, *cam, *g, r0, r1, plan->num_visible, gw, dbg, s))) return rc;      // A.6 for this chunk's Gaussians only
        const bool groups = sw.fwd_groups >= 0 ? sw.fwd_groups != 0 : small_splats(chunk_n, chunk_max, plan_filtered);
        if ((rc = launch_render_fwd(f, *cam, c, last, sort_result, gw, bw, iw, out_color, dbg, s, groups, variant))) return rc;
        plan->chunks_run = c + 1;
        plan->instances_emitted = -1;                 // the last chunk's count stays on the device
        if (last) break;
        // readback
        CtrlMirror mirror;
        if ((rc = next_mirror(&mirror))) return rc;
        if ((rc = launch_open_update(f, gw, iw, dbg, s, mirror))) return rc;
        if (fill) {                                   // behind the kernel that posts the readback, ahead of the wait for it
            ProfileScope prof("zero_outputs", s);
            if ((rc = launch_zero_segments(*fill, s))) return rc;
            *fill_done = true; fill = nullptr;
        }
        Ctrl h;
        if ((rc = wait_ctrl(gw.ctrl, &h, s))) return rc;
        plan->instances_emitted = (int64_t)h.chunk_base[c + 1];
        now = Progress{(uint64_t)h.chunk_base[c + 1], h.open_count, h.open_stuck};
        if (h.open_count == 0) break;
    }
    plan->sort_result = sort_result;
    return GSR_OK;
}

int gsr_forward_render(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                       void *image_ws, gsr_frame_plan *plan, float *out_color, void *stream)
{
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr, {});
}

static int forward_impl(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                        gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill, void *stream,
                        const FwdArgs &v)
{
    int rc = validate_contrib(desc, v.stats, v.err, "gsr_forward_contrib");      // (before stage 1: a refused call launches nothing)
    if (rc) return rc;
    if (v.ext && (rc = validate_extra(desc, v.aux, v.extra, v.extra_map, "gsr_forward_extra"))) return rc;
    if (v.med && (rc = validate_median(desc, v.aux, v.median, v.median_enc, false, "gsr_forward_median"))) return rc;
    if ((rc = gsr_forward_preprocess(desc, cam, g, geom_ws, image_ws, radii, plan, stream))) return rc;
    const int64_t need = first_chunk_capacity(*plan);
    if (plan->num_rendered > 0 && (!binning_ws || binning_capacity < need)) {
        set_error("gsr_forward: the binning workspace holds %lld instances, the first depth chunk may need %lld: allocate and call "
                  "gsr_forward_render", (long long)binning_capacity, (long long)need);
        return GSR_ERR_WORKSPACE;
    }
    plan->binning_capacity = binning_capacity < plan->num_rendered ? binning_capacity : plan->num_rendered;
    if (plan->binning_capacity <= 0) plan->binning_capacity = 0;
    // The early fill: the zeros of a depth-complex frame's gradient tensors + the blend backward's row flags, 50 us of HBM writes at
    // 1M Gaussians.  It is enqueued behind the first chunk's blend and the kernel that posts its readback, BEFORE the host waits, so that it
    // runs while the host is idle in the wait and then busy getting back to its caller and on to the next launch (~60 us in which the
    // GPU has nothing else to do).  For which frames: gsr_dispatch.h early_fill_before_wait; the others fill late, below.  (Measured and dropped: the
    // fill on a side stream beside the blend - the cross-queue waits cost more than it hid; the fill as the first job of every wave
    // of the blend forward - 17 us there instead of 47, but the gap after the readback was empty again: 0.694 ms per step, not 0.678.)
    const bool fill_wanted = early_fill && !early_fill->prezeroed && desc->P > 0 && plan->num_rendered > 0;
    const FrameK f = make_frame(*desc);
    ZeroSegs fill;
    fill.n = 0;
    bool filled = false;
    if (fill_wanted && early_fill_before_wait(*plan, desc->P)) {
        const long long cap = plan_capacity(plan);
        const BinningWS bw = carve_binning(binning_ws, cap, f);
        fill = zero_segments(f, *g, nullptr, *early_fill, bw.row_valid, row_flag_bytes(cap));
    }
    if ((rc = forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, fill.n > 0 ? &fill : nullptr, &filled, v)))
        return rc;
    if (fill_wanted && plan->chunks_run > 0 && effective_binned_ranks(*plan) * 4 < (long long)desc->P) {
        if (!filled) {
            const BinningWS bw = carve_binning(binning_ws, plan_capacity(plan), f);
            ProfileScope prof("zero_outputs", (hipStream_t)stream);
            if ((rc = launch_zero_outputs(f, *g, nullptr, *early_fill, (hipStream_t)stream, bw.row_valid, valid_bytes(plan)))) return rc;
        }
        early_fill->prezeroed = 1;
        plan->tile_order_ready = 1;                      // the fill also cleared the blend backward's row flags
    }
    return GSR_OK;
}

int gsr_forward(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill, void *stream)
{
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream, {});
}

int gsr_forward_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                    gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill,
                    const gsr_aux_outputs *aux, void *stream)
{
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream, {aux});
}

int gsr_forward_render_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                           void *image_ws, gsr_frame_plan *plan, float *out_color, const gsr_aux_outputs *aux, void *stream)
{
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr, {aux});
}

int gsr_forward_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                      gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill,
                      const gsr_aux_outputs *aux, const float *extra, float *extra_map, void *stream)
{
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream,
                        {aux, nullptr, nullptr, true, extra, extra_map});
}

int gsr_forward_render_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                             void *image_ws, gsr_frame_plan *plan, float *out_color, const gsr_aux_outputs *aux, const float *extra,
                             float *extra_map, void *stream)
{
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr,
                               {aux, nullptr, nullptr, true, extra, extra_map});
}

int gsr_forward_median(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                       gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill,
                       const gsr_aux_outputs *aux, float *median, int32_t *median_enc, void *stream)
{
    FwdArgs v{aux};
    v.med = true; v.median = median; v.median_enc = median_enc;
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream, v);
}

int gsr_forward_render_median(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                              void *image_ws, gsr_frame_plan *plan, float *out_color, const gsr_aux_outputs *aux, float *median,
                              int32_t *median_enc, void *stream)
{
    FwdArgs v{aux};
    v.med = true; v.median = median; v.median_enc = median_enc;
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr, v);
}

int gsr_extra_workspace_size(const gsr_frame_desc *desc, int64_t binning_capacity, size_t *bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (binning_capacity < 0 || !bytes) { set_error("gsr_extra_workspace_size: bad binning_capacity / NULL out"); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = carve_aux(nullptr, binning_capacity, make_frame(*desc), kExtCkptPlanes).total;
    return GSR_OK;
}

int gsr_forward_contrib(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws, int32_t *radii,
                        gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color, gsr_grads *early_fill,
                        const gsr_contrib_stats *stats, void *stream)
{
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream, {nullptr, stats});
}

int gsr_forward_render_contrib(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                               void *image_ws, gsr_frame_plan *plan, float *out_color, const gsr_contrib_stats *stats, void *stream)
{
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr, {nullptr, stats});
}

int gsr_forward_contrib_error(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *image_ws,
                              int32_t *radii, gsr_frame_plan *plan, void *binning_ws, int64_t binning_capacity, float *out_color,
                              gsr_grads *early_fill, const gsr_contrib_stats *stats, const gsr_contrib_error *err, void *stream)
{
    return forward_impl(desc, cam, g, geom_ws, image_ws, radii, plan, binning_ws, binning_capacity, out_color, early_fill, stream, {nullptr, stats, err});
}

int gsr_forward_render_contrib_error(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, void *geom_ws, void *binning_ws,
                                     void *image_ws, gsr_frame_plan *plan, float *out_color, const gsr_contrib_stats *stats,
                                     const gsr_contrib_error *err, void *stream)
{
    return forward_render_impl(desc, cam, g, geom_ws, binning_ws, image_ws, plan, out_color, stream, nullptr, nullptr, {nullptr, stats, err});
}

int gsr_contrib_error_fold(int64_t P, uint64_t *error_frame_q32, uint64_t *error_sum_q32, float *error_max, void *stream)
{
    if (P < 0) {
        set_error("gsr_contrib_error_fold: P = %lld", (long long)P);
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (P == 0) return GSR_OK;
    if (!error_frame_q32 || !error_sum_q32 || !error_max) {
        set_error("gsr_contrib_error_fold: error_frame_q32, error_sum_q32 and error_max are required ([P] each)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    return launch_contrib_error_fold((long long)P, error_frame_q32, error_sum_q32, error_max, false, (hipStream_t)stream);
}

int gsr_aux_workspace_size(const gsr_frame_desc *desc, int64_t binning_capacity, size_t *bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (binning_capacity < 0 || !bytes) { set_error("gsr_aux_workspace_size: bad binning_capacity / NULL out"); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = carve_aux(nullptr, binning_capacity, make_frame(*desc)).total;
    return GSR_OK;
}

int gsr_backward_rows_size(const gsr_frame_desc *desc, const gsr_frame_plan *plan, size_t *rows_bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!plan || !rows_bytes) { set_error("gsr_backward_rows_size: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    *rows_bytes = align_up((size_t)rows_bound(plan) * kRowFloats * sizeof(float));
    return GSR_OK;
}

int gsr_extra_rows_size(const gsr_frame_desc *desc, const gsr_frame_plan *plan, size_t *bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!plan || !bytes) { set_error("gsr_extra_rows_size: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = align_up((size_t)rows_bound(plan) * sizeof(float4));
    return GSR_OK;
}

int gsr_backward_prepare(const gsr_frame_desc *desc, const gsr_gaussians *g, gsr_frame_plan *plan, float *screen_grads,
                         gsr_grads *grads, void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!g || !plan || !grads) { set_error("gsr_backward_prepare: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->P == 0) return GSR_OK;
    const FrameK f = make_frame(*desc);
    ProfileScope prof("zero_outputs", (hipStream_t)stream);
    if ((rc = launch_zero_outputs(f, *g, screen_grads, *grads, (hipStream_t)stream))) return rc;
    if (screen_grads) plan->screen_prezeroed = 1;
    grads->prezeroed = 1;
    return GSR_OK;
}

int gsr_bwd_segment_entries(void) { return kSeg; }

static int backward_render_impl(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                                const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color,
                                const gsr_aux_outputs *aux_out, const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                                float *screen_grads, void *stream, BwdKind kind, const ExtWS *ext = nullptr, const MedWS *med = nullptr)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (kind == BwdKind::kMed && (rc = validate_median(desc, aux_out, nullptr, med->median_enc, true, "gsr_backward_render_median"))) return rc;
    if (kind == BwdKind::kExt) {
        if ((rc = validate_extra(desc, aux_out, (const float *)ext->table, ext->map, "gsr_backward_render_extra"))) return rc;
        if (desc->P > 0 && !ext->dL_dtable) { set_error("gsr_backward_render_extra: dL_dextra is NULL ([P,3])"); return GSR_ERR_INVALID_ARGUMENT; }
        if (plan && plan->num_rendered > 0 && !ext->rows) { set_error("gsr_backward_render_extra: extra_rows_ws is NULL (gsr_extra_rows_size bytes)"); return GSR_ERR_INVALID_ARGUMENT; }
    }
    if (kind == BwdKind::kAbs && (desc->tile_row_begin != 0 || desc->tile_row_end > 0)) {
        set_error("gsr_backward_render_abs: whole images only (tile_row_begin = tile_row_end = 0)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (aux_out && (!aux_out->depth || (plan && plan->num_rendered > 0 && !aux_out->ckpt_ws))) {
        set_error("gsr_backward_render_aux: aux->depth and (for a frame that binned anything) aux->ckpt_ws are required");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (!cam || !cam->bg || (!dL_dcolor && !aux_out) || !out_color || !plan || (desc->P > 0 && (!screen_grads || !geom_ws)) || !image_ws ||
        (plan->num_rendered > 0 && (!binning_ws || !rows_ws))) {
        set_error("gsr_backward_render: NULL argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    const bool dbg = desc->debug != 0;
    const FrameK f = make_frame(*desc);
    if (f.P == 0) return GSR_OK;
    if (kind == BwdKind::kExt && plan->num_rendered <= 0)      // no launch below touches it
        GSR_HIP_CHECK(hipMemsetAsync(ext->dL_dtable, 0, (size_t)f.P * 3 * sizeof(float), s));
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
    ImageWS iw = carve_image(const_cast<void *>(image_ws), f);
    BinningWS bw = carve_binning(binning_ws, plan_capacity(plan), f);
    bw.grad_rows = (float *)rows_ws;
    long long rows_upper = 0;
    for (int c = 0; c < plan->chunks_run && c < GSR_MAX_CHUNKS; ++c) rows_upper += plan->chunk_instances_max[c];
    if (plan->num_rendered > 0) {
        if (!plan->tile_order_ready) GSR_HIP_CHECK(hipMemsetAsync(bw.row_valid, 0, valid_bytes(plan), s));
        const long long rows_n = plan->instances_emitted >= 0 ? (long long)plan->instances_emitted : rows_upper;
        const AuxWS ax = aux_workspace(aux_out, true, plan_capacity(plan), f, kind == BwdKind::kExt ? kExtCkptPlanes : 1);
        if ((rc = launch_render_bwd(f, plan->chunks_run, plan->sort_result, rows_n, gw, bw, iw, out_color, dL_dcolor, dbg, s,
                                    {kind, &ax, dL_ddepth, dL_dalpha, ext, med})))
            return rc;
    }
    if (kind == BwdKind::kMed) {      // (kMedianReducesAsAux: the rows are the aux backward's)
        static_assert(kMedianReducesAsAux, "a median frame's rows are reduced by the aux instantiation");
        return launch_reduce_rows(f, *plan, gw, bw, screen_grads, plan->screen_prezeroed, dbg, s, BwdKind::kAux);
    }
    // only the depth ranks of chunks that ran can own gradient rows
    if (kind == BwdKind::kExt && plan->num_rendered <= 0) return launch_reduce_rows(f, *plan, gw, bw, screen_grads, plan->screen_prezeroed, dbg, s, BwdKind::kAux);
    return launch_reduce_rows(f, *plan, gw, bw, screen_grads, plan->screen_prezeroed, dbg, s, kind, ext);
}

int gsr_backward_render(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                        const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color, const float *dL_dcolor,
                        float *screen_grads, void *stream)
{
    return backward_render_impl(desc, cam, geom_ws, binning_ws, image_ws, rows_ws, plan, out_color, nullptr, dL_dcolor, nullptr, nullptr,
                                screen_grads, stream, BwdKind::kPlain);
}

int gsr_backward_render_abs(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                            const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color, const float *dL_dcolor,
                            float *screen_grads, void *stream)
{
    return backward_render_impl(desc, cam, geom_ws, binning_ws, image_ws, rows_ws, plan, out_color, nullptr, dL_dcolor, nullptr, nullptr,
                                screen_grads, stream, BwdKind::kAbs);
}

int gsr_screen_absgrad(const gsr_frame_desc *desc, const int32_t *radii, const void *geom_ws, const float *screen_grads,
                       int32_t binned_ranks, const gsr_frame_plan *own_plan, float *out, void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (desc->tile_row_begin != 0 || desc->tile_row_end > 0) {
        set_error("gsr_screen_absgrad: whole images only (tile_row_begin = tile_row_end = 0)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if (desc->P == 0) return GSR_OK;
    if (!radii || !geom_ws || !screen_grads || !out) { set_error("gsr_screen_absgrad: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    const FrameK f = make_frame(*desc);
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
    const GeomRows rows = geom_rows(f, 0, f.P, binned_ranks, own_plan, gw.order, gw.cnt_open);          // the rows gsr_backward_geom visits
    return launch_screen_absgrad(f, radii, screen_grads, rows, out, desc->debug != 0, (hipStream_t)stream);
}

int gsr_backward_render_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                            const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color,
                            const gsr_aux_outputs *aux, const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                            float *screen_grads, void *stream)
{
    return backward_render_impl(desc, cam, geom_ws, binning_ws, image_ws, rows_ws, plan, out_color, aux, dL_dcolor, dL_ddepth, dL_dalpha,
                                screen_grads, stream, aux ? BwdKind::kAux : BwdKind::kPlain);      // aux NULL: gsr_backward_render
}

int gsr_backward_render_extra(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                              const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color,
                              const gsr_aux_outputs *aux, const float *extra, const float *extra_map, const float *dL_dcolor,
                              const float *dL_ddepth, const float *dL_dalpha, const float *dL_dextra_map, float *screen_grads,
                              void *extra_rows_ws, float *dL_dextra, void *stream)
{
    const ExtWS ext{reinterpret_cast<const float4 *>(extra), const_cast<float *>(extra_map), dL_dextra_map,
                    reinterpret_cast<float4 *>(extra_rows_ws), dL_dextra};
    return backward_render_impl(desc, cam, geom_ws, binning_ws, image_ws, rows_ws, plan, out_color, aux, dL_dcolor, dL_ddepth, dL_dalpha,
                                screen_grads, stream, BwdKind::kExt, &ext);
}

int gsr_backward_render_median(const gsr_frame_desc *desc, const gsr_camera *cam, const void *geom_ws, void *binning_ws,
                               const void *image_ws, void *rows_ws, const gsr_frame_plan *plan, const float *out_color,
                               const gsr_aux_outputs *aux, const float *dL_dcolor, const float *dL_ddepth, const float *dL_dalpha,
                               const int32_t *median_enc, const float *dL_dmedian, float *screen_grads, void *stream)
{
    const MedWS med{nullptr, const_cast<int32_t *>(median_enc), dL_dmedian};
    return backward_render_impl(desc, cam, geom_ws, binning_ws, image_ws, rows_ws, plan, out_color, aux, dL_dcolor, dL_ddepth, dL_dalpha,
                                screen_grads, stream, BwdKind::kMed, nullptr, &med);
}

static int backward_geom_impl(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                              const void *geom_ws, const float *screen_grads, int32_t g_begin, int32_t g_end, int32_t binned_ranks,
                              const gsr_frame_plan *own_plan, const gsr_grads *out, void *stream, bool depth_chain)
{
    int rc = validate(desc);
    if (rc) return rc;
    if ((rc = validate_inputs(desc, cam, g))) return rc;
    if (!out) { set_error("gsr_backward_geom: NULL grads"); return GSR_ERR_INVALID_ARGUMENT; }
    if (g_begin < 0 || g_end > desc->P || g_begin > g_end) { set_error("bad Gaussian range [%d, %d)", g_begin, g_end); return GSR_ERR_INVALID_ARGUMENT; }
    if (g_end == g_begin) return GSR_OK;
    if (!radii || !geom_ws || !screen_grads) { set_error("gsr_backward_geom: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    const FrameK f = make_frame(*desc);
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
    const GeomRows rows = geom_rows(f, g_begin, g_end, binned_ranks, own_plan, gw.order, gw.cnt_open);
    if ((rc = launch_geom_bwd(f, *cam, *g, radii, gw, screen_grads, rows, *out, desc->debug != 0, (hipStream_t)stream))) return rc;
    if (!depth_chain) return GSR_OK;
    return launch_geom_bwd_depth(f, *cam, radii, screen_grads, rows, out->means3D, desc->debug != 0, (hipStream_t)stream);
}

int gsr_backward_geom(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                      const void *geom_ws, const float *screen_grads, int32_t g_begin, int32_t g_end, int32_t binned_ranks,
                      const gsr_frame_plan *own_plan, const gsr_grads *out, void *stream)
{
    return backward_geom_impl(desc, cam, g, radii, geom_ws, screen_grads, g_begin, g_end, binned_ranks, own_plan, out, stream, false);
}

int gsr_backward_geom_aux(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                          const void *geom_ws, const float *screen_grads, int32_t g_begin, int32_t g_end, int32_t binned_ranks,
                          const gsr_frame_plan *own_plan, const gsr_grads *out, void *stream)
{
    return backward_geom_impl(desc, cam, g, radii, geom_ws, screen_grads, g_begin, g_end, binned_ranks, own_plan, out, stream, true);
}

int gsr_camera_grad_workspace_size(const gsr_frame_desc *desc, size_t *bytes)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!bytes) { set_error("gsr_camera_grad_workspace_size: NULL out"); return GSR_ERR_INVALID_ARGUMENT; }
    *bytes = camera_grad_workspace_bytes(desc->P);
    return GSR_OK;
}

int gsr_backward_camera(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                        const void *geom_ws, const float *screen_grads, int32_t binned_ranks, const gsr_frame_plan *own_plan,
                        int32_t depth_chain, void *workspace, const gsr_camera_grads *out, void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (desc->tile_row_begin != 0 || desc->tile_row_end > 0) {
        set_error("gsr_backward_camera: whole images only (tile_row_begin = tile_row_end = 0)");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    if ((rc = validate_inputs(desc, cam, g))) return rc;
    if (!out || !workspace) { set_error("gsr_backward_camera: NULL grads / workspace"); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->P > 0 && (!radii || !geom_ws || !screen_grads)) { set_error("gsr_backward_camera: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    const FrameK f = make_frame(*desc);
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
    const GeomRows rows = geom_rows(f, 0, f.P, binned_ranks, own_plan, gw.order, gw.cnt_open);          // the rows gsr_backward_geom visits
    return launch_camera_bwd(f, *cam, *g, radii, gw, screen_grads, rows, depth_chain != 0, (float *)workspace, *out, desc->debug != 0,
                             (hipStream_t)stream);
}

int gsr_backward_geom_rows(const gsr_frame_desc *desc, const gsr_camera *cam, const gsr_gaussians *g, const int32_t *radii,
                           const void *geom_ws, const float *screen_grads, const int32_t *rows, int32_t n_rows, const gsr_grads *out,
                           void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if ((rc = validate_inputs(desc, cam, g))) return rc;
    if (!out || n_rows < 0 || n_rows > desc->P || (n_rows > 0 && !rows)) { set_error("gsr_backward_geom_rows: bad argument"); return GSR_ERR_INVALID_ARGUMENT; }
    if (desc->P == 0) return GSR_OK;
    if (!radii || !geom_ws || !screen_grads) { set_error("gsr_backward_geom_rows: NULL argument"); return GSR_ERR_INVALID_ARGUMENT; }
    const FrameK f = make_frame(*desc);
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
    // the caller's list: sparse below P / 4 rows, else the dense kernel over every Gaussian
    const GeomRows visit = geom_rows(f, 0, f.P, n_rows, nullptr, reinterpret_cast<const uint32_t *>(rows), nullptr);
    return launch_geom_bwd(f, *cam, *g, radii, gw, screen_grads, visit, *out, desc->debug != 0, (hipStream_t)stream);
}

int gsr_frame_arrays(const gsr_frame_desc *desc, const void *geom_ws, const uint32_t **depth_keys, const uint32_t **depth_order)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!geom_ws) { set_error("gsr_frame_arrays: NULL workspace"); return GSR_ERR_INVALID_ARGUMENT; }
    GeomWS gw = carve_geom(const_cast<void *>(geom_ws), desc->P);
    if (depth_keys) *depth_keys = gw.sort_keys[0];
    if (depth_order) *depth_order = gw.order;
    return GSR_OK;
}

int gsr_exchange_rows_gather(const gsr_frame_desc *desc, void *geom_ws, uint32_t key_max, const float *screen_grads, int32_t n_rows,
                             int32_t *rows, float *packed, void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (n_rows < 0 || !geom_ws || (n_rows > 0 && (!screen_grads || !rows || !packed))) {
        set_error("gsr_exchange_rows_gather: bad argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    const FrameK f = make_frame(*desc);
    GeomWS gw = carve_geom(geom_ws, f.P);
    return launch_rows_gather(f, gw, key_max, screen_grads, n_rows, rows, packed, desc->debug != 0, (hipStream_t)stream);
}

int gsr_exchange_rows_scatter(const gsr_frame_desc *desc, int32_t n_rows, const int32_t *rows, const float *packed, float *screen_grads,
                              void *stream)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (n_rows < 0 || (n_rows > 0 && (!rows || !packed || !screen_grads))) { set_error("gsr_exchange_rows_scatter: bad argument"); return GSR_ERR_INVALID_ARGUMENT; }
    return launch_rows_scatter(n_rows, desc->P, rows, packed, screen_grads, desc->debug != 0, (hipStream_t)stream);
}

int gsr_mark_visible(int32_t P, const float *means3D, const float *viewmatrix, const float *projmatrix, uint8_t *present,
                     void *stream)
{
    (void)projmatrix;
    if (P < 0 || (P > 0 && (!means3D || !viewmatrix || !present))) { set_error("gsr_mark_visible: bad argument"); return GSR_ERR_INVALID_ARGUMENT; }
    return launch_mark_visible(P, means3D, viewmatrix, present, (hipStream_t)stream);
}

int gsr_debug_sort_temp_bytes(size_t *bytes)
{
    if (!bytes) return GSR_ERR_INVALID_ARGUMENT;
    *bytes = radix_temp_bytes() + 256;
    return GSR_OK;
}

int gsr_debug_sort_pairs(uint32_t *keys0, uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, int64_t n, int32_t end_bit,
                         int32_t count_on_device, void *temp, int32_t *result_buffer, void *stream)
{
    if (!keys0 || !keys1 || !vals0 || !vals1 || !temp || !result_buffer || n < 0 || n > 0xFFFFFFFFll || end_bit < 1 || end_bit > 32) {
        set_error("gsr_debug_sort_pairs: bad argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t *keys[2] = {keys0, keys1}, *vals[2] = {vals0, vals1};
    uint32_t *n_dev = reinterpret_cast<uint32_t *>((char *)temp + radix_temp_bytes());
    const uint32_t n32 = (uint32_t)n;
    if (count_on_device) GSR_HIP_CHECK(hipMemcpyAsync(n_dev, &n32, 4, hipMemcpyHostToDevice, s));
    int result = 0;
    int rc = launch_radix_sort<uint32_t>(keys, vals, count_on_device ? n_dev : nullptr, n32, (uint64_t)n, nullptr, 0, end_bit, temp,
                                         &result, "debug_sort", false, s);
    *result_buffer = result;
    if (count_on_device) GSR_HIP_CHECK(hipStreamSynchronize(s));     // n32 lives on this stack frame
    return rc;
}

int gsr_debug_sort_pairs_ex(uint32_t *keys0, uint32_t *keys1, uint32_t *vals0, uint32_t *vals1, uint32_t *vals2_0, uint32_t *vals2_1,
                            int64_t n, int64_t n_max, int64_t base, int32_t end_bit, int32_t even_passes, void *temp,
                            int32_t *result_buffer, void *stream)
{
    if (!keys0 || !keys1 || !vals0 || !vals1 || !temp || !result_buffer || (!vals2_0 != !vals2_1) || n < 0 || n > n_max ||
        n_max > 0xFFFFFFFFll || base < 0 || base + n_max > 0xFFFFFFFFll || end_bit < 1 || end_bit > 32) {
        set_error("gsr_debug_sort_pairs_ex: bad argument");
        return GSR_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = (hipStream_t)stream;
    uint32_t *keys[2] = {keys0, keys1}, *vals[2] = {vals0, vals1}, *vals2[2] = {vals2_0, vals2_1};
    uint32_t *dev = reinterpret_cast<uint32_t *>((char *)temp + radix_temp_bytes());
    const uint32_t words[2] = {(uint32_t)n, (uint32_t)base};         // count and base on the device, as the tile sort reads them
    GSR_HIP_CHECK(hipMemcpyAsync(dev, words, sizeof words, hipMemcpyHostToDevice, s));
    int result = 0;
    int rc = launch_radix_sort<uint32_t>(keys, vals, dev, 0, (uint64_t)n_max, dev + 1, 0, end_bit, temp, &result, "debug_sort", false, s,
                                         even_passes != 0, vals2_0 ? vals2 : nullptr);
    *result_buffer = result;
    GSR_HIP_CHECK(hipStreamSynchronize(s));                           // words lives on this stack frame
    return rc;
}

int gsr_profile_enable(int enable)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    profile_drain();
    g_prof.acc.clear();
    g_prof.on = enable != 0;
    return GSR_OK;
}

int gsr_profile_read(int max_entries, char (*names)[GSR_PROFILE_NAME_LEN], float *total_ms, int32_t *launches)
{
    std::lock_guard<std::mutex> lk(g_prof_mu);
    profile_drain();
    int n = 0;
    for (auto &a : g_prof.acc) {
        if (n >= max_entries) break;
        if (names) strcpy(names[n], a.name);
        if (total_ms) total_ms[n] = (float)a.ms;
        if (launches) launches[n] = a.n;
        ++n;
    }
    return n;
}

int gsr_debug_get_views(const gsr_frame_desc *desc, const void *geom_ws, const void *binning_ws, const void *image_ws,
                        const gsr_frame_plan *plan, gsr_debug_views *v)
{
    int rc = validate(desc);
    if (rc) return rc;
    if (!v || !plan) { set_error("NULL views / plan"); return GSR_ERR_INVALID_ARGUMENT; }
    memset(v, 0, sizeof *v);
    const FrameK f = make_frame(*desc);
    if (geom_ws) {
        GeomWS gw = carve_geom(const_cast<void *>(geom_ws), f.P);
        v->splat_records = reinterpret_cast<const float *>(gw.records);
        v->tiles_touched = reinterpret_cast<const uint32_t *>(gw.tiles_mass); v->depth_order = gw.order; v->point_offsets = gw.offs_full;
        v->clamped = gw.clamped;
    }
    if (binning_ws) {
        BinningWS bw = carve_binning(const_cast<void *>(binning_ws), plan_capacity(plan), f);
        v->sorted_gaussian = bw.gids[1];
        v->bwd_units = reinterpret_cast<const uint32_t *>(bw.units.units); v->bwd_unit_cap_full = bw.units.cap_full; v->bwd_unit_cap_part = bw.units.cap_part;
    }
    if (image_ws) {
        ImageWS iw = carve_image(const_cast<void *>(image_ws), f);
        v->ranges = reinterpret_cast<const uint32_t *>(iw.ranges);
        v->final_T = iw.T_state; v->n_contrib = iw.last_enc;
        v->tile_walk = iw.tile_walk; v->bwd_unit_count = iw.unit_count;
    }
    return GSR_OK;
}

}  // extern "C"
