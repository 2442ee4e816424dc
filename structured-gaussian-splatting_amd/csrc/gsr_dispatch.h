// gsr_dispatch.h — the host-side path rules of a frame, each stated once: which kernels a chunk's ordering, binning, colours, blend
// and backward take, when the remaining chunks merge, and what the plan says about sizes.  Every rule is a named constant plus a
// pure function of plain values, FrameK and gsr_frame_plan: no HIP, no environment (the switches arrive as booleans), no state.
// Plain C++17: tests/dispatch_host.cpp compiles this header with g++ and tests/test_dispatch_ref.py holds it to the Python mirrors
// (tests/binning_ref.py chunk_cells, tests/test_gpu_parity.py _geom_variants, _native.py) without a GPU.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/gsrast.h"
#include "gsr_math.h"

namespace gsr {

inline int bit_width(uint32_t v)          // bits needed to write v: 0 for 0, else 1 + the position of its highest set bit
{
    int b = 0;
    while (v) { ++b; v >>= 1; }
    return b;
}

// ---- what the plan says about sizes
// instances the frame's binning workspace holds
inline long long plan_capacity(const gsr_frame_plan *plan) { return plan->binning_capacity > 0 ? plan->binning_capacity : plan->num_rendered; }

// Instances the backward's scratch must hold: exact when the forward stopped early (the count was read back with the open-tile
// count); when the LAST chunk ran its count stayed on the device and the bound is what the chunks that ran could have emitted.
inline long long rows_bound(const gsr_frame_plan *plan)
{
    long long n = plan->instances_emitted;
    if (n < 0) {
        n = 0;
        for (int c = 0; c < plan->chunks_run && c < GSR_MAX_CHUNKS; ++c) n += plan->chunk_instances_max[c];
    }
    return n < 1 ? 1 : n;
}

// bytes of the row-valid flags of n instances: one byte each, rounded up to whole 16-byte words of their padded block
inline size_t row_flag_bytes(long long n) { return ((size_t)(n < 1 ? 1 : n) + 15) & ~(size_t)15; }

// row-valid flags to clear ahead of the blend backward: those of the instances the chunks that ran can have emitted (never more
// than the binning workspace holds)
inline size_t valid_bytes(const gsr_frame_plan *plan)
{
    const long long n = rows_bound(plan), cap = plan_capacity(plan);
    return row_flag_bytes(n > cap ? cap : n);
}

// What a binning workspace sized for the first chunk only must hold: what the first depth chunk can emit at most, plus headroom for
// a small straggler chunk; never more than R.  (A frame whose tiles saturate never gets past that chunk.)
constexpr int64_t kFirstChunkSlack = 1 << 20;
inline int64_t first_chunk_capacity(const gsr_frame_plan &plan)
{
    const int64_t n = plan.num_chunks > 1 ? plan.chunk_instances_max[0] + plan.chunk_instances_max[0] / 4 + kFirstChunkSlack : plan.num_rendered;
    return n > plan.num_rendered ? plan.num_rendered : n;
}

// gsr_forward's early zero fill goes behind the first chunk's readback kernel, ahead of the wait for it.  Whether the frame ends up
// sparse is only known after the readback: the fill is enqueued when the first planned chunk alone is sparse - a frame whose first
// chunk holds a quarter of the Gaussians takes the dense path whatever follows - and is wasted bandwidth, nothing more, when later
// chunks make the frame dense after all.  A one-chunk frame has no readback to hide it behind: it fills late.
inline bool early_fill_before_wait(const gsr_frame_plan &plan, int P)
{
    return plan.num_chunks > 1 && (long long)plan.chunk_rank_begin[1] * 4 < (long long)P;
}

// ---- the live filter and the merge of the remaining chunks
// A late, large chunk with most tiles closed (a frame with a corner no splat covers runs every chunk, and the last one is most of
// the scene): first move the Gaussians whose rectangle still holds an open tile to the front of its range (launch_live_filter) —
// only those get sorted and binned, one wave each.
constexpr int kLiveFilterMin = 1 << 16;         // the filter's launches pay off from this many Gaussians on
// ... and the one-wave-per-Gaussian count pass a filtered chunk takes needs its mask scratch, ceil(n_max / 64) + n words of 8 bytes,
// inside the n_max instance slots the chunk may fill
inline bool live_filter_pays(long long n, uint64_t n_max) { return n >= kLiveFilterMin && n_max / 32 + 2 * (uint64_t)n + 4 <= n_max; }
inline bool mostly_closed(uint32_t open_now, long long slab_tiles) { return (long long)open_now * 2 < slab_tiles; }

// what the chunks so far left behind, read back with the open-tile count (the defaults: before the first readback)
struct Progress {
    uint64_t emitted = 0;               // instances earlier chunks emitted (exact)
    uint32_t open = 0xFFFFFFFFu;        // tiles still open before the current chunk
    uint32_t stuck = 0;                 // ... and those with a pixel nothing covers yet (known from chunk 1 on)
};

// chunk c goes through the live filter (c > 0: nothing is closed before the first chunk)
inline bool chunk_filtered(int c, long long n, uint64_t n_max, const Progress &now, long long slab_tiles, bool no_live_filter)
{
    return c > 0 && !no_live_filter && mostly_closed(now.open, slab_tiles) && live_filter_pays(n, n_max);
}

// a chunk that may emit n_max instances behind those already emitted does not fit the binning workspace: the frame stops with
// GSR_ERR_WORKSPACE before anything of that chunk is written
inline bool capacity_short(uint64_t emitted_before, uint64_t n_max, long long capacity) { return emitted_before + n_max > (uint64_t)capacity; }

// relative keys: a chunk's keys are re-based to its lower end, the first chunk's to the near cut
constexpr uint32_t kNearBits = 0x3E4CCCCDu;                      // 0.2f (GSR_NEAR_CUT): in_frustum() keeps view depth > 0.2
// parts: a filtered range may span several planned chunks (merged below); their relative keys are re-based to the first one's
struct LiveParts { int n; uint32_t end[GSR_MAX_CHUNKS]; uint32_t delta[GSR_MAX_CHUNKS]; };      // end: position in the range; delta: added to the key

// The plan step in front of chunk c.  A frame that is not going to close (an uncovered corner: some open tile still has a pixel that
// nothing has covered after the chunks so far, k_render_fwd marks those): every further chunk costs its fixed ~250 us for little.
// All remaining chunks then become ONE, which goes through the live filter (its Gaussians' relative keys are re-based there: parts).
// The plan keeps the planned chunks' bounds behind the merged one.  kShort: the merged chunk does not fit the workspace (*need
// instances); the plan is untouched, so that the re-run decides the same.
enum class Merge { kNone, kMerged, kShort };
inline Merge merge_rest(gsr_frame_plan *plan, int c, const Progress &now, long long slab_tiles, long long capacity, bool enabled,
                        LiveParts *parts, uint64_t *need)
{
    *parts = LiveParts{1, {0}, {0}};
    const int last_c = plan->num_chunks - 1;
    if (!enabled || c <= 0 || c < plan->chunks_sorted || c >= last_c || now.stuck == 0 || !mostly_closed(now.open, slab_tiles)) return Merge::kNone;
    uint64_t m_max = 0;
    for (int j = c; j <= last_c; ++j) m_max += (uint64_t)plan->chunk_instances_max[j];
    const long long m_n = plan->chunk_rank_begin[last_c + 1] - plan->chunk_rank_begin[c];
    if (!live_filter_pays(m_n, m_max) || m_max > 0xFFFFFFFFull) return Merge::kNone;
    if (capacity_short(now.emitted, m_max, capacity)) { *need = now.emitted + m_max; return Merge::kShort; }
    auto base_of = [&](int j) { const uint32_t e = plan->chunk_key_end[j - 1]; return e < kNearBits ? kNearBits : e; };
    parts->n = last_c - c + 1;
    for (int j = c; j <= last_c; ++j) {
        parts->end[j - c] = (uint32_t)(plan->chunk_rank_begin[j + 1] - plan->chunk_rank_begin[c]);
        parts->delta[j - c] = base_of(j) - base_of(c);
    }
    plan->chunk_rank_begin[c + 1] = plan->chunk_rank_begin[last_c + 1];
    plan->chunk_key_end[c] = plan->chunk_key_end[last_c];
    plan->chunk_instances_max[c] = (int64_t)m_max;
    plan->num_chunks = c + 1;
    return Merge::kMerged;
}

// ---- the chunk's depth order (launch_chunk_order)
constexpr int kSmallSortMax = 16384;            // chunks of up to this many Gaussians are ordered by one launch; a filtered chunk never
inline bool order_in_one_launch(int n, bool filtered) { return n <= kSmallSortMax && !filtered; }      // (its count lives on the device)

// ---- the chunk's tile lists (launch_chunk_binning)
// Variant B (flat) packs the (Gaussian, tile) candidates of 64 Gaussians into full wave steps: right when rectangles are small;
// chunks of few large splats (the nearest ones) get a team of 1, 4 or 16 waves per Gaussian (variant A).  By the chunk's average
// tiles per Gaussian, n_max / n:
constexpr uint64_t kFlatBelowAvg = 24, kTeam4FromAvg = 96, kTeam16FromAvg = 1024;
// A' (gather instead of emit + sort) when the ranks x tiles bit tests are cheaper than sorting the instances: up to kGatherTestsPerInstance
// tests per instance of the bound plus kGatherTestsSlack; its scratch (mask prefixes, rank metadata: n_max / 64 + 9 n + 5 words) sits
// in the idle key buffer, inside the n_max slots of the chunk
constexpr uint64_t kGatherTestsPerInstance = 24, kGatherTestsSlack = 1ull << 22;
constexpr int kGatherMaxRanks = 1 << 26;
// chunks of up to this many Gaussians: k_tile_ranges scans the per-rank counts itself (saves the launch of a one-block scan)
constexpr int kRankScanMax = 16384;
// The blend kernels find a sorted entry's Gaussian (| quadrant mask) in gids[1], always.  Sorts from this many instances on carry the
// word through the radix passes as a second payload (the emit kernels then write it into the buffer the passes leave in [1]); smaller
// ones, whose slot -> Gaussian table stays in the L2 / Infinity Cache, gather it behind the sort (the gather read 128 B per 4-byte
// word, 3.1 GB at 23 M)
constexpr uint64_t kCarryGidFrom = 4ull << 20;
// a filtered chunk: a fixed grid walks the live front part; everybody else's count is zero from the start
constexpr int kFilteredGridMax = 65536;         // (4 k: +35 us per launch, 256 k: +20 us; measured)

struct BinPath {
    bool flat;            // variant B; else variant A with
    int team;             //   this many waves per Gaussian (1, 4, 16)
    int team_grid;        //   and this many workgroups
    bool gather;          // A': lists by gather (never flat), else emit + radix sort
    bool fused_scan;      // gather: the rank scan rides in k_tile_ranges
    bool carry_gid;       // sort: the Gaussian word is a second payload of the radix passes
    int tile_bits;        // key bits of the tile sort (>= 1)
    int sort_passes;      // 8-bit radix passes over them
    int result;           // the buffer the passes leave the lists in; a gathered list ends there too, so that all chunks of a frame agree
    int gid_emit;         // sort: the gids buffer the emit kernels write, so that the passes (or the gather behind them) end in gids[1]
};

// n > 0 Gaussians that may emit n_max instances; slab_tiles: tiles of the frame's slab, Tn: of the whole image.
// A chunk the live filter went through: few survivors, every one of them with work -> one wave per Gaussian whatever the rectangle
// size (64 ranks per wave would leave a handful of long-running waves), never gathered
inline BinPath bin_path(int n, uint64_t n_max, bool filtered, uint64_t slab_tiles, size_t Tn, bool no_gather)
{
    BinPath p;
    const uint64_t avg = n_max / (uint64_t)n;
    p.flat = avg < kFlatBelowAvg && !filtered;
    p.team = filtered ? 1 : avg >= kTeam16FromAvg ? 16 : avg >= kTeam4FromAvg ? 4 : 1;
    p.team_grid = filtered && n > kFilteredGridMax ? kFilteredGridMax : n;
    const uint64_t scratch_words = n_max / 64 + 1 + 9 * (uint64_t)n + 4;
    p.gather = !p.flat && !filtered && !no_gather && n < kGatherMaxRanks &&
               (uint64_t)n * slab_tiles <= kGatherTestsPerInstance * n_max + kGatherTestsSlack && scratch_words <= n_max;
    p.fused_scan = p.gather && n <= kRankScanMax;
    p.carry_gid = n_max >= kCarryGidFrom;
    p.tile_bits = bit_width((uint32_t)(Tn ? Tn - 1 : 0));
    if (p.tile_bits < 1) p.tile_bits = 1;
    p.sort_passes = (p.tile_bits + 7) / 8;
    p.result = p.sort_passes & 1;
    p.gid_emit = p.carry_gid && !(p.sort_passes & 1) ? 1 : 0;
    return p;
}

// ---- the chunk's colours (launch_chunk_colors): the chunk is every visible Gaussian and most Gaussians are visible: walk the tensor
// in index order
inline bool colors_in_index_order(int r0, int r1, int num_visible, int P)
{
    return r0 == 0 && r1 >= num_visible && (long long)num_visible * 2 >= (long long)P;
}

// ---- the chunk's blend forward: small splats (fewer than 4.5 tiles per Gaussian on average; filtered chunks bin a small, unknown part
// of their bound) take one 16-lane group per quadrant
inline bool small_splats(uint64_t n, uint64_t n_max, bool filtered) { return !filtered && n > 0 && n_max * 2 < n * 9; }

// ---- a median frame (include/gsrast_median.h) is an aux frame at every step: its chunks take the mapping small_splats() chooses, in
// the median instantiation of the aux blend forward; its blend backward is ONE more instantiation of the aux one (row slot 9 carries the
// median's share of dL/dz), so the row reduction and the depth chain that follow are the aux frame's own kernels, and no launch is added.
// With extra colours the ext kernels would be needed too: ext x median is not built, such a frame is refused.
constexpr bool kMedianReducesAsAux = true;      // launch_reduce_rows / k_geom_bwd_depth of a median frame: the aux frame's
inline bool median_frame_allowed(bool aux, bool ext, bool stats, bool whole_image) { return aux && !ext && !stats && whole_image; }

// ---- the chunk's row reduction (launch_reduce_rows): a whole wave per Gaussian where the chunk's Gaussians own many rows each (the
// nearest, screen-filling splats: a few thousand rows), eight lanes otherwise — and always eight for a chunk that went through the live
// filter, whose instance bound says nothing about what it emitted (a training frame's last chunk is most of the scene with a bound of
// tens of millions: 64 lanes for each of its 1e6 ranks was 100 us of idle threads).
// (two lanes per Gaussian for small splats, measured: 89 us against 81 at cfg3n, 352 against 374 at cfg5n — not kept)
constexpr long long kReduceWideFromAvg = 48;
inline bool reduce_wide(int n, long long n_max, bool filtered) { return !filtered && n_max / (long long)n >= kReduceWideFromAvg; }      // n > 0

// ---- the geometry backward's rows
// Depth ranks that can own a gradient, as far as the host knows: the chunks that ran, a chunk that went through the live filter
// counted as nothing (only the Gaussians that still reached an open tile were binned: few, and how few is the device's knowledge).
// Decides "sparse geometry backward + zero fill" against "dense geometry backward" (sparse below P / 4).
inline long long effective_binned_ranks(const gsr_frame_plan &plan)
{
    long long n = 0;
    const int chunks = (plan.num_rendered > 0 && plan.chunks_run > 0) ? plan.chunks_run : 0;
    for (int c = 0; c < chunks && c < GSR_MAX_CHUNKS; ++c)
        if (!((plan.chunks_filtered >> c) & 1)) n += plan.chunk_rank_begin[c + 1] - plan.chunk_rank_begin[c];
    return n;
}
// the backward visits the ranks [0, n_ranks) of a row list (sparse) instead of the Gaussians [g0, g1)
inline bool geom_bwd_sparse(const FrameK &f, int g0, int g1, int n_ranks, bool own_frame_sparse)
{
    return n_ranks >= 0 && g0 == 0 && g1 == f.P && (own_frame_sparse || (long long)n_ranks * 4 < (long long)f.P);
}
// The rows gsr_backward_geom(_aux), gsr_backward_geom_rows, gsr_screen_absgrad and gsr_backward_camera visit; the choice is made here,
// once, and every launcher of the geometry backward takes it as it is.
struct GeomRows {
    int g0, g1;                 // dense: the Gaussians [g0, g1)
    int n_ranks;                // sparse: the ranks [0, n_ranks) of `rows`
    bool own_sparse, sparse;
    const uint32_t *rows;       // (device) sparse: the row list, else NULL
    const uint32_t *cnt_open;   // (device) own_sparse and sparse: GeomWS::cnt_open - ranks that emitted no instance are skipped before
                                // anything of theirs is read; else NULL
    int count() const { return sparse ? n_ranks : g1 - g0; }      // threads of a launch over them
};
// own_plan (honoured for the whole range [0, P) only): the gradients come from gsr_backward_render of THIS frame: the ranks of the
// chunks that ran, and among them only those that emitted an instance, can be non-zero; sparse (fill + visit those) unless unfiltered
// chunks hold P / 4 Gaussians or more.  rows / cnt_open: the list binned_ranks counts (the frame's depth order, or the caller's) and
// the frame's per-rank instance counts.
inline GeomRows geom_rows(const FrameK &f, int g_begin, int g_end, int binned_ranks, const gsr_frame_plan *own_plan, const uint32_t *rows,
                          const uint32_t *cnt_open)
{
    GeomRows r{g_begin, g_end, binned_ranks, false, false, nullptr, nullptr};
    if (own_plan && g_begin == 0 && g_end == f.P && own_plan->num_rendered > 0 && own_plan->chunks_run > 0) {
        r.n_ranks = own_plan->chunk_rank_begin[own_plan->chunks_run];
        r.own_sparse = effective_binned_ranks(*own_plan) * 4 < (long long)f.P;
    }
    r.sparse = g_end > g_begin && geom_bwd_sparse(f, g_begin, g_end, r.n_ranks, r.own_sparse);
    if (r.sparse) { r.rows = rows; r.cnt_open = r.own_sparse ? cnt_open : nullptr; }
    return r;
}

}  // namespace gsr
