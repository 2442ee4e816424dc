// dispatch_host.cpp — csrc/gsr_dispatch.h compiled by g++ (under AddressSanitizer and UBSan: tests/test_dispatch_ref.py builds it) as a
// stand-alone program: reads one case per line from stdin, prints the header's decisions, one line per case.  Test infrastructure:
// nothing in the product loads it.
//
//   bin n n_max filtered slab_tiles Tn no_gather     -> flat team team_grid gather fused_scan carry_gid tile_bits sort_passes result gid_emit
//   filter c n n_max open slab_tiles no_live_filter  -> live_filter_pays mostly_closed chunk_filtered
//   small n n_max filtered                           -> small_splats
//   wide n n_max filtered                            -> reduce_wide
//   order n filtered                                 -> order_in_one_launch
//   colors r0 r1 V P                                 -> colors_in_index_order
//   plan <27 + 3 GSR_MAX_CHUNKS numbers: read_plan>  -> (sets the plan of the commands below; prints nothing)
//   sizes                                            -> plan_capacity rows_bound valid_bytes first_chunk_capacity
//   early P                                          -> early_fill_before_wait
//   geom P g0 g1 binned_ranks own                    -> effective_binned_ranks n_ranks own_sparse sparse count has_rows has_cnt_open
//   merge c emitted open stuck slab capacity enabled -> status need num_chunks rank_begin[c + 1] key_end[c] instances_max[c] parts.n
//                                                       end[0 .. n) delta[0 .. n)        (the plan stays merged for later commands)
#include <inttypes.h>
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <sstream>
#include <string>

#include "../structured-gaussian-splatting_amd/csrc/gsr_dispatch.h"

using namespace gsr;

static gsr_frame_plan read_plan(std::istringstream &in)
{
    gsr_frame_plan p;
    memset(&p, 0, sizeof p);
    long long v;
    in >> p.num_rendered >> p.num_visible >> p.num_chunks >> p.chunks_run >> p.chunks_filtered >> p.chunks_sorted >> p.instances_emitted >>
        p.binning_capacity >> p.key_max;
    for (int c = 0; c <= GSR_MAX_CHUNKS; ++c) { in >> v; p.chunk_rank_begin[c] = (int32_t)v; }
    for (int c = 0; c < GSR_MAX_CHUNKS; ++c) { in >> v; p.chunk_instances_max[c] = v; }
    for (int c = 0; c < GSR_MAX_CHUNKS; ++c) { in >> v; p.chunk_key_end[c] = (uint32_t)v; }
    return p;
}

int main()
{
    gsr_frame_plan plan;
    memset(&plan, 0, sizeof plan);
    static const uint32_t rows_dev[1] = {0}, cnt_dev[1] = {0};      // stand-ins for the device arrays: geom_rows only hands them on
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        if (!(in >> cmd)) continue;
        if (cmd == "bin") {
            long long n, filtered, no_gather;
            unsigned long long n_max, slab, Tn;
            in >> n >> n_max >> filtered >> slab >> Tn >> no_gather;
            const BinPath p = bin_path((int)n, n_max, filtered != 0, slab, (size_t)Tn, no_gather != 0);
            printf("%d %d %d %d %d %d %d %d %d %d\n", p.flat, p.team, p.team_grid, p.gather, p.fused_scan, p.carry_gid, p.tile_bits,
                   p.sort_passes, p.result, p.gid_emit);
        } else if (cmd == "filter") {
            long long c, n, slab, off;
            unsigned long long n_max, open;
            in >> c >> n >> n_max >> open >> slab >> off;
            Progress now;
            now.open = (uint32_t)open;
            printf("%d %d %d\n", live_filter_pays(n, n_max), mostly_closed((uint32_t)open, slab),
                   chunk_filtered((int)c, n, n_max, now, slab, off != 0));
        } else if (cmd == "small" || cmd == "wide") {
            long long n, n_max, filtered;
            in >> n >> n_max >> filtered;
            printf("%d\n", cmd == "small" ? small_splats((uint64_t)n, (uint64_t)n_max, filtered != 0) : reduce_wide((int)n, n_max, filtered != 0));
        } else if (cmd == "order") {
            long long n, filtered;
            in >> n >> filtered;
            printf("%d\n", order_in_one_launch((int)n, filtered != 0));
        } else if (cmd == "colors") {
            long long r0, r1, V, P;
            in >> r0 >> r1 >> V >> P;
            printf("%d\n", colors_in_index_order((int)r0, (int)r1, (int)V, (int)P));
        } else if (cmd == "plan") {
            plan = read_plan(in);
        } else if (cmd == "sizes") {
            printf("%lld %lld %zu %" PRId64 "\n", plan_capacity(&plan), rows_bound(&plan), valid_bytes(&plan), first_chunk_capacity(plan));
        } else if (cmd == "early") {
            long long P;
            in >> P;
            printf("%d\n", early_fill_before_wait(plan, (int)P));
        } else if (cmd == "geom") {
            long long P, g0, g1, binned, own;
            in >> P >> g0 >> g1 >> binned >> own;
            FrameK f;
            memset(&f, 0, sizeof f);
            f.P = (int)P;
            const GeomRows r = geom_rows(f, (int)g0, (int)g1, (int)binned, own ? &plan : nullptr, rows_dev, cnt_dev);
            printf("%lld %d %d %d %d %d %d\n", effective_binned_ranks(plan), r.n_ranks, r.own_sparse, r.sparse, r.count(), r.rows != nullptr,
                   r.cnt_open != nullptr);
        } else if (cmd == "merge") {
            long long c, slab, capacity, enabled;
            unsigned long long emitted, open, stuck;
            in >> c >> emitted >> open >> stuck >> slab >> capacity >> enabled;
            Progress now;
            now.emitted = emitted; now.open = (uint32_t)open; now.stuck = (uint32_t)stuck;
            LiveParts parts;
            uint64_t need = 0;
            const Merge m = merge_rest(&plan, (int)c, now, slab, capacity, enabled != 0, &parts, &need);
            printf("%d %" PRIu64 " %d %d %u %" PRId64 " %d", (int)m, need, plan.num_chunks, plan.chunk_rank_begin[c + 1], plan.chunk_key_end[c],
                   plan.chunk_instances_max[c], parts.n);
            for (int j = 0; j < parts.n; ++j) printf(" %u", parts.end[j]);
            for (int j = 0; j < parts.n; ++j) printf(" %u", parts.delta[j]);
            printf("\n");
        } else {
            fprintf(stderr, "dispatch_host: unknown command '%s'\n", cmd.c_str());
            return 2;
        }
        if (in.fail()) { fprintf(stderr, "dispatch_host: bad arguments in '%s'\n", line.c_str()); return 2; }
    }
    return 0;
}
