// vga_subgraph_host.hpp -- the subgraphs of a vga_align_batch call from host threads (vga_subgraph_host.hip), as vga_align.hip
// sees them: selected by VGA_SUBGRAPH=host in place of the device store of vga_subgraph.hpp.
#pragma once

#include "vga_poa_internal.hpp"

struct sg_host_walk {
    // the call's problems: problem p is chain prob_chain[p] of read prob_read[p] (both outlive the walk)
    sg_host_walk(vga_ctx *ctx, const vga_batch *b, const vga_map_result *m, const std::vector<uint64_t> &prob_read,
                 const std::vector<uint64_t> &prob_chain);
    ~sg_host_walk();
    sg_host_walk(const sg_host_walk &) = delete;
    sg_host_walk &operator=(const sg_host_walk &) = delete;
    // poa_feed::prepare: builds the listed problems' subgraphs and fills in the graph part of their views
    void build(const uint32_t *ids, uint64_t cnt, poa_view *views);
    // the packed handles of problem p's nodes, in node order (valid once the problem is built)
    const uint32_t *handles(uint64_t p) const;
    // VGA_TRACE: where the threads' time went since the last call of this, over every walk of the process
    static void trace_thread_time();

    vga_ctx *const ctx;
    const vga_batch *const b;
    const vga_map_result *const m;
    const std::vector<uint64_t> &prob_read, &prob_chain;
    struct impl;
    impl *const d;
};
