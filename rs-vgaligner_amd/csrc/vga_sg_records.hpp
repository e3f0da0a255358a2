// vga_sg_records.hpp -- the plain records host and kernels exchange for the device-side subgraph extraction (vga_subgraph.hip).
// No HIP type: vga_align_plan.hpp fills sg_desc and reads sg_sum under a host compiler alone.
#pragma once

#include <cstdint>

// one chain, as the host hands it over (the extremes of its anchors; the reduction over the anchors is the one the launch
// order needs anyway)
struct sg_desc {
    uint32_t pmin, pmax;        // smallest / largest forward position among the anchors' begins and inclusive ends
    uint32_t q_first, t_first;  // first anchor: query_begin, target_begin
    uint32_t q_last, te_last;   // last anchor: query_begin, target_end (exclusive)
    uint32_t qlen, pad;
};

// what the kernels report per problem
struct sg_sum {
    uint32_t n_nodes;  // handles of the subgraph
    uint32_t N;        // rows = graph bases
    uint32_t n_preds, n_sinks;
    uint32_t wlo, whi;  // words of the handle bitmap that hold set bits
    uint32_t longest;   // `remain` of the virtual source: graph bases on the source-sink path the remain rule follows
    uint32_t life;      // largest edge span (in nodes) among the nodes that use the value-row ring
    uint32_t flags;     // bit 0: malformed for the POA kernels (in-degree > 255, too many rows)
    uint32_t pad[3];
};

// where a problem's pieces live in the store
struct sg_off {
    uint64_t node0;  // handles / first_row: node0 .. node0 + n_nodes;  node table: node0 + problem index (one source entry each)
    uint64_t pred0, sink0, seq0;
    uint64_t q_src;  // first base of the query in the batch's device copy of the reads
};
