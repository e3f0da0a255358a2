// vga_subgraph.hpp -- device-side chain -> subgraph -> POA node table (vga_subgraph.hip), as vga_align.hip and poa_run see it.
//
// Replaces, on the GPU, the host walk of find_range_chain / extend_range_chain_2 / find_nodes_edges_for_abpoa
// (src/align.rs:267-402, 523-665, 670-724) and the node-table construction poa_prepare does for host graphs.
#pragma once

#include <cstdint>

#include "vga_common.hpp"
#include "vga_sg_records.hpp"  // sg_desc, sg_sum, sg_off

// The prepared problems of one vga_align_batch call (device store + what the host needs of it).  The problems come in
// launch order and are prepared in two parts: [0, split) before the first DP launch, [split, n) beside it on a stream
// of its own (sg_prepare_rest), so that only the first part's kernels sit in front of the DP.
struct sg_part {
    uint64_t p0 = 0, p1 = 0;
    const uint4 *d_ntab = nullptr;
    const uint32_t *d_preds = nullptr, *d_sinks = nullptr;
    const char *d_seq = nullptr;
    const uint32_t *d_handles = nullptr;  // packed handle of every node, indexed from off[p].node0 (k_cov_runs)
    const uint32_t *h_handles = nullptr, *h_first_row = nullptr;  // host copies (pinned), indexed from off[p].node0
    bool ready = false;
};
struct sg_store {
    uint64_t n = 0, split = 0;
    int remain_rule = 0;            // vga_poa_params.remain_rule the node tables are built for
    const sg_sum *sum = nullptr;    // host, n entries (valid for a part once it is ready)
    const sg_off *off = nullptr;    // host, n entries, offsets inside the problem's part
    const sg_off *d_off = nullptr;  // device copy
    const char *d_reads = nullptr;
    sg_part part[2];
    const sg_part &of(uint64_t p) const { return part[p >= split ? 1 : 0]; }
};

// Runs the extraction for chains [0, split) of n on ctx->stream and waits for it.  `store` points into the context's
// workspace and stays valid until the next call.  read_no[p] is the read of chain p in the batch: it only labels the records of
// the VGA_SG_DUMP diagnostic.  Returns VGA_OK or a negative VGA_ERR_*.
int sg_prepare(vga_ctx *ctx, const sg_desc *descs, const uint64_t *q_src, const uint64_t *read_no, uint64_t n, uint64_t split, const char *d_reads,
               int remain_rule, sg_store &store);
// ... and for chains [split, n), on the workspace's side stream (it may run beside DP launches); waits for it.
int sg_prepare_rest(vga_ctx *ctx, sg_store &store);
