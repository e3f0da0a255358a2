// vga_path_support.hpp -- how well every reported alignment fits every haplotype path of the graph (vga_path_support.hip), as
// vga_align_batch sees it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  Path support is defined on the record the
// alignments GAF reports for a read and on the GFA's S and P lines, and can be recomputed from those texts alone
// (tests/path_support_ref.py).  It reads what coverage reads -- the list k_cov_runs condenses every finished problem into (the
// ids of the nodes its path enters, then the events of its runs of matched bases on the linearised graph; vga_coverage.hpp) --
// and the lists are made while either of the two is on.  k_ps_build, once per vga_path_support_begin, turns the paths into one
// bitset per node (bit p: path p visits the node forward) and one per edge slot (bit p: path p steps over that edge, forward to
// forward); k_ps_score, once the host has picked the winners, gives each winner one wave.
//
// k_ps_score puts the PATHS across the lanes and walks the list: lane l of path block q owns path 64 q + l and keeps its two sums.
// The wave takes 64 list items at a time (a piece of a run inside one node with its length, or a consecutive pair of nodes with
// the slot of its edge), every lane fetches the bitset words of its own item, and the items are then handed round one by one
// (v_readlane): the owner of a path adds the item's value when its bit is set.  No atomics and no reduction on the way; LDS only
// holds the sums between rounds (each lane reads and writes its own words, so there is no barrier).  Per alignment of W nodes
// and R runs cut into E pieces, with PW = ceil(n_paths / 32) words per bitset, it reads (W - 1 + E) PW bitset words, the W + 2 R
// words of its list, and for every pair the outgoing edge slice of its first node.
#pragma once

#include "vga_common.hpp"
#include "vga_coverage.hpp"

// LDS of k_ps_score: two 32-bit sums per path
#define PS_MAX_PATHS 4096u

struct gt_state;
struct gl_state;
struct pe_state;
struct pe_queries;
// The bitsets and accumulators of a context's index while path support is on (vga_dev_index::ps: released with the index), and
// the matrices of the most recent vga_align_batch.
struct ps_state {
    uint32_t n_paths = 0, PW = 0;
    vga_dbuf<uint32_t> d_node_paths, d_edge_paths;  // n_nodes x PW, n_edges x PW
    vga_dbuf<unsigned long long> d_acc;              // sum_bases, sum_edges, top, top_alone (n_paths each), n_alignments, n_unplaced
    std::vector<unsigned long long> h_off;           // the paths as vga_path_support_begin got them: steps [h_off[p], h_off[p + 1]) of
    std::vector<uint32_t> h_steps;                   // h_steps, packed handles (vga_path_edit_begin builds the path sequences from them)
    // ---- the last call
    vga_dbuf<uint32_t> d_bases, d_edges, d_rows;
    vga_hbuf<uint32_t> h_rows;
    uint64_t last_reads = 0;
    bool have_last = false;
    // ---- the pair table while genotyping is on (vga_genotype.hip), released with this state
    gt_state *gt = nullptr;
    void (*gt_free)(gt_state *) = nullptr;
    // ---- the cost table while the read likelihood is on (vga_genotype_lik.hip), released with this state
    gl_state *gl = nullptr;
    void (*gl_free)(gl_state *) = nullptr;
    // ---- the path sequences and accumulators while the edit distance is on (vga_path_edit.hip), released with this state
    pe_state *pe = nullptr;
    void (*pe_free)(pe_state *) = nullptr;
    ps_state() = default;
    ps_state(const ps_state &) = delete;
    ps_state &operator=(const ps_state &) = delete;
    ~ps_state()
    {
        if (gt && gt_free) gt_free(gt);
        if (gl && gl_free) gl_free(gl);
        if (pe && pe_free) pe_free(pe);
    }
};
// the context's path support state while it is on (vga_path_support_begin), else null
ps_state *ps_active(vga_ctx *ctx);
// k_ps_score over the staged winners of the call that just ended (reads[i]: the read winner i is reported for), on the context's
// stream; waits for it.  The call's two n_reads x n_paths matrices are kept on the device for vga_path_support_last.  q: the
// winners' queries, read only while the edit distance is on (ps->pe).
int ps_score_winners(vga_ctx *ctx, ps_state *ps, const cov_win_view &v, const std::vector<uint32_t> &reads, uint64_t n_reads, const pe_queries *q);
