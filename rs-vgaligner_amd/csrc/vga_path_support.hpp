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
struct ab_state;

// The per-path accumulators of path support and of the edit distance: four columns of n_paths 64-bit words, then two scalars.
struct ps_acc_block {
    uint32_t n_paths = 0;
    vga_dbuf<unsigned long long> d;
    size_t words() const { return 4 * (size_t)n_paths + 2; }
    hipError_t reserve(uint32_t paths) { n_paths = paths; return d.reserve(words()); }
    int zero(vga_ctx *ctx);  // (waits for the stream)
    // column k to col[k] where col[k] is not null, the scalars to s0 and s1 likewise
    int read(vga_ctx *ctx, uint64_t *const col[4], uint64_t *s0, uint64_t *s1);
};
// behind vga_path_support_last and vga_path_edit_last (`who`): a vga_align_batch of n_reads reads has been scored; its
// n_reads x n_paths matrices src[k] go to dst[k] where dst[k] is not null
int ps_read_last(vga_ctx *ctx, const char *who, bool have_last, uint64_t last_reads, uint64_t n_reads, uint32_t n_paths, uint32_t *const dst[2],
                 const uint32_t *const src[2]);

// The bitsets and accumulators of a context's index while path support is on (vga_dev_index::ps: released with the index), and
// the matrices of the most recent vga_align_batch.
struct ps_state {
    uint32_t n_paths = 0, PW = 0;
    vga_dbuf<uint32_t> d_node_paths, d_edge_paths;  // n_nodes x PW, n_edges x PW
    ps_acc_block acc;                                // sum_bases, sum_edges, top, top_alone (n_paths each), n_alignments, n_unplaced
    std::vector<unsigned long long> h_off;           // the paths as vga_path_support_begin got them: steps [h_off[p], h_off[p + 1]) of
    std::vector<uint32_t> h_steps;                   // h_steps, packed handles (vga_path_edit_begin builds the path sequences from them)
    // ---- the last call
    vga_dbuf<uint32_t> d_bases, d_edges, d_rows;
    vga_hbuf<uint32_t> h_rows;
    uint64_t last_reads = 0;
    bool have_last = false;
    // ---- the pair table while genotyping is on (vga_genotype.hip), released with this state
    vga_owned<gt_state> gt{nullptr, nullptr};
    // ---- the cost table while the read likelihood is on (vga_genotype_lik.hip), released with this state
    vga_owned<gl_state> gl{nullptr, nullptr};
    // ---- the path sequences and accumulators while the edit distance is on (vga_path_edit.hip), released with this state
    vga_owned<pe_state> pe{nullptr, nullptr};
    // ---- the store of deficit rows while the path abundance is on (vga_abundance.hip), released with this state
    vga_owned<ab_state> ab{nullptr, nullptr};
};
// the context's path support state while it is on (vga_path_support_begin), else null
ps_state *ps_active(vga_ctx *ctx);

// The life cycle of a stage S that lives in a slot of ps_state (gt, gl, pe, ab), behind its _begin, _end and _reset entry points, which
// keep their own argument checks.  begin: path support is on; a second begin starts over; init(ps, s) sets the new state up, and a
// failure drains the stream (host arrays of init, or of the state itself, may be on their way) and releases it.
template <typename S, class Init>
int ps_child_begin(vga_ctx *ctx, const char *who, vga_owned<S> ps_state::*slot, Init &&init)
{
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "%s: path support is off (vga_path_support_begin)", who);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vga_owned<S> &own = ps->*slot;
    own.reset();
    if (!(own = vga_make_owned<S>())) return vga_set_error(ctx, VGA_ERR_NOMEM, "%s: out of host memory", who);
    int rc;
    try {
        rc = init(ps, own.get());
    } catch (const std::bad_alloc &) {
        rc = vga_set_error(ctx, VGA_ERR_NOMEM, "%s: out of host memory", who);
    }
    if (rc != VGA_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        own.reset();
    }
    return rc;
}
// end: harmless when the stage, or path support, is off
template <typename S>
int ps_child_end(vga_ctx *ctx, vga_owned<S> ps_state::*slot)
{
    ps_state *ps = ps_active(ctx);
    if (!ps) return VGA_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    (ps->*slot).reset();
    return VGA_OK;
}
// reset: zero() the stage's accumulators; off_message when it is off
template <class Zero>
int ps_child_reset(vga_ctx *ctx, bool on, const char *off_message, Zero &&zero)
{
    if (!on) return vga_set_error(ctx, VGA_ERR_ARG, "%s", off_message);
    (void)hipSetDevice(ctx->device);
    return zero();
}
// k_ps_score over the staged winners of the call that just ended (reads[i]: the read winner i is reported for), on the context's
// stream; waits for it.  The call's two n_reads x n_paths matrices are kept on the device for vga_path_support_last.  q: the
// winners' queries, read only while the edit distance is on (ps->pe).
int ps_score_winners(vga_ctx *ctx, ps_state *ps, const cov_win_view &v, const std::vector<uint32_t> &reads, uint64_t n_reads, const pe_queries *q);
