// vga_coverage.hpp -- read coverage of graph bases, nodes and edges (vga_coverage.hip), as poa_run and vga_align_batch see it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  Coverage is defined on the record the
// alignments GAF reports for a read (the winner of best_alignment_for_query) and can be recomputed from that text alone
// (tests/coverage_ref.py).  Two facts of the POA pipeline shape it: the operations of a sub-batch are recycled when its slot is
// refilled, and the winner among a read's candidates is known only after poa_run has returned.  So k_cov_runs, enqueued behind
// k_poa_text on the slot's stream, condenses every finished problem into a short list (the ids of the nodes its path enters, then
// the +1 / -1 events of its runs of matched bases on the linearised graph), and k_cov_add, once the host has picked the winners,
// adds the winners' lists to the counters: a difference array over the bases, a word per node, a word per edge slot.
#pragma once

#include "vga_common.hpp"
#include "vga_poa_launch.hpp"
#include "vga_subgraph.hpp"

// one problem's list: n_nodes node ids, then n_events words (position << 1 | 1 for a -1 event), at word `off` of its buffer
struct cov_rec {
    uint32_t off, n_nodes, n_events;
    uint32_t flags;  // 0 nothing (the problem has no alignment yet), 1 in the call's device buffer, 2 no room there, 3 built by the host
};

struct cov_state;
// The lists have two readers: the coverage counters (k_cov_add) and path support (vga_path_support.hip: k_ps_score).  The state
// exists, and poa_run makes lists, while either is on.
enum : uint32_t { COV_USER_COVERAGE = 1u, COV_USER_PATHS = 2u };
// the context's counters while counting is on (vga_coverage_begin), else null
cov_state *cov_active(vga_ctx *ctx);
// the context's list state while any reader is on, else null
cov_state *cov_lists_active(vga_ctx *ctx);
// a reader turns itself on (creates the state if it is the first) / off (the last one out releases it)
int cov_lists_acquire(vga_ctx *ctx, uint32_t user, const char *who);
void cov_lists_release(vga_ctx *ctx, uint32_t user);
// start of a poa_run call of n problems whose queries hold total_q bases: the buffer of lists is sized and its cursor zeroed
int cov_call_begin(vga_ctx *ctx, cov_state *cv, uint64_t n, uint64_t total_q);
// k_cov_runs for the nb problems staged on a slot, and the copy of their records into the slot's result set `oset`
hipError_t cov_enqueue_runs(vga_ctx *ctx, cov_state *cv, hipStream_t st, int slot, int oset, uint32_t nb, const poa_launch_bufs &b, const uint32_t *ids,
                            const sg_store &store);
// the records of a finished launch (valid once its stream is synchronised)
const cov_rec *cov_launch_recs(const cov_state *cv, int slot, int oset);
// keeps the record of problem p (a later run of the same problem replaces it)
void cov_keep(cov_state *cv, uint32_t p, const cov_rec &r);
// the host route for a problem whose list found no room: the same list from the operations as they came back (stored sink -> source)
void cov_keep_from_ops(cov_state *cv, uint32_t p, const uint8_t *ops, const uint32_t *orow, uint32_t nops, const uint32_t *first_row, uint32_t n_nodes,
                       const uint32_t *handles, const std::vector<uint32_t> &node_start);
// the records of the winners (problem indices of the call that just ended) and the lists the host built go to the device, on the
// context's stream; `v` is what a kernel launched on that stream afterwards reads (all null for no winners)
struct cov_win_view {
    const cov_rec *recs;          // one per winner
    const uint32_t *lists;        // records with flags 1 index this buffer,
    const uint32_t *host_lists;   // records with flags 3 this one
};
int cov_stage_winners(vga_ctx *ctx, cov_state *cv, const std::vector<uint32_t> &winners, cov_win_view &v);
// k_cov_add over the nw staged winners, on the context's stream; waits for it
int cov_add_winners(vga_ctx *ctx, cov_state *cv, size_t nw);
