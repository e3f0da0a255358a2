// vga_coverage.hpp -- read coverage of graph bases, nodes and edges (vga_coverage.hip), as poa_run and vga_align_batch see it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  Coverage is defined on the record the
// alignments GAF reports for a read (the winner of best_alignment_for_query) and can be recomputed from that text alone
// (tests/coverage_ref.py).  Two facts of the POA pipeline shape it: the operations of a sub-batch are recycled when its slot is
// refilled, and the winner among a read's candidates is known only after poa_run has returned.  So k_cov_runs, enqueued behind
// k_poa_text on the slot's stream, condenses every finished problem into a short list (the ids of the nodes its path enters, then
// the +1 / -1 events of its runs of matched bases on the linearised graph), and k_cov_add, once the host has picked the winners,
// adds the winners' lists to the counters: a difference array over the bases, a word per node, a word per edge slot.
//
// poa_run and vga_align_batch reach all of that through cov_maker() (vga_oplist.hpp: the frame of a list maker); what is declared
// beside it is the second reader of the run lists, path support.
#pragma once

#include "vga_oplist.hpp"

// one problem's list (vga_oplist.hpp): n_a node ids, then n_b event words (position << 1 | 1 for a -1 event); flags 0 to 3
using cov_rec = oplist_rec;

struct cov_state;
const oplist_maker &cov_maker();
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
// what a kernel launched on the context's stream reads once the nw winners of a call are staged (oplist_call::stage_winners): all null
// for no winners
struct cov_win_view {
    const cov_rec *recs;          // one per winner
    const uint32_t *lists;        // records with flags 1 index this buffer,
    const uint32_t *host_lists;   // records with flags 3 this one
};
cov_win_view cov_staged_winners(const cov_state *cv, size_t nw);
