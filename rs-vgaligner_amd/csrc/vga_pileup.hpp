// vga_pileup.hpp -- what the reported alignments say at every graph base (vga_pileup.hip), as poa_run and vga_align_batch see it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  The pileup is defined on the record the
// alignments GAF reports for a read and can be recomputed from that text alone (tests/pileup_ref.py): per graph base seven
// counters, A C G T N del ins.  It has the shape of coverage (vga_coverage.hpp) for the same two reasons -- a sub-batch's operations
// are recycled with its slot, and the winners are picked on the host after poa_run has returned -- with lists and buffers of its
// own, so that coverage and path support see nothing of it: k_pu_events, enqueued behind k_poa_text on the slot's stream,
// condenses every finished problem into a list (the +1 / -1 events of its runs of MATCHED bases on the linearised graph, then one
// word per mismatch, deleted base and insertion); k_pu_add, once the host has picked the winners, adds the winners' lists to a
// difference array of match depth and to the table of the sparse operations; k_pu_finish, on read, prefix-sums the match depth into
// the column of every base's own letter.
//
// The price of lists of its own is a second copy of code that has to stay in step: k_pu_events repeats k_cov_runs' walk (which
// row opens a node, the offset carried from block to block, runs cut by position) and k_poa_text's query index, k_pu_finish
// k_cov_depth's scan, and pu_call_begin / pu_enqueue_events / pu_add_winners the cov_* functions of the same names.  Whoever
// changes the meaning of an operation, of a row record or of the subgraph store's handles in one of them changes it here too.
#pragma once

#include "vga_common.hpp"
#include "vga_poa_launch.hpp"
#include "vga_subgraph.hpp"

// columns of the table
enum : uint32_t { PU_COL_N = 4u, PU_COL_DEL = 5u, PU_COL_INS = 6u, PU_COLS = 7u };
// a sparse word is position << 3 | column
#define PU_MAX_SEQ (1ull << 29)

// one problem's list: n_match event words (position << 1 | 1 for a -1 event), then n_sparse words, at word `off` of its buffer
struct pu_rec {
    uint32_t off, n_match, n_sparse;
    uint32_t flags;  // low two bits: 0 nothing (the problem has no alignment yet), 1 in the call's device buffer, 2 no room there,
                     // 3 built by the host; bit 2: the alignment starts with an insertion (it belongs to no base)
};
#define PU_LEADING 4u

struct pu_state;
// the context's pileup state while counting is on (vga_pileup_begin), else null
pu_state *pu_active(vga_ctx *ctx);
// start of a poa_run call of n problems whose queries hold total_q bases: the buffer of lists is sized (cap_words caps it when
// has_cap: VGA_PILEUP_LIST_WORDS) and its cursor zeroed
int pu_call_begin(vga_ctx *ctx, pu_state *pu, uint64_t n, uint64_t total_q, bool has_cap, uint64_t cap_words);
// k_pu_events for the nb problems staged on a slot, and the copy of their records into the slot's result set `oset`
hipError_t pu_enqueue_events(vga_ctx *ctx, pu_state *pu, hipStream_t st, int slot, int oset, uint32_t nb, const poa_launch_bufs &b, const uint32_t *ids,
                             const sg_store &store);
// the records of a finished launch (valid once its stream is synchronised)
const pu_rec *pu_launch_recs(const pu_state *pu, int slot, int oset);
// keeps the record of problem p (a later run of the same problem replaces it)
void pu_keep(pu_state *pu, uint32_t p, const pu_rec &r);
// the host route for a problem whose list found no room: the same list from the operations as they came back (stored sink ->
// source); bases[r - 1] is the base of graph row r, query the sequence that was aligned
void pu_keep_from_ops(pu_state *pu, uint32_t p, const uint8_t *ops, const uint32_t *orow, uint32_t nops, const uint32_t *first_row, uint32_t n_nodes,
                      const uint32_t *handles, const std::vector<uint32_t> &node_start, const char *bases, uint32_t n_rows, const char *query);
// k_pu_add over the lists of the winners (problem indices of the call that just ended), on the context's stream; waits for it
int pu_add_winners(vga_ctx *ctx, pu_state *pu, const std::vector<uint32_t> &winners);
// k_pu_finish on the context's stream, not waited for: the table vga_pileup_read copies out (seq_length x PU_COLS), left on the
// device for vga_variant.hip.  VGA_ERR_UNSUPPORTED once a 32-bit counter may have wrapped.
int pu_finish_device(vga_ctx *ctx, pu_state *pu, const char *who, const uint32_t **table, uint32_t *seq_length);
