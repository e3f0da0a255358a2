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
// What the pileup shares with coverage -- the walk over the operations on the device and on the host, the record of a list and
// the per-call store of lists -- has one copy, in vga_oplist.hpp, and so has the host frame of a maker: poa_run and
// vga_align_batch reach the pileup through pu_maker().  Here is what is the pileup's own.
#pragma once

#include "vga_oplist.hpp"

// columns of the table
enum : uint32_t { PU_COL_N = 4u, PU_COL_DEL = 5u, PU_COL_INS = 6u, PU_COLS = 7u };
// a sparse word is position << 3 | column
#define PU_MAX_SEQ (1ull << 29)

// one problem's list (vga_oplist.hpp): n_a event words of its runs of matches (position << 1 | 1 for a -1 event), then n_b sparse
// words; flags 0 to 3, and PU_LEADING
using pu_rec = oplist_rec;

struct pu_state;
const oplist_maker &pu_maker();
// the context's pileup state while counting is on (vga_pileup_begin), else null
pu_state *pu_active(vga_ctx *ctx);
// k_pu_finish on the context's stream, not waited for: the table vga_pileup_read copies out (seq_length x PU_COLS), left on the
// device for vga_variant.hip.  VGA_ERR_UNSUPPORTED once a 32-bit counter may have wrapped.
int pu_finish_device(vga_ctx *ctx, pu_state *pu, const char *who, const uint32_t **table, uint32_t *seq_length);
