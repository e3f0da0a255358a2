// vga_insertion.hpp -- the letters reads insert behind a graph base (vga_insertion.hip), as poa_run and vga_align_batch see it.
//
// Nothing in the reference stands behind this.  The pileup (vga_pileup.hpp) counts THAT reads insert behind a base, in one column;
// this table keeps how long the inserted runs are and what their first letters are, so that a site the variant call reports with an
// insertion can be given its allele without the cs strings being parsed again.  It is defined on the record the alignments GAF
// reports for a read and can be recomputed from that text alone (tests/insertion_ref.py).  It is the third list maker of
// vga_oplist.hpp, with lists and buffers of its own: k_ia_events, enqueued behind k_poa_text on the slot's stream, condenses every
// finished problem into one event per run of I operations that has a base before it; k_ia_add, once the host has picked the
// winners, adds the winners' events to the table; k_ia_call calls length and letters of the sites it is asked for.
//
// The constants are shared by host and device (and read by tests/test_insertion_cpu.py).
#pragma once

// the letters of a run that are kept: a choice, not a measurement (README, "Insertion call")
#define IA_MAX_LEN 8u
// 32-bit counters per graph base: the bins of length 1 .. 8 and `more`, then per kept position the letters A C G T N
#define IA_LETTERS 5u
#define IA_BINS 9u
#define IA_COLS 49u
// a position shares a word with the bin, and the table is indexed in 32 bits
#define IA_MAX_SEQ (1ull << 26)
// one event: position << 4 | bin (1 .. 9, 9 = more), then the 3-bit codes of the kept letters from bit 0 up (0 .. 4 = A C G T N,
// IA_NO_LETTER behind the run's last)
#define IA_EVENT_WORDS 2u
#define IA_NO_LETTER 7u
// vga_insertion_call_table serves counters below this (vga_variant_call_table's bound)
#define IA_MAX_COUNT (1ull << 40)
#define IA_BLOCK 256u

#ifdef __HIPCC__
#include "vga_oplist.hpp"

static_assert(IA_COLS == IA_BINS + IA_MAX_LEN * IA_LETTERS && IA_BINS == IA_MAX_LEN + 1u, "the row of a base");
static_assert(IA_MAX_LEN * 3u <= 32u && IA_MAX_SEQ * 16ull <= (1ull << 32) && IA_MAX_SEQ * IA_COLS <= (1ull << 32), "the event words and the index");

// one problem's list (vga_oplist.hpp): n_a words, IA_EVENT_WORDS per event, and no words of a second kind; flags 0 to 3, and
// PU_LEADING for a run of insertions with no base before it
using ia_rec = oplist_rec;

// all that poa_run and vga_align_batch see of it (vga_oplist.hpp: the frame of a list maker)
const oplist_maker &ia_maker();
#endif
