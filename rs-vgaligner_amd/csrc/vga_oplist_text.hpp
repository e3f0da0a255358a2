// vga_oplist_text.hpp -- the words of the list makers (vga_oplist.hpp): what each is called in an error, in the traces and in the
// refusal of the host route, and the one copy of every error text their entry points share.  An entry point hands in its own name
// (__func__), so no text names a function by hand.  Plain C++: no HIP type or call, so that a host compiler builds it alone
// (tests/test_oplist_text_cpu.py pins every text against the literal it replaced).
#pragma once

struct oplist_text {
    const char *name;        // its entry points are vga_<name>_begin / _reset / _end / _read
    const char *who, *what;  // the maker and its list, in the error for a reported alignment without a list
    const char *list;        // as poa_run's trace calls its list
    const char *mark;        // its line of vga_align_batch's trace
    const char *refusal;     // what vga_align_batch refuses under VGA_SUBGRAPH=host while it is on
    const char *limit;       // the positions a graph has to fit for it
};
static const oplist_text OPLIST_TEXT_COV = {"coverage", "coverage", "run", "run list", "coverage", "read coverage is not counted", "32-bit"};
static const oplist_text OPLIST_TEXT_PU = {"pileup", "pileup", "event", "pileup list", "pileup", "the pileup is not counted", "29-bit"};
static const oplist_text OPLIST_TEXT_DL = {"deletion", "deletions", "deletion", "deletion list", "deletions", "the deletion events are not kept", "29-bit"};
static const oplist_text OPLIST_TEXT_IA = {"insertion", "insertions", "insertion", "insertion list", "insertions", "the inserted letters are not counted", "26-bit"};
#define OPLIST_REFUSAL_PATHS "path support is not scored"  // (no maker: it reads coverage's lists, and is refused and scored right behind coverage)

// the formats; the first %s of each is the entry point
#define OPLIST_ERR_NO_INDEX "%s: no index uploaded"
#define OPLIST_ERR_TOO_LARGE "%s: graph too large for %s positions"                               // oplist_text::limit
#define OPLIST_ERR_NO_MEMORY "%s: out of host memory"
#define OPLIST_ERR_RESERVE "%s: %s"                                                               // hipGetErrorString
#define OPLIST_ERR_OFF "%s: counting is off (vga_%s_begin)"                                        // oplist_text::name
#define OPLIST_ERR_WRAPPED "%s: %llu alignments counted: a 32-bit counter may have wrapped"
#define OPLIST_ERR_NO_LIST "%s: reported alignment %zu has no %s list (flags %u)"                  // who, the winner, what, its flags
#define OPLIST_ERR_REFUSED "vga_align_batch: %s under VGA_SUBGRAPH=host (the subgraph handles are then on the host only)"
// ... and of the calls over a table of 64-bit counters (vga_variant_call_table, vga_insertion_call_table)
#define OPLIST_ERR_WIDE "%s: a counter of 2^40 or more"
