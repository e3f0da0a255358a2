// vga_deletion.hpp -- deletions of several graph bases as one event each (vga_deletion.hip), as poa_run and vga_align_batch see it,
// and the one definition of the call.
//
// Nothing in the reference stands behind this.  The pileup (vga_pileup.hpp) counts a deleted base where it lies and
// vga_variant_call calls every base alone, so a deletion of ten bases is ten `-` calls.  Here a maximal run of D operations of the
// reported record of a read -- one "-g.." token of its cs string -- is one event (first, len, last): the positions on the
// linearised graph of its first and last deleted base and the number of bases.  last - first != len - 1 when the run crosses
// nodes, and the same (first, len) may end at two places through a bubble, so all three words are the identity.  A run with no M
// operation (":" or "*" token) before it, or none behind it, is an end run: the alignment is global over its subgraph, so such a
// run says where the subgraph ends and nothing about the sample; it is counted and otherwise ignored.  It is the fourth list
// maker of vga_oplist.hpp: k_dl_events lists the events of every finished problem, k_dl_keep appends those of the reported
// alignments to a grow-only store of the context, and vga_deletion_call sorts, groups, counts and calls them on the device.  It is
// defined on the alignments GAF text, the node starts and the pileup table alone (tests/deletion_ref.py recomputes it).
//
// The constants and the rule are shared by host and device; down to the #ifdef this header is plain C++ and compiles alone with a
// host compiler (tests/test_deletion_cpu.py reads the constants and the host driver prints with the state names).
#pragma once

#include <stdint.h>

// an event of the store: first, len, last
#define DL_EVENT_WORDS 3u
// the grow-only store's first size in events (it doubles from there): a choice, small enough that a few hundred reads pass it
#define DL_STORE_EVENTS0 1024ull
// the store holds fewer words than this, and a call takes fewer events (the sort's payload is a 32-bit index)
#define DL_MAX_WORDS 0xFFFFFFFFull
#define DL_MAX_EVENTS 0xFFFFFFFFull
// a 64-bit counter of an explicit pileup table (vga_deletion_call_table) stays below this (vga_variant_call_table's bound)
#define DL_MAX_COUNT (1ull << 40)
// the states of a call, in the order in which a tie is decided
#define DL_NONE 0u
#define DL_HET 1u
#define DL_HOM 2u
// threads of a workgroup of the call's element-wise kernels
#define DL_BLOCK 256u

#if defined(__HIPCC__)
#define DL_HD __host__ __device__
#else
#define DL_HD
#endif

// The rule, integer-only: the one definition (vga_deletion_state exports it).  `reads` alignments hold the event, `depth` cover
// or delete its first base, E is the cost of an observation that no allele explains (--call-error, 1/256 bit).  With
// k = min(reads, depth):  none costs k E,  het 256 depth,  hom (depth - k) E;  the first minimum in that order is the state and
// *qual the second smallest cost minus the smallest, saturated at 2^32 - 1.  This is the insertion-state rule of
// vga_variant_call.  depth < 6 * 2^40 and E <= 8192 keep every product far below 2^64.
static inline DL_HD uint32_t dl_rule(uint64_t reads, uint64_t depth, uint32_t E, uint32_t *qual)
{
    const uint64_t k = reads < depth ? reads : depth;
    const uint64_t c0 = k * E, c1 = 256ull * depth, c2 = (depth - k) * E;
    uint32_t state = DL_NONE;
    uint64_t best = c0;
    if (c1 < best) { best = c1; state = DL_HET; }
    if (c2 < best) { best = c2; state = DL_HOM; }
    const uint64_t lo01 = c0 < c1 ? c0 : c1, hi01 = c0 < c1 ? c1 : c0;
    const uint64_t second = c2 <= lo01 ? lo01 : (c2 < hi01 ? c2 : hi01);  // the median of the three
    const uint64_t q = second - best;
    *qual = q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q;
    return state;
}
// a group is reported when its first base is deep enough, the event is called and the call is sure enough
static inline DL_HD bool dl_reported(uint32_t state, uint32_t qual, uint64_t depth, uint64_t min_depth, uint64_t min_qual)
{
    return depth >= min_depth && state != DL_NONE && (uint64_t)qual >= min_qual;
}
static inline const char *dl_state_name(uint32_t state) { return state == DL_HET ? "het" : state == DL_HOM ? "hom" : "none"; }

#ifdef __HIPCC__
#include "vga_oplist.hpp"

// one problem's list (vga_oplist.hpp): n_a words, DL_EVENT_WORDS per event, and no words of a second kind; flags 0 to 3 in the
// low two bits and the number of the record's end runs above them
using dl_rec = oplist_rec;
#define DL_END_SHIFT 2u

struct dl_state;
// all that poa_run and vga_align_batch see of it (vga_oplist.hpp: the frame of a list maker)
const oplist_maker &dl_maker();
#endif
