// vga_phase.hpp -- which alleles of the heterozygous variant calls travel together on the reads (vga_phase.hip), as the pileup
// and the host see it, and which stored reads go with which haplotype of the sets the chain forms (k_ph_tag, k_ph_tag_scan).
//
// Nothing in the reference stands behind this.  The variant call (vga_variant.hpp) reports independent diploid sites; a read of
// 10 kbp crosses many of them, so the linkage is in the alignments.  The sites are known only once the last read has been piled
// up, and the operations are gone by then: what stays is the pileup's list of every reported alignment (vga_pileup.hpp), which
// holds exactly what an observation needs.  While the store is on, k_ph_keep copies the winners' lists of every vga_align_batch
// into a grow-only store of the context; vga_phase_links then runs k_ph_obs (what each stored read shows at each site) and
// k_ph_link (the pair counts of sites up to PH_WINDOW apart) over tiles of reads.  The measure is defined on the alignments GAF
// and the rows of <out>-variants.tsv alone (tests/phase_ref.py recomputes it).
// vga_phase_tags runs k_ph_obs again and, behind it, k_ph_tag (count), k_ph_tag_scan and k_ph_tag (emit): one row per (read, set)
// in which a site votes, the votes for haplotype a and for haplotype b (tests/haplotag_ref.py recomputes them).
//
// The constants, the word formats and the chain rule are shared by host and device (and read by tests/test_phase_cpu.py).
#pragma once

#include <stdint.h>

// sites further apart than this in site order are not linked: a choice, not a measurement (README, "Phase")
#define PH_WINDOW 8u
// link[h][d - 1][2 a + b], d = 1 .. PH_WINDOW: the reads with observation a at site h and b at site h + d
#define PH_LINK_COLS 4u
#define PH_LINK_ROW 32u
// per site: the reads that show x, y, anything else
#define PH_SITE_COLS 3u
// a stored read: `n_runs` run-event words at word `off` of the store, then `n_sparse` sparse words.
//   run-event words come in pairs: position << 1 where a run of matched bases starts, (position behind its last base) << 1 | 1
//     where it ends -- the start word at p covers p, the end word at p does not;
//   a sparse word is position << 3 | column: 0 .. 3 the read shows A C G T at the base, 4 another letter, 5 the base is deleted,
//     6 an insertion behind the base (not an observation of the base: ignored).
struct ph_rec {
    uint32_t off, n_runs, n_sparse;
};
#define PH_COL_OTHER 4u
#define PH_COL_DEL 5u
#define PH_COL_INS 6u
#define PH_COLS 7u
// alleles A < C < G < T < D; the own letter of a base that is none of A C G T is PH_REF_OTHER
#define PH_ALLELE_DEL 4u
#define PH_REF_OTHER 4u
// the own letter of a graph base as the links take it: 0 .. 3 for a c g t in either case, PH_REF_OTHER for anything else
static inline uint8_t ph_ref_of(char c)
{
    const char l = (char)(c | 0x20);
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : (uint8_t)PH_REF_OTHER;
}
// positions share a word with three bits; the store is indexed in 32 bits
#define PH_MAX_SEQ (1ull << 29)
#define PH_MAX_WORDS 0xFFFFFFFFull
#define PH_MAX_SITES (1ull << 24)
// --phase-min-links
#define PH_MIN_LINKS_DEFAULT 2u
#define PH_MIN_LINKS_MAX 65535u
// the three bits of (site, read) in the observation tile, one byte each: the read shows x, y, anything else at the base
#define PH_SAW_X 1u
#define PH_SAW_Y 2u
#define PH_SAW_OTHER 4u
// the observation tile in HBM: reads x sites bytes at most (the reads a multiple of 64), the grow-only store's first size in
// words, the threads of k_ph_link's workgroup
#define PH_TILE_BYTES (64ull << 20)
#define PH_STORE_WORDS0 (1ull << 20)
#define PH_LINK_BLOCK 256u
// the haplotype tags (vga_phase_tags): a row is read, ps, votes_a, votes_b; the threads of k_ph_tag's workgroup (a read per lane)
// and of k_ph_tag_scan's one workgroup
#define PH_TAG_COLS 4u
#define PH_TAG_BLOCK 64u
#define PH_SCAN_BLOCK 1024u

// The chain, integer-only: the one definition (vga_phase_chain exports it, Tables::write prints from it).  links: n x 8 x 4.
// For h in order the smallest d in 1 .. min(PH_WINDOW, h) whose link[h - d][d - 1] has cis = l[0] + l[3] and trans = l[1] + l[2]
// that differ by at least min_links joins h to the set of h - d, flipped when trans > cis; else h opens a set numbered h + 1,
// its own line among the sites.
static inline void ph_chain(uint64_t n, const uint32_t *links, uint32_t min_links, uint32_t *ps, uint8_t *flip, uint8_t *link_d)
{
    for (uint64_t h = 0; h < n; h++) {
        ps[h] = (uint32_t)(h + 1u);
        flip[h] = 0;
        link_d[h] = 0;
        for (uint32_t d = 1; d <= PH_WINDOW && d <= h; d++) {
            const uint32_t *l = links + ((h - d) * PH_WINDOW + (d - 1u)) * PH_LINK_COLS;
            const uint64_t cis = (uint64_t)l[0] + l[3], trans = (uint64_t)l[1] + l[2];
            const uint64_t diff = cis > trans ? cis - trans : trans - cis;
            if (diff == 0 || diff < min_links) continue;
            ps[h] = ps[h - d];
            flip[h] = (uint8_t)(flip[h - d] ^ (trans > cis ? 1u : 0u));
            link_d[h] = (uint8_t)d;
            break;
        }
    }
}

#ifdef __HIPCC__
#include "vga_oplist.hpp"

static_assert(PH_LINK_ROW == PH_WINDOW * PH_LINK_COLS, "the links of a site");

struct ph_state;
// the context's phase store while it is on (vga_phase_begin, with the pileup counted), else null
ph_state *ph_active(vga_ctx *ctx);
// k_ph_keep: the lists of the nw winners that the pileup's add step (pu_add) has just staged (lists.d_win / h_win, the device lists and the
// host-built ones) join the store, on the context's stream; not waited for.  VGA_ERR_NOMEM when the store cannot grow.
int ph_keep_winners(vga_ctx *ctx, ph_state *ph, const oplist_call &lists, size_t nw);
// the reads the store holds
uint64_t ph_kept_reads(const ph_state *ph);
// The deficit store of the haplotype paths (vga_hap_paths.hpp) belongs to the phase store: a row per kept read, emptied and released
// with it.  Empty until vga_haplotype_paths_begin makes it.
struct hp_state;
vga_owned<hp_state> &ph_hap_paths(ph_state *ph);
#endif
