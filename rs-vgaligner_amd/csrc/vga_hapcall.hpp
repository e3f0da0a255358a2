// vga_hapcall.hpp -- what the reads of each haplotype of a phase set show at every reported call inside the set's span
// (vga_haplotype_counts*, k_hc_tags, k_hc_cols, k_hc_count in vga_phase.hip), and the haploid call on those counts.
//
// Nothing in the reference stands behind this.  The haplotype tags (vga_phase.hpp) say which kept reads go with haplotype a or b of
// each phase set; this is their consumer.  A read shows column k at base p when it has a sparse word p << 3 | k, or, for k the
// base's own letter (0 .. 3, 4 for anything else), when one of its runs covers p -- at most once per column and base, however often
// it consumes the base.  tag(r, S) is a for votes_a > votes_b of the haplotag row (r, S), b for votes_b > votes_a, nothing otherwise.
// For every call c and set S with first[S] <= cpos[c] <= last[S] (the job rule below) a row of HC_ROW words: c, ps, then per column
// the reads tagged a that show it, then the same for b.  The measure is defined on the alignments GAF, the node starts, the graph's
// letters, the rows of <out>-variants.tsv and the chain's ps / flip alone (tests/haplotype_calls_ref.py recomputes it).
//
// The constants, the job rule and the call rule are shared by host and device code (and read by tests/test_haplotype_calls_cpu.py).
#pragma once

#include <stdint.h>

#include <vector>

// a row: c, ps, a[0 .. 6], b[0 .. 6]; the columns are those of a sparse word (A C G T, other, deleted, inserts behind)
#define HC_ROW 16u
#define HC_COLS 7u
#define HC_COL_DEL 5u
#define HC_COL_INS 6u
// calls and jobs of one vga_haplotype_counts
#define HC_MAX_CALLS (1ull << 24)
#define HC_MAX_JOBS (1ull << 24)
// the threads of k_hc_tags' workgroup (a read per lane, as k_ph_tag) and of k_hc_count's (a job per workgroup, as k_ph_link)
#define HC_TAG_BLOCK 64u
#define HC_COUNT_BLOCK 256u
// the haploid call of hc_call: 0 .. 4 the allele A C G T D, then "?" (no strict majority) and "." (nothing observed); HC_CALL_INS
// is added when more than half of the observing reads insert behind the base
#define HC_CALL_NONE 5u
#define HC_CALL_EMPTY 6u
#define HC_CALL_INS 8u

// The haploid call, integer-only: the one definition (vga_haplotype_call exports it, Tables::write prints from it).  n: the seven
// counts of one haplotype.  obs = n[0] + .. + n[5].  obs = 0: "."; else the first maximum of A, C, G, T, D in that order, which must
// hold 2 n > obs (else "?"); "+" when 2 n[ins] > obs.  There are no parameters: the strict majority is a choice, not a measurement.
static inline uint32_t hc_call(const uint32_t *n)
{
    const uint64_t obs = (uint64_t)n[0] + n[1] + n[2] + n[3] + n[4] + n[HC_COL_DEL];
    if (obs == 0) return HC_CALL_EMPTY;
    const uint32_t of[5] = {n[0], n[1], n[2], n[3], n[HC_COL_DEL]};
    uint32_t best = 0;
    for (uint32_t k = 1; k < 5u; k++)
        if (of[k] > of[best]) best = k;
    return (2ull * of[best] > obs ? best : HC_CALL_NONE) | (2ull * n[HC_COL_INS] > obs ? HC_CALL_INS : 0u);
}

// the call as the file prints it: A C G T, - for D, ? or ., then + or nothing; at most two characters and the 0 behind them
static inline void hc_call_text(uint32_t call, char out[3])
{
    out[0] = "ACGT-?."[(call & 7u) < 7u ? (call & 7u) : 6u];
    out[1] = (call & HC_CALL_INS) ? '+' : 0;
    out[2] = 0;
}

// The jobs, integer-only: the one definition (vga_haplotype_jobs exports it).  cpos ascends strictly, pos ascends strictly, ps[h]
// names the site that opens the set of h (1-based, at or before h), all checked by the caller.  first[S] and last[S] are the
// smallest and largest pos of the sites of S -- the site that opens S and its last site in site order.  A job (c, S) for every call
// with first[S] <= cpos[c] <= last[S]; by c, then by ps ascending.  Returns their number J and writes the first `cap` of them as
// pairs (c, ps).  The sets come in ascending ps, which is ascending first: one sweep over the calls with the open sets kept in that
// order.
static inline uint64_t hc_jobs(uint64_t n_calls, const uint32_t *cpos, uint64_t n_sites, const uint32_t *pos, const uint32_t *ps, uint64_t cap, uint32_t *jobs)
{
    std::vector<uint32_t> last(n_sites), open;  // last[h]: of the set that site h opens; open: the opening sites of the open sets
    for (uint64_t h = 0; h < n_sites; h++) last[ps[h] - 1u] = pos[h];
    uint64_t next = 0, made = 0;  // next: the first site not yet looked at
    for (uint64_t c = 0; c < n_calls; c++) {
        const uint32_t p = cpos[c];
        for (; next < n_sites && pos[next] <= p; next++)
            if (ps[next] == next + 1u) open.push_back((uint32_t)next);
        size_t kept = 0;
        for (size_t k = 0; k < open.size(); k++)
            if (last[open[k]] >= p) open[kept++] = open[k];
        open.resize(kept);
        for (size_t k = 0; k < kept; k++, made++)
            if (made < cap) {
                jobs[2u * made] = (uint32_t)c;
                jobs[2u * made + 1u] = open[k] + 1u;
            }
    }
    return made;
}
