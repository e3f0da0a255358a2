// vga_phase_join.hpp -- which phase sets of the chain go together, by the reads that are tagged in both (vga_phase_set_links*,
// k_sj_bits and k_sj_pairs in vga_phase.hip), and the rule that joins them.
//
// Nothing in the reference stands behind this.  The chain (vga_phase.hpp: ph_chain) links sites at most PH_WINDOW apart in site
// order and joins nothing again; a read of 10 kbp crosses far more sites than that and is tagged in several sets at once.  tag(r, s)
// is a for votes_a > votes_b of the haplotag row (r, s), b for votes_b > votes_a, nothing otherwise (k_hc_tags, unchanged).  The
// table holds, for every pair of sets s <= t (the S sets of the chain in ascending ps, rows in vga_pair_index(S, s, t) order), the
// PJ_COLS counters n[2 i + j]: the kept reads with tag(r, s) = i and tag(r, t) = j, 0 for a and 1 for b.  On the diagonal n[0] and
// n[3] are the reads tagged a and b in the set, n[1] = n[2] = 0.  The measure is defined on the alignments GAF and the rows of
// <out>-variants.tsv alone (tests/phase_join_ref.py recomputes it).
//
// The constants and the join rule are shared by host and device code; this header is plain C++ and compiles alone with a host
// compiler (tests/test_phase_join_cpu.py does that).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <vector>

#include "vga_pair_index.hpp"

// a row of the table: (a, a), (a, b), (b, a), (b, b)
#define PJ_COLS 4u
// the sets of one vga_phase_set_links: the table is 134 MB there
#define PJ_MAX_SETS 4096u
// --phase-join-min-reads: a choice, not a measurement (README, "Phase join")
#define PJ_MIN_READS_DEFAULT 2u
#define PJ_MIN_READS_MAX 65535u
// k_sj_bits: a wave per word of 64 reads and PJ_BITS_SETS sets, a set per lane at the store.  k_sj_pairs: a workgroup owns
// PJ_TILE x PJ_TILE pairs of sets and stages PJ_CHUNK_ROWS bit rows of both ranges at a time (a row: the 64-bit word "tagged a" or
// "tagged b" of 64 reads for every set; PJ_CHUNK_ROWS / 2 words, 1024 reads)
#define PJ_BITS_SETS 64u
#define PJ_TILE 32u
#define PJ_CHUNK_ROWS 32u

// an accepted link as vga_phase_join returns it: s, t, cis, trans
#define PJ_JOIN_COLS 4u

// The join, integer-only: the one definition (vga_phase_join exports it, Tables::write prints from it).  table: the
// vga_pair_count(S) rows of PJ_COLS counters.  For s < t: cis = n[0] + n[3], trans = n[1] + n[2], diff = |cis - trans|; the pair
// is a link when diff >= min_reads (min_reads >= 1: cis = trans is never a link).  The links are taken by diff descending, then s
// ascending, then t ascending.  A link whose sets are in different components at its turn joins them, the haplotypes related
// trans when trans > cis, else cis, and is written to joins (s, t, cis, trans; at most S - 1 of them); a link inside one component
// joins nothing and is counted as agreeing or conflicting with the orientation the component already implies.  set_root[s]: the
// smallest set of the component of s, which keeps its orientation; set_flip[s]: the parity of s against it.  A link is accepted
// exactly when its ends are in different components, so the result does not depend on how the components are kept.
static inline void pj_join(uint64_t S, const uint32_t *table, uint32_t min_reads, uint32_t *set_root, uint8_t *set_flip, uint32_t *joins, uint64_t *n_joins,
                           uint64_t *n_agree, uint64_t *n_conflict)
{
    struct link {
        uint32_t diff, s, t;
    };
    const auto counts = [&](uint64_t s, uint64_t t, uint64_t &cis, uint64_t &trans) {
        const uint32_t *n = table + vga_pair_index(S, s, t) * PJ_COLS;
        cis = (uint64_t)n[0] + n[3];
        trans = (uint64_t)n[1] + n[2];
    };
    std::vector<link> links;
    for (uint64_t s = 0; s < S; s++)
        for (uint64_t t = s + 1; t < S; t++) {
            uint64_t cis, trans;
            counts(s, t, cis, trans);
            const uint64_t diff = cis > trans ? cis - trans : trans - cis;
            if (diff == 0 || diff < min_reads) continue;
            links.push_back(link{(uint32_t)std::min<uint64_t>(diff, 0xFFFFFFFFull), (uint32_t)s, (uint32_t)t});
        }
    std::stable_sort(links.begin(), links.end(), [](const link &a, const link &b) { return a.diff > b.diff; });  // (made in (s, t) order)
    // up[s]: a set of the component of s nearer to its smallest set (itself: s is that set); par[s]: the parity of s against up[s]
    std::vector<uint32_t> up(S);
    std::vector<uint8_t> par(S, 0);
    for (uint64_t s = 0; s < S; s++) up[s] = (uint32_t)s;
    const auto find = [&](uint32_t s, uint8_t &parity) {
        uint32_t root = s;
        uint8_t p = 0;
        while (up[root] != root) { p ^= par[root]; root = up[root]; }
        parity = p;
        while (up[s] != root) {  // every set on the way hangs on the root from now on
            const uint32_t next = up[s];
            const uint8_t rest = (uint8_t)(p ^ par[s]);
            up[s] = root; par[s] = p;
            s = next; p = rest;
        }
        return root;
    };
    *n_joins = *n_agree = *n_conflict = 0;
    for (const link &l : links) {
        uint64_t cis, trans;
        counts(l.s, l.t, cis, trans);
        const uint8_t rel = trans > cis ? 1u : 0u;
        uint8_t ps = 0, pt = 0;
        const uint32_t rs = find(l.s, ps), rt = find(l.t, pt);
        if (rs == rt) {
            ((ps ^ pt) == rel ? *n_agree : *n_conflict)++;
            continue;
        }
        const uint32_t keep = std::min(rs, rt), hang = std::max(rs, rt);  // the smallest set names the component
        up[hang] = keep;
        par[hang] = (uint8_t)(ps ^ pt ^ rel);
        uint32_t *j = joins + *n_joins * PJ_JOIN_COLS;
        j[0] = l.s; j[1] = l.t; j[2] = (uint32_t)cis; j[3] = (uint32_t)trans;
        (*n_joins)++;
    }
    for (uint64_t s = 0; s < S; s++) {
        uint8_t p = 0;
        set_root[s] = find((uint32_t)s, p);
        set_flip[s] = p;
    }
}

// The joined sets per site.  ps[h] names the site that opens the chain set of h (1-based, at or before h; the k-th opening site
// opens set k).  ps_out[h]: the name of the set that names the component of the set of h -- again a site that opens its set, at
// or before h; flip_out[h] = flip[h] xor set_flip[set of h].  -> the number of chain sets.
static inline uint64_t pj_sites(uint64_t n_sites, const uint32_t *ps, const uint8_t *flip, const uint32_t *set_root, const uint8_t *set_flip, uint32_t *ps_out,
                                uint8_t *flip_out)
{
    std::vector<uint32_t> set_of(n_sites), set_ps;  // set_of[h]: the set that site h opens
    for (uint64_t h = 0; h < n_sites; h++)
        if (ps[h] == h + 1u) { set_of[h] = (uint32_t)set_ps.size(); set_ps.push_back((uint32_t)(h + 1u)); }
    for (uint64_t h = 0; h < n_sites; h++) {
        const uint32_t s = set_of[ps[h] - 1u];
        ps_out[h] = set_ps[set_root[s]];
        flip_out[h] = (uint8_t)(flip[h] ^ set_flip[s]);
    }
    return set_ps.size();
}
