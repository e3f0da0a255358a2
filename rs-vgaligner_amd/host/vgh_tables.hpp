// vgh_tables.hpp -- the per-run analysis tables of `vgaligner map` (--coverage, --path-support, --pileup, --genotype,
// --genotype-likelihood, --path-edit, --call-variants, --call-insertions, --call-deletions, --phase, --haplotag, --haplotype-calls, --phase-join, --haplotype-paths, --path-abundance): what a context has counted and scored, added over the contexts in 64 bits,
// and the TSV files.  Internal to the host library: map_chunk, map_reads and map_reads_multi (vgh_map.cpp) drive one Tables per
// context through begin .. write and know nothing of the single analyses.
#pragma once

#include "vgh.hpp"

#include <functional>

namespace vgh {

inline void put_u64(std::string &s, uint64_t v)
{
    char t[24];
    int n = 0;
    do { t[n++] = (char)('0' + v % 10); v /= 10; } while (v);
    while (n) s.push_back(t[--n]);
}

void write_file(const std::string &name, const std::string &body);

// A few vectors of 64-bit counters and two scalar counts.  A table nothing was read into (a device slot that got no read) has no
// vectors at all: add() grows to the larger side and pad() fills up to the sizes a writer indexes.
struct Counters {
    std::vector<std::vector<uint64_t>> v;
    uint64_t n[2] = {0, 0};
    void add(const Counters &o);
    void pad(const std::vector<size_t> &sizes);
};

// The variant calls as the library returns them (MapOptions::call_variants)
struct VariantCalls {
    std::vector<uint32_t> pos, qual;
    std::vector<uint8_t> gt;
    std::vector<uint64_t> ins_qual, depth, counts;  // counts: 7 per call
    uint64_t n_tested = 0, n_calls = 0;
};

// The insertion calls at the sites of VariantCalls whose insertion state is het or hom, in that order (MapOptions::call_insertions)
struct InsertionCalls {
    std::vector<uint64_t> site;  // index into the variant calls
    std::vector<uint8_t> length, seq;            // seq: 8 per site
    std::vector<uint64_t> length_reads, seq_reads;  // seq_reads: 8 per site
};

// The deletion events (MapOptions::call_deletions): three words per event, of this context's store or of the concatenated stores
// (kept only for the route of several contexts; the counts are kept either way), and the calls in sort order
struct DeletionCalls {
    std::vector<uint32_t> events;
    uint64_t n_alignments = 0, n_events = 0, n_end_runs = 0;
    std::vector<uint32_t> first, len, last, qual;
    std::vector<uint8_t> state;
    std::vector<uint64_t> depth, reads;
    uint64_t n_distinct = 0, n_calls = 0;
};

// The heterozygous sites of VariantCalls in that order, and their links (MapOptions::phase)
struct PhaseLinks {
    std::vector<uint32_t> pos;
    std::vector<uint8_t> x, y;
    std::vector<uint32_t> links, site_reads;  // 32 and 3 per site
    uint64_t n_reads = 0;
    // the chain on the links (ph_chain), per site
    std::vector<uint32_t> ps;
    std::vector<uint8_t> flip, link_d;
    void chain(uint32_t min_links);
};
// The phase stores of several contexts, concatenated: three words per read (off, n_runs, n_sparse) and the words
struct PhaseStore {
    std::vector<uint32_t> recs, words;
    void add(const PhaseStore &o);
};
// The number in the input file of every kept read, in store order, and the haplotype tags: four words per row (read, ps, votes_a,
// votes_b), the read an index into the store until Tables::write numbers it by the input file (MapOptions::haplotag)
struct PhaseTags {
    std::vector<uint64_t> read_ids;
    std::vector<uint32_t> rows;
    uint64_t n_rows = 0;
};
// The haplotype counts: sixteen words per job (c: an index into VariantCalls, ps, a[0 .. 6], b[0 .. 6]), in job order
// (MapOptions::haplotype_calls)
struct HaplotypeCounts {
    std::vector<uint32_t> rows;
    uint64_t n_rows = 0;
};

// The set links of the chain's sets and what the join rule makes of them (MapOptions::phase_join): the table of four counters per
// pair of sets, per chain set its name, the set that names its component and its parity against it, the accepted links (s, t, cis,
// trans), and per site the joined ps and flip that the tags and the haplotype counts take in the place of the chain's
struct PhaseJoin {
    std::vector<uint32_t> table, set_ps, set_root, joins;
    std::vector<uint8_t> set_flip;
    uint64_t n_sets = 0, n_joins = 0, n_agree = 0, n_conflict = 0;
    std::vector<uint32_t> ps;
    std::vector<uint8_t> flip;
};

// The haplotype paths (MapOptions::haplotype_paths): the deficit rows of the kept reads, dense, and their scored bytes, in store
// order (kept whole only for the route of several contexts; the scored reads are counted either way); per group 2 s + h the reads
// and per (group, path) the entry (cost, best)
struct HapPaths {
    std::vector<uint8_t> deficits, scored;
    uint64_t n_scored = 0;
    std::vector<uint64_t> reads, table;
    uint64_t n_sets = 0;
};

// The path abundance (MapOptions::path_abundance): the deficit rows of the reported alignments, dense, and their scored bytes (kept
// only for the route of several contexts), the rows kept, and the estimate
struct Abundance {
    std::vector<uint8_t> deficits, scored;
    uint64_t n_kept = 0, n_scored = 0;
    std::vector<uint32_t> theta;
    std::vector<uint64_t> reads_q16, best;
    uint32_t iterations = 0, converged = 0;
};

// The per-read lines of <out>-path-support-reads.tsv and <out>-path-edit-reads.tsv, in read order
struct ReadRows {
    std::string path, edit;
    void operator+=(const ReadRows &o) { path += o.path; edit += o.edit; }
};

// the options are refused here when they contradict each other (before any device is opened)
void check_aligner(const MapOptions &opt);

class Tables {
public:
    // `ix` and `opt` outlive the object
    Tables(const Index &ix, const MapOptions &opt);

    // Which analyses run.  Each of --genotype, --genotype-likelihood and --path-edit turns the scoring on, not its files; the
    // likelihood from the edit distance turns that on; --call-variants turns the counting of the pileup on, not its file.
    bool coverage() const { return opt_.coverage || opt_.coverage_only; }
    bool scoring() const { return scoring_on(opt_); }
    bool edit() const { return opt_.path_edit || (opt_.genotype_likelihood && opt_.genotype_from_edit) || (opt_.haplotype_paths && opt_.haplotype_paths_from_edit) ||
                              (opt_.path_abundance && opt_.abundance_from_edit); }
    bool piling() const { return opt_.pileup || opt_.call_variants; }
    bool inserting() const { return opt_.call_insertions; }
    bool deleting() const { return opt_.call_deletions; }
    bool phasing() const { return opt_.phase; }
    bool tagging() const { return opt_.haplotag; }
    bool hap_calling() const { return opt_.haplotype_calls; }
    bool joining() const { return opt_.phase_join; }
    bool hap_typing() const { return opt_.haplotype_paths; }
    bool abundance() const { return opt_.path_abundance; }
    bool any() const { return coverage() || scoring() || piling() || inserting(); }  // (phasing needs piling)
    // --call-variants over several contexts: they hand their pileup tables over, and the first calls from the sum (call());
    // --path-abundance likewise: they hand their stores over, and the first estimates from the concatenated rows
    bool call_summed(uint32_t n_contexts) const { return (opt_.call_variants || opt_.path_abundance) && n_contexts > 1; }

    // turns the analyses on, on a context that holds the index
    void begin(vga_ctx *ctx) const;
    // the rows of reads [b0, b0 + n), the most recent vga_align_batch of ctx, while the context still holds them (`aligned`: of that
    // call's result; mark(what): a trace mark after each of the two tables).  The reads of the call that the phase store has kept
    // are noted by their number.
    void chunk_rows(vga_ctx *ctx, uint64_t b0, uint64_t n, const uint8_t *aligned, ReadRows &rows, const std::function<void(const char *)> &mark);
    // What the context has counted and scored so far joins this object.  call_now: the variants are called from the context's own
    // counters, and the insertions at their sites, and the heterozygous sites are linked, the reads tagged and the haplotypes counted from its own store; otherwise its pileup
    // table, its insertion table and its whole phase store are kept for the sum.  (`slot` names the context in the trace.)
    void take(vga_ctx *ctx, uint32_t slot, bool call_now);
    // turns the analyses off on a context that stays with the caller
    void end(vga_ctx *ctx) const;
    void add(const Tables &o);
    // the variants of the summed pileup table, and the insertions at their sites from the summed insertion table, called on `ctx`
    // and the links of the heterozygous sites, the reads' tags and the haplotype counts from the concatenated stores (any context: its own counters are not touched);
    // the path abundance from the concatenated rows
    void call(vga_ctx *ctx);
    // the TSV files beside the GAF files (out_prefix == "": none) and the fields of `out`
    void write(MapOutput &out, const ReadRows &rows, const std::string &out_prefix);

private:
    const Index &ix_;
    const MapOptions &opt_;
    Counters coverage_;  // base, node, edge; n: alignments
    Counters paths_;     // sum_bases, sum_edges, top, top_alone; n: alignments, unplaced
    Counters pairs_;     // sum_bases, sum_edges, prefer_a, prefer_b at vga_pair_index
    Counters costs_;     // cost at vga_pair_index, in 1/256 bit; n: rows scored
    Counters edit_;      // n_scored, sum_edit, best, best_alone; n: alignments, too long
    Counters pileup_;    // seq_length x 7; n: alignments, leading insertions
    VariantCalls variants_;
    Counters insertions_;  // seq_length x 49; n: alignments, leading insertions (only kept for the sum of several contexts)
    InsertionCalls ins_calls_;
    DeletionCalls deletions_;
    PhaseStore phase_store_;  // (only kept for the route of several contexts)
    PhaseLinks phase_;
    PhaseTags tags_;  // (read_ids: of this context's store, then of the concatenated stores)
    HaplotypeCounts hap_counts_;
    PhaseJoin join_;
    HapPaths hap_paths_;
    Abundance abundance_;
    // the sets the tags and the haplotype counts work on: the joined ones under --phase-join, else the chain's
    const std::vector<uint32_t> &sets_ps() const { return joining() ? join_.ps : phase_.ps; }
    const std::vector<uint8_t> &sets_flip() const { return joining() ? join_.flip : phase_.flip; }
    // the heterozygous variant calls as sites; sizes the tables of phase_
    void phase_sites();
    // the positions of the variant calls whose insertion state is het or hom; fills ins_calls_.site and sizes its arrays
    std::vector<uint32_t> insertion_sites();
};

}  // namespace vgh
