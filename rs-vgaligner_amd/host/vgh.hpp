// vgh.hpp -- C++ host side of the MI355X vgaligner: everything around the C ABI of libvga_hip.so.
//
// Mirrors the reference's public interface for the map -> chain -> align path (same names, argument
// meaning and error behaviour; panics become vgh::Error):
//   HashGraph / from_gfa ........ handlegraph 0.5.0 + gfa 0.8.0 as used at src/subcommands/index_main.rs:72-74
//   Index::build ................ src/index.rs:109-281 (+ src/utils.rs:81-146, src/kmer.rs:277-505, 816-928,
//                                 src/dna.rs:5-33)
//   read_seqs_from_file ......... src/io.rs:74-162
//   map_reads ................... src/map.rs:27-216   (anchors/chains/alignments come from the GPU)
//   GAFAlignment ................ src/align.rs:746-1028, 1096-1168
//   CLI ......................... src/subcommands/cli.yml, index_main.rs, map_main.rs
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/vga_hip.h"

namespace vgh {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

typedef uint64_t Handle;  // (id << 1) | is_reverse
inline Handle pack(uint64_t id, bool rev) { return (id << 1) | (rev ? 1u : 0u); }
inline uint64_t id_of(Handle h) { return h >> 1; }
inline bool is_rev(Handle h) { return (h & 1) != 0; }
inline Handle flip(Handle h) { return h ^ 1; }

// ---- graph ------------------------------------------------------------------------------------
struct Node {
    std::string seq;
    std::vector<Handle> left, right;  // insertion order, relative to the forward orientation
    bool present = false;
};

struct Path {
    std::string name;
    std::vector<Handle> steps;
};

class HashGraph {
  public:
    std::vector<Node> nodes;  // indexed by id
    uint64_t min_id = UINT64_MAX, max_id = 0, n_nodes = 0;
    std::vector<Path> paths;

    Handle create_handle(const std::string &seq, uint64_t id);
    void create_edge(Handle left, Handle right);
    std::string sequence(Handle h) const;
    size_t node_len(uint64_t id) const { return nodes[id].seq.size(); }
    // handle_edges_iter(h, Direction::Left | Right)
    std::vector<Handle> neighbors(Handle h, bool left) const;
    // GFAParser::parse_file + HashGraph::from_gfa
    static HashGraph from_gfa(const std::string &path);
};

// The P lines of a graph as vga_path_support_begin takes them: path p has the packed handles steps[step_off[p] .. step_off[p+1]).
struct PathTable {
    std::vector<std::string> names;
    std::vector<uint64_t> step_off;  // n_paths + 1
    std::vector<Handle> steps;
    std::vector<uint64_t> length;    // bases of the forward ("id+") steps of each path
    size_t n_paths() const { return names.size(); }
};
PathTable path_table(const HashGraph &g);

// ---- index ------------------------------------------------------------------------------------
struct NodeRef {
    uint64_t seq_idx, edge_idx, edges_to_node;
};

struct Index {
    uint64_t kmer_length = 0, seq_length = 0, n_edges = 0, n_nodes = 0, n_kmers = 0, n_kmer_pos = 0;
    std::string seq_fwd, seq_rev;
    std::vector<uint8_t> seq_bv;
    std::vector<Handle> edges;
    std::vector<NodeRef> node_ref;
    std::string kmer_keys;              // n_kmers * k, sorted
    std::vector<uint64_t> kmer_starts;  // the MPHF's values
    std::vector<vga_kmerpos> kmer_pos_table;

    static Index build(const HashGraph &g, uint64_t kmer_length, uint64_t max_furcations, uint64_t max_degree);
    // the same index with the k-mer half built on the GPU of `ctx` (vga_index_build_kmers), which keeps it loaded
    static Index build_on_device(const HashGraph &g, uint64_t kmer_length, uint64_t max_furcations, uint64_t max_degree, vga_ctx *ctx);
    // own container format ("VGAIDX1"); the reference's bincode .idx needs boomphf/bv/ahash internals
    void store(const std::string &path) const;
    static Index load(const std::string &path);
    // fills a vga_index_desc whose pointers stay valid while *this and `scratch` live
    struct DescScratch {
        std::vector<uint64_t> seq_idx, edge_idx, edges_to;
    };
    void describe(vga_index_desc &d, DescScratch &scratch) const;

    uint64_t get_bv_select(uint64_t element_no) const;
    uint64_t node_id_from_fwd_pos(uint64_t pos) const;
};

// ---- reads ------------------------------------------------------------------------------------
struct QuerySequence {
    std::string name, seq;
};
std::vector<QuerySequence> read_seqs_from_file(const std::string &filename);

// ---- GAF --------------------------------------------------------------------------------------
std::string gaf_placeholder(const QuerySequence &q);
std::string gaf_from_chain(const Index &ix, const QuerySequence &q, const vga_map_result *m, uint64_t read, uint64_t chain);
void gaf_from_chain_text(std::string &out, const Index &ix, const QuerySequence &q, const vga_map_result *m, uint64_t read, uint64_t chain,
                         const char *path, uint64_t path_len);
// A read mapped on its reverse complement (vga_map_result.strand[read] = 1) gets PAF's '-' convention: column 5 is '-', the
// reverse complement aligns to the path as written.  The chain writers read the strand from the map result; the query columns of
// a chain record are then flipped into the read's own frame.  An alignment record keeps 0 / length and the forward path.
std::string gaf_from_alignment(const QuerySequence &q, const vga_align_result *a, uint64_t read, bool reverse = false);
void gaf_from_alignment(std::string &out, const QuerySequence &q, const vga_align_result *a, uint64_t read, bool reverse = false);  // (appends)
// the reverse complement of a read (src/dna.rs:20-33 switch_base; a byte outside it becomes N)
std::string reverse_complement(const std::string &s);
// ValidationRecord::from_graph_and_alignment + to_string (src/validate.rs:36-102) from one alignments-GAF line
// A '-' record (--both-strands) carries the reverse complement of the read, the sequence its CIGAR describes.
std::string validation_record(const Index &ix, const std::string &gaf_line, const std::vector<QuerySequence> &reads);

// ---- map_reads --------------------------------------------------------------------------------
struct MapOptions {
    uint64_t bandwidth = 50;             // map_main.rs:103
    uint64_t max_gap = 1000;             // -g
    uint64_t chain_min_n_anchors = 3;    // -a
    double secondary_chain_threshold = 0.5;
    double max_mismatch_rate = 0.1;      // -r (parsed, unused by the reference's live code)
    double max_mapq = 60.0;
    bool write_console = false;          // -C
    bool also_align = false;             // -D
    uint64_t align_best_n = 1;           // -b
    std::string poa_aligner = "abpoa";   // -p
    int poa_remain_rule = -1;            // --poa-remain longest|first-edge: vga_poa_params.remain_rule (-1: the library's default)
    int device = 0;                      // used when `devices` is empty and map_reads is handed a context
    // Multi-GPU / streaming (not in the reference, which is single-threaded): one context and one host thread per entry of
    // `devices` (an id may repeat: two contexts on one GPU), each mapping a contiguous slice of the reads balanced by bases, in
    // chunks of at most `chunk_reads` reads (0 = the whole slice at once) so that host and device memory stay bounded.
    std::vector<int> devices;            // empty: `device` alone (--devices all: every visible GPU)
    bool all_devices = false;
    uint64_t chunk_reads = 32768;
    // the caller is about to leave the process with _exit: the contexts are not torn down (freeing tens of GB of HBM takes the
    // driver hundreds of milliseconds that a command line tool would only spend waiting), tear-down threads may still be running
    // when map_reads_multi returns.  ONLY for callers that leave the process right after a successful return (the contexts leak
    // otherwise); when anything fails, map_reads_multi joins those threads and destroys every context before it throws.
    bool leave_contexts = false;
    // false: map_reads_multi writes the GAF files chunk by chunk and returns no text (the CLI without -C / -v); true: the
    // whole GAF text comes back in MapOutput
    bool keep_text = true;
    bool also_validate = false;          // -v: write validation records (src/validate.rs:18-102, map.rs:186-208)
    std::string validation_path;         // -P
    // --both-strands (not in the reference): map each read and its reverse complement and keep the orientation that chains better
    // (vga_map_params.strands = VGA_STRANDS_BOTH)
    bool both_strands = false;
    // --coverage (not in the reference): count, on the GPU, how many reported alignments cover every base, node and edge of the
    // graph (vga_coverage_begin / vga_coverage_read) and write <out>-coverage-nodes.tsv, -bases.tsv and -edges.tsv next to the GAF
    // files.  Needs also_align.  Every context counts its own reads; the arrays are added in 64 bits at the end.
    bool coverage = false;
    // --coverage-only: coverage, and the alignments GAF text is neither built nor written (the chains GAF still is)
    bool coverage_only = false;
    // --path-support (not in the reference): score, on the GPU, every reported alignment against every P line of the graph
    // (vga_path_support_begin / _read / _last; `paths` is path_table() of the GFA the index was built from) and write
    // <out>-path-support.tsv and <out>-path-support-reads.tsv next to the GAF files.  Needs also_align.  Every context scores its own
    // reads; the per-path totals are added in 64 bits at the end.
    bool path_support = false;
    // --pileup (not in the reference): count, on the GPU, what the reported alignments say at every graph base -- read alleles
    // A C G T N, deletions, insertions (vga_pileup_begin / vga_pileup_read) -- and write <out>-pileup.tsv next to the GAF files
    // (needs also_align)
    bool pileup = false;
    // --genotype (not in the reference): add up, on the GPU, how well every pair of P lines explains the reported alignments
    // (vga_genotype_begin / vga_genotype_read over path support's matrices; `paths` as for path_support, which it turns on inside
    // the library without its two files) and write the ranked pairs to <out>-genotype.tsv: at most genotype_top of them, 0 = all.
    // Needs also_align.  Every context adds up its own reads; the pair tables are added in 64 bits at the end.
    bool genotype = false;
    uint64_t genotype_top = 20;
    // --genotype-likelihood (not in the reference): add up, on the GPU, the diploid read likelihood cost of every pair of P lines
    // (vga_genotype_lik_begin / vga_genotype_lik_read over path support's matrices, which it turns on like genotype) and write the
    // pairs from the cheapest up to <out>-genotype-likelihood.tsv: at most genotype_top of them, 0 = all.  genotype_lambda: the
    // cost of one unit of deficit in 1/256 bit (1..4096); genotype_cap: the largest deficit told apart (1..255).  Needs
    // also_align.  Every context adds up its own reads; the cost tables are added in 64 bits at the end.
    bool genotype_likelihood = false;
    uint32_t genotype_lambda = 512, genotype_cap = 64;
    // --path-edit (not in the reference): score, on the GPU, the read of every reported alignment against every P line by edit
    // distance (vga_path_edit_begin / _read / _last, which needs path support and turns it on without its files) and write
    // <out>-path-edit.tsv and <out>-path-edit-reads.tsv next to the GAF files.  Needs also_align.  Every context scores its own reads;
    // the per-path totals are added in 64 bits at the end.
    bool path_edit = false;
    // --genotype-from edit: the likelihood reads m - e of the edit distance (vga_genotype_lik_source), which it turns on without its
    // files; false: path support's matrices
    bool genotype_from_edit = false;
    // --call-variants (not in the reference): an integer-only diploid call at every graph base, made on the GPU from the pileup
    // counters (vga_variant_call; several contexts: their tables added in 64 bits, then vga_variant_call_table on the first), and
    // <out>-variants.tsv with the bases where the reads disagree with the graph.  Turns the pileup counting on without its file.
    // call_error: the cost of an observation that neither allele explains in 1/256 bit (257..8192); call_min_depth: the depth from
    // which a base is tested (at least 1); call_min_qual: the margin from which a call is reported.  Needs also_align.
    bool call_variants = false;
    uint32_t call_error = 1280;
    uint64_t call_min_depth = 4, call_min_qual = 512;
    // --call-insertions (not in the reference; needs call_variants): count, on the GPU, the lengths and the first eight letters of
    // what the reads insert behind every graph base (vga_insertion_begin), call length and letters at exactly the sites of
    // <out>-variants.tsv whose insertion state is het or hom, in that order (vga_insertion_call; several contexts: each hands its
    // whole table over, 196 bytes per base and context over PCIe, they are added in 64 bits, then vga_insertion_call_table on the
    // first with the summed rows of the sites), and write <out>-insertions.tsv
    bool call_insertions = false;
    // --call-deletions (not in the reference; needs call_variants): keep, on the GPU, every run of deleted graph bases of the
    // reported alignments as one event (vga_deletion_begin), sort, group and call the events against the pileup's depth with the
    // parameters of --call-variants (vga_deletion_call; several contexts: each hands its store over, 12 bytes per event, and the
    // first calls once on the summed pileup table with vga_deletion_call_table), and write <out>-deletions.tsv
    bool call_deletions = false;
    // --phase [--phase-min-links N] (not in the reference; needs call_variants): keep, on the GPU, the pileup list of every
    // reported alignment (vga_phase_begin), count the read-backed links between the heterozygous sites of <out>-variants.tsv up to
    // eight sites apart (vga_phase_links; several contexts: each hands its whole store over PCIe, the stores are concatenated,
    // then vga_phase_links_lists on the first), chain them on the host (vga_phase.hpp: ph_chain) and write <out>-phase.tsv
    bool phase = false;
    uint32_t phase_min_links = 2;
    // --haplotag (not in the reference; needs phase): per kept read and phase set the sites that vote for haplotype a and for
    // haplotype b of <out>-phase.tsv, counted on the GPU from the same store (vga_phase_tags; several contexts: vga_phase_tags_lists
    // on the first, from the concatenated stores), and write <out>-haplotag.tsv with the reads numbered as in the input file
    bool haplotag = false;
    // --haplotype-calls (not in the reference; needs haplotag): per phase set and per row of <out>-variants.tsv inside the set's
    // span, what the reads tagged a and the reads tagged b show there, counted on the GPU from the same store behind the tag call
    // (vga_haplotype_counts; several contexts: vga_haplotype_counts_lists on the first, from the concatenated stores), a haploid
    // call on each (vga_hapcall.hpp: hc_call), and write <out>-haplotype-calls.tsv
    bool haplotype_calls = false;
    // --phase-join (not in the reference; needs phase): join the phase sets of the chain by the reads that are tagged in two of
    // them, counted on the GPU from the same store behind the chain (vga_phase_set_links; several contexts:
    // vga_phase_set_links_lists on the first, from the concatenated stores), the join rule of vga_phase_join.hpp with links of at
    // least phase_join_min_reads reads (1 .. 65535), and write <out>-phase-joined.tsv, <out>-phase-sets.tsv and
    // <out>-phase-joins.tsv; haplotag and haplotype_calls then work on the joined sets.  <out>-phase.tsv stays the chain's.
    bool phase_join = false;
    uint32_t phase_join_min_reads = 2;
    // --haplotype-paths (not in the reference; needs phase and the P lines of --graph): keep a row of path deficits per kept read
    // beside the phase store (vga_haplotype_paths_begin: haplotype_paths_cap 1 .. 255, from the edit distance under
    // haplotype_paths_from_edit), sum the rows by (phase set, haplotype) on the GPU (vga_haplotype_paths; several contexts:
    // vga_haplotype_paths_lists on the first, from the concatenated stores), rank the paths of every group by the rule of
    // vga_hap_paths.hpp and write the best haplotype_paths_top (0: all) to <out>-haplotype-paths.tsv.  Turns path support on, not
    // its files; works on the joined sets under phase_join.
    bool haplotype_paths = false, haplotype_paths_from_edit = false;
    uint32_t haplotype_paths_cap = 64;
    uint64_t haplotype_paths_top = 5;
    // --path-abundance (not in the reference; needs also_align and the P lines of --graph): keep a row of path deficits per reported
    // alignment (vga_path_abundance_begin: abundance_cap 1 .. 255, from the edit distance under abundance_from_edit) and estimate,
    // on the GPU, the share of the reads that every P line explains by expectation-maximisation (vga_path_abundance: abundance_lambda
    // 1 .. 4096 in 1/256 bit per unit of deficit, at most abundance_iters iterations, 1 .. 100 000, until no share moves by more than
    // abundance_tol, 0 .. 2^24, in units of 2^-24; several contexts: each hands its store over, n_paths + 1 bytes per reported
    // alignment, and the first estimates once from the concatenated rows, vga_path_abundance_rows).  Writes the paths of at least
    // abundance_min parts per million (0: every path) to <out>-path-abundance.tsv.  Turns path support on, not its files; the edit
    // distance likewise under abundance_from_edit.
    bool path_abundance = false, abundance_from_edit = false;
    uint32_t abundance_lambda = 512, abundance_cap = 64, abundance_iters = 1000, abundance_tol = 16;
    uint64_t abundance_min = 10000;
    PathTable paths;
};
// the run scores alignments against the P lines of the graph (path_support, genotype, genotype_likelihood, path_edit, haplotype_paths,
// path_abundance): it needs `paths`
bool scoring_on(const MapOptions &opt);

// VGA_TRACE=1: wall-clock marks of the driver's phases on stderr (since the first call)
void trace_mark(const char *what);

struct MapOutput {
    std::string chains_gaf, alignments_gaf, validation;
    uint64_t n_reads = 0, n_aligned = 0, n_anchors = 0, poa_cells = 0;
    uint64_t n_reverse = 0;              // reads mapped on their reverse complement (both_strands)
    double ms_map = 0, ms_align = 0;     // summed over chunks (per device: the maximum over devices)
    uint64_t n_chunks = 0, n_devices = 0;
    uint64_t n_pileup = 0, n_leading_ins = 0;  // alignments counted into the pileup and their insertions before any base (MapOptions::pileup)
    uint64_t n_variant_tested = 0, n_variant_calls = 0;  // bases tested and bases reported (MapOptions::call_variants)
    uint64_t n_phase_sites = 0, n_phase_sets = 0, n_phase_reads = 0;  // heterozygous sites, phase sets and reads kept (MapOptions::phase)
    uint64_t n_haplotag_rows = 0, n_haplotag_a = 0, n_haplotag_b = 0, n_haplotag_tied = 0;  // rows and their haplotypes (MapOptions::haplotag)
    // the sets, the groups with reads, the scored and the kept reads, and the call of the largest set (MapOptions::haplotype_paths)
    uint64_t n_hap_path_sets = 0, n_hap_path_groups = 0, n_hap_path_scored = 0, n_hap_path_kept = 0;
    std::string hap_path_call;
    uint64_t n_join_sets = 0, n_joins = 0, n_join_agree = 0, n_join_conflict = 0;  // chain sets, accepted links, links inside a component (MapOptions::phase_join)
    uint64_t n_hapcall_jobs = 0, n_hapcall_rows = 0, n_hapcall_differ = 0;  // jobs, lines written, lines whose two decided calls differ (MapOptions::haplotype_calls)
    // runs of deleted bases, the alignments they come from, those at an end of an alignment, distinct events, calls (MapOptions::call_deletions)
    uint64_t n_deletion_runs = 0, n_deletion_alignments = 0, n_deletion_end_runs = 0, n_deletion_distinct = 0, n_deletion_calls = 0;
    uint64_t n_insertion_sites = 0, n_insertion_long = 0;  // sites called and those longer than 8 letters (MapOptions::call_insertions)
    uint64_t n_coverage = 0;             // alignments counted into the coverage tables (MapOptions::coverage)
    uint64_t n_edit_alignments = 0, n_edit_too_long = 0;  // alignments seen by the edit distance, and those whose read it does not serve (MapOptions::path_edit)
    uint64_t n_path_scored = 0, n_path_unplaced = 0;  // alignments scored against the paths, and those no path supports (MapOptions::path_support)
    // MapOptions::genotype: the pairs ranked, and the first of them (names of its P lines, its sums); no pair ranked: no call
    uint64_t n_genotype_pairs = 0, genotype_sum_bases = 0, genotype_sum_edges = 0;
    std::string genotype_a, genotype_b;
    // MapOptions::genotype_likelihood: the rows scored (0: no call), the cheapest pair (names of its P lines, its cost in 1/256
    // bit) and how much more the next pair costs
    uint64_t n_likelihood_scored = 0, likelihood_cost = 0, likelihood_next = 0;
    std::string likelihood_a, likelihood_b;
    // MapOptions::path_abundance: the scored rows (0: no call) of the rows kept, the iterations and whether they converged, and the
    // parts per million of the paths written, from the largest down
    uint64_t n_abundance_scored = 0, n_abundance_kept = 0, abundance_iterations = 0;
    bool abundance_converged = false;
    std::vector<uint64_t> abundance_ppm;
};

// One [begin, end) range of the read list, the device slot (index into MapOptions::devices) that maps it.
struct Shard {
    uint64_t begin, end;
    uint32_t slot;
};
// Contiguous slices balanced by bases, one per device slot (the rule of sharding.py::split_by_bases), each cut into chunks of
// at most chunk_reads reads.  Shards come in read order; concatenating their outputs reproduces the single-batch output.
std::vector<Shard> plan_shards(const std::vector<uint64_t> &read_lengths, uint32_t n_slots, uint64_t chunk_reads);

// diagnostics: the text half of the product path replayed (vgh_map.cpp: textpath_replay)
struct TextReplay { uint64_t bytes = 0, chains_bytes = 0; double seconds = 0, text_seconds = 0, write_seconds = 0; unsigned threads = 0; };
TextReplay textpath_replay(vga_ctx *ctx, const Index &ix, const std::vector<QuerySequence> &inputs, const MapOptions &opt, const std::string &out_prefix,
                           unsigned repeat, unsigned n_threads);
// ctx must already hold the uploaded index: maps everything on that one context, in chunks of opt.chunk_reads.
// out_prefix == "" writes no files.
MapOutput map_reads(vga_ctx *ctx, const Index &ix, const std::vector<QuerySequence> &inputs, const MapOptions &opt,
                    const std::string &out_prefix);
// Creates one context per entry of opt.devices (all visible GPUs when empty), uploads the index to each and maps the slices
// concurrently; GAF order = read order (src/map.rs:123-133, 174-184).
MapOutput map_reads_multi(const Index &ix, const std::vector<QuerySequence> &inputs, const MapOptions &opt,
                          const std::string &out_prefix);
// throws unless `g` has the nodes of `ix`: the same count and the same lengths (what --path-support asks of --graph)
void check_graph_matches_index(const HashGraph &g, const Index &ix);
// Begins to create the contexts map_reads_multi(.., opt, ..) will use, on a thread of its own: starting HIP takes 0.1-0.3 s,
// which a caller can spend reading its index and reads.  The next map_reads_multi call picks them up (and reports any error).
void prewarm_contexts(const MapOptions &opt);

}  // namespace vgh
