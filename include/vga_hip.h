/*
 * vga_hip.h -- C ABI of libvga_hip.so: the MI355X (gfx950) implementation of rs-vgaligner's
 * per-read hot path  map.rs -> chain.rs -> align.rs.
 *
 * Plain C, plain pointers and sizes, int error codes.  No C++/torch types cross this boundary.
 * Every entry point names the reference interface it stands in for (paths relative to the
 * AlgoLab/rs-vgaligner checkout).  A Rust `extern "C"` block binding exactly these symbols is shown
 * in INTEGRATION.md.
 *
 * Ownership: inputs are borrowed for the duration of a call; result objects are allocated by the
 * library and released with the matching *_free.  Device memory belongs to the ctx.  One ctx per
 * GPU; calls on one ctx must be serialised by the caller, different ctxs may be driven from
 * different threads/processes concurrently.  Nothing throws or aborts across the ABI: a negative
 * return code plus vga_last_error(ctx) replaces the reference's panic!/unwrap().
 */
#ifndef VGA_HIP_H
#define VGA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VGA_OK 0
#define VGA_ERR_ARG (-1)
#define VGA_ERR_HIP (-2)          /* a HIP runtime call failed (message has the hipError string) */
#define VGA_ERR_NOMEM (-3)
#define VGA_ERR_UNSUPPORTED (-4)  /* k > 32, non-ACGT k-mer in the table, bandwidth > 64, ... */
#define VGA_ERR_NO_INDEX (-5)
#define VGA_ERR_NO_DEVICE (-6)    /* no gfx950 device visible: the library never falls back to a CPU path */
#define VGA_ERR_POOL (-7)         /* traceback pool exhausted; retry with a smaller sub-batch */

#define VGA_NO_PRED (-1)

/* the longest k-mer vga_index_upload accepts: k <= 15 is probed through a direct-address table, 16 <= k <= 32 through a
 * table hashed on the 2-bit packed k-mer (64 bits) */
#define VGA_MAX_KMER_LENGTH 32

typedef struct vga_ctx vga_ctx;

/* ---- context ---------------------------------------------------------------------------- */
/* Creates a context on HIP device `device` with a private stream.  Fails with VGA_ERR_NO_DEVICE
 * when no GPU is present. */
int vga_ctx_create(int device, vga_ctx **out);
void vga_ctx_destroy(vga_ctx *ctx);
/* Message of the last error of `ctx`.  The pointer is a copy that belongs to the calling thread (valid until that thread calls
 * vga_last_error again); two entry points of one context may run on two threads (vga_chain_paths_text beside vga_align_batch)
 * and each may read it. */
const char *vga_last_error(const vga_ctx *ctx);
/* Per-context settings (replace the VGA_POOL_FRACTION / VGA_HOST_THREADS environment hand-off of ABI <= 5; src/map.rs has no
 * counterpart: the reference is single-threaded and holds no device memory).
 *   vga_ctx_set_pool_fraction: the share (0, 1] of the device memory that is free when vga_align_batch sizes its traceback pool
 *     that THIS context may take -- 1 / n for n contexts on one GPU (`vgaligner map --devices 0,0`).  Default 1.
 *   vga_ctx_set_host_threads: host threads the calls of this context fan out to (subgraph fallback, CIGAR / cs strings, result
 *     copies); 0 = the default (VGA_HOST_THREADS if set, else the hardware's concurrency, at most 32).
 * Both take effect with the next call on the context; VGA_ERR_ARG outside those ranges. */
int vga_ctx_set_pool_fraction(vga_ctx *ctx, double fraction);
int vga_ctx_set_host_threads(vga_ctx *ctx, uint32_t n_threads);
/* Blocks until all work queued on the ctx's stream has finished. */
int vga_ctx_synchronize(vga_ctx *ctx);
/* ABI version of the library (bumped on any signature change). */
int vga_abi_version(void);

/* ---- index upload ------------------------------------------------------------------------ */
/* KmerPos, src/kmer.rs:733-738 (SeqPos = {orient, position}, src/kmer.rs:27-31).
 * The delimiter record is {1, UINT64_MAX, 1, UINT64_MAX} (src/kmer.rs:740-749). */
typedef struct {
    uint64_t start;
    uint64_t end;
    uint8_t start_orient; /* 0 Forward, 1 Reverse */
    uint8_t end_orient;
} vga_kmerpos;

/* Host view of the fields of `Index` the query side reads (src/index.rs:37-90).  The boomphf MPHF
 * and the ahash keys are replaced by the k-mer strings themselves: the reference checks exact
 * membership before it consults the MPHF (src/index.rs:319-320), so an exact map is equivalent. */
typedef struct {
    uint32_t kmer_length;          /* Index.kmer_length */
    uint64_t seq_length;           /* Index.seq_length */
    const char *seq_fwd;           /* Index.seq_fwd, seq_length bytes */
    uint64_t n_nodes;              /* Index.n_nodes */
    const uint64_t *node_seq_idx;  /* NodeRef.seq_idx,       n_nodes+1 (src/utils.rs:15-22) */
    const uint64_t *node_edge_idx; /* NodeRef.edge_idx,      n_nodes+1 */
    const uint64_t *node_edges_to; /* NodeRef.edges_to_node, n_nodes+1 */
    uint64_t n_edges;              /* Index.n_edges */
    const uint64_t *edges;         /* Index.edges as packed handles (id<<1 | is_reverse) */
    uint64_t n_kmers;              /* Index.n_kmers */
    const char *kmer_keys;         /* n_kmers * kmer_length bytes, the distinct k-mers */
    const uint64_t *kmer_starts;   /* per k-mer: first record in kmer_pos_table (the MPHF's values) */
    uint64_t n_kmer_pos;           /* Index.n_kmer_pos (records incl. delimiters) */
    const vga_kmerpos *kmer_pos_table; /* Index.kmer_pos_table */
} vga_index_desc;

/* Stands in for Index::load_from_file + every per-read Index accessor
 * (src/index.rs:296-305, 309-382, 388-606): copies the index to HBM once.
 * VGA_ERR_UNSUPPORTED: kmer_length outside 1..VGA_MAX_KMER_LENGTH, a k-mer with a base outside upper-case ACGT, a graph
 * beyond 32-bit device coordinates.  On failure the context holds no index. */
int vga_index_upload(vga_ctx *ctx, const vga_index_desc *desc);

/* Stands in for generate_kmers_parallel + sort/dedup + generate_pos_on_ref_2 of Index::build
 * (src/index.rs:162-220, src/kmer.rs:277-505, 816-928).  Reads the graph half of *desc (kmer_length, seq_length,
 * seq_fwd, n_nodes, node_seq_idx / node_edge_idx / node_edges_to, n_edges, edges) and fills its k-mer half
 * (n_kmers, kmer_keys, kmer_starts, n_kmer_pos, kmer_pos_table) with arrays the library allocates; release them with
 * vga_index_kmers_free.  On VGA_OK the context also holds the index, exactly as after vga_index_upload(ctx, desc), with
 * the probe tables built on the device.  The arrays equal the host builder's byte for byte.
 * VGA_ERR_UNSUPPORTED: k = 0 or k > 15 (the k-mer walk on the GPU keeps 32-bit keys: the host builder handles k-mers of up to
 * VGA_MAX_KMER_LENGTH bases, and vga_index_upload takes its index), a byte of seq_fwd outside upper-case ACGTN, an empty node, a graph beyond 32-bit
 * device coordinates.  VGA_ERR_NOMEM (with a message, never a fault) when the k-mer paths blow up.  A graph with no
 * k-mer of this length fails with the host's message.  On failure the context holds no index.  With ctx == NULL:
 * VGA_ERR_NO_DEVICE when no GPU is visible (there is no CPU path).
 * (ABI 6 gained these two calls; no existing signature changed.) */
int vga_index_build_kmers(vga_ctx *ctx, vga_index_desc *desc, uint64_t max_furcations, uint64_t max_degree);
/* frees the five k-mer fields vga_index_build_kmers filled and zeroes them */
void vga_index_kmers_free(vga_index_desc *desc);

/* ---- read batches -------------------------------------------------------------------------- */
typedef struct vga_batch vga_batch;
/* reads_concat: all read sequences back to back; read_off[i]..read_off[i+1] delimits read i
 * (n_reads+1 offsets).  Copies the reads to HBM (the Vec<QuerySequence> of src/io.rs:74-162). */
int vga_batch_create(vga_ctx *ctx, const char *reads_concat, const uint64_t *read_off, uint64_t n_reads,
                     vga_batch **out);
/* May be called before or after vga_ctx_destroy of the batch's context: destroying the context releases the
 * batch's device memory and detaches it (later map / align calls on it return VGA_ERR_ARG). */
void vga_batch_destroy(vga_batch *b);
/* The two halves of a batch as the map and align kernels read them: forward[total] and reverse[total] (either may be NULL),
 * read r at read_off[r] in both.  from_host = 0: the device's copy (built with k_revcomp_reads if the batch has none yet);
 * from_host = 1: the host's (vga_batch_revcomp_host).  The kernel seam of the reverse complement, as vga_poa_batch is for POA:
 * the library itself never reads a reverse half back.  VGA_ERR_ARG for a NULL batch or one whose context is gone.
 * (Added within ABI 6: one function, no struct.) */
int vga_batch_strands(vga_batch *b, int from_host, char *forward, char *reverse);

/* ---- map: anchors + chains ------------------------------------------------------------------ */
typedef struct {
    uint32_t bandwidth;           /* 50   (src/subcommands/map_main.rs:103) */
    uint64_t max_gap;             /* 1000 (map_main.rs:30-34) */
    uint32_t chain_min_n_anchors; /* 3    (map_main.rs:42-46) */
    int only_forward;             /* 1    (src/map.rs:62).  0 = anchors_for_query(.., false) (src/chain.rs:154-155): every
                                   * k-mer record becomes an anchor and bit 31 of target_begin / target_end is the
                                   * orientation of that end (1 = reverse strand); k <= 13 or k >= 16; such chains cannot be passed
                                   * to vga_align_batch unless they are all-forward */
    int emit_dp;                  /* 1: the result also carries Anchor.id, f(i) and the best predecessor of every anchor
                                   *    (what the reference keeps inside chain_anchors; parity checks read them).
                                   * 0: anchor_id / max_chain_score / best_pred_id are NULL -- the GAF writers and
                                   *    vga_align_batch only read the anchor coordinates and the chain membership, and
                                   *    16 of the 40 bytes per anchor stay on the GPU. */
    int32_t strands;              /* VGA_STRANDS_*: which orientations of each read are mapped (not in the reference, whose
                                   * map.rs looks at the read as given).  It occupies what was tail padding: size and offsets
                                   * are unchanged.  VGA_ERR_ARG for any other value; BOTH needs only_forward = 1
                                   * (VGA_ERR_UNSUPPORTED otherwise). */
} vga_map_params;
/* FORWARD: the read as given (the default).  BOTH: the read and its reverse complement (each byte through the reference's
 * switch_base, src/dna.rs:20-33, any byte outside it becoming N) are mapped alike; per read the orientation whose chaining
 * optimum curr_max is larger wins (vga_map_result.strand), a tie going to the read as given, and a side with only the
 * placeholder chain never winning.  Every per-read field of the result then describes the chosen orientation only, in its
 * own frame: query coordinates of a reverse read count from the start of its reverse complement. */
#define VGA_STRANDS_FORWARD 0
#define VGA_STRANDS_BOTH 1
void vga_map_default_params(vga_map_params *p);

/* Result of anchors_for_query + chain_anchors for every read of a batch.
 * Anchors of read r occupy [anchor_off[r], anchor_off[r+1]) and are in the order chain_anchors
 * leaves them in (stable sort by target_end.position, src/chain.rs:386-389).
 * Chains of read r are chain_off[r]..chain_off[r+1]; a read with no chain has exactly one
 * placeholder entry (src/chain.rs:644-649) with chain_len == 0. */
typedef struct {
    uint64_t n_reads;
    uint64_t n_anchors;
    uint64_t *anchor_off;    /* n_reads+1 */
    uint32_t *anchor_id;     /* Anchor.id (src/chain.rs:146,162); NULL when emit_dp = 0 */
    uint32_t *query_begin;   /* Anchor.query_begin; query_end = query_begin + k */
    uint32_t *target_begin;  /* Anchor.target_begin.position (Forward) */
    uint32_t *target_end;    /* Anchor.target_end.position   (Forward) */
    double *max_chain_score; /* f(i) after src/chain.rs:403-450; NULL when emit_dp = 0 */
    int32_t *best_pred_id;   /* id of the best predecessor after the DP, VGA_NO_PRED for None; NULL when emit_dp = 0 */
    double *curr_max;        /* per read */
    uint64_t n_chains;
    uint64_t *chain_off;        /* n_reads+1 */
    uint8_t *chain_placeholder; /* n_chains */
    uint64_t *chain_anchor_off; /* n_chains+1, into chain_anchor_idx */
    uint32_t *chain_anchor_idx; /* index (within the read's sorted anchors) of each chain member, ascending */
    /* timing of the last call, milliseconds, measured with hipEvents on the ctx stream */
    float ms_probe, ms_sort, ms_chain, ms_total;
    uint64_t n_hits;            /* position records touched (H of the byte model); with VGA_STRANDS_BOTH, of both orientations */
    uint8_t *strand;            /* n_reads: 0 the read as given, 1 its reverse complement (VGA_STRANDS_BOTH); NULL otherwise.
                                 * vga_align_batch aligns the chosen orientation against the forward graph. */
} vga_map_result;

/* Stands in for the pass-1 loop of map_reads: anchors_for_query (src/map.rs:62 -> src/chain.rs:134)
 * followed by chain_anchors (src/map.rs:79-89 -> src/chain.rs:370). */
int vga_map_batch(vga_batch *b, const vga_map_params *params, vga_map_result **out);
void vga_map_result_free(vga_map_result *r);

/* The path column of every chain's GAF record -- GAFAlignment::from_chain (src/align.rs:762-911) with AnchorPosOnGraph::new
 * (src/chain.rs:90-127): for each anchor of a chain, in order, "(>N:off,>N:off)," = node id and offset inside the node of
 * target_begin and of the inclusive target_end.  `text` holds the fields of all chains back to back, without terminators;
 * chain c's field is text[text_off[c] .. text_off[c + 1]) (empty for a placeholder chain).  Forward-strand anchors only
 * (vga_map_params.only_forward = 1, the reference's only live setting).
 * Threads: the one call on a context that may run beside another -- one thread may be in vga_chain_paths_text while
 * another is in vga_align_batch on the same context (it works on a stream of its own and shares only the index and, on
 * failure, the error string). */
typedef struct {
    uint64_t n_chains;
    uint64_t *text_off; /* n_chains + 1 */
    char *text;
    float ms_total;
} vga_chain_text;
int vga_chain_paths_text(vga_ctx *ctx, const vga_map_result *chains, vga_chain_text **out);
void vga_chain_text_free(vga_chain_text *t);

/* ---- align: chain -> subgraph -> POA ---------------------------------------------------------- */
typedef struct {
    int32_t match;     /* 2  */
    int32_t mismatch;  /* 4  */
    int32_t gap_open1; /* 4  */
    int32_t gap_ext1;  /* 2  */
    int32_t gap_open2; /* 24 */
    int32_t gap_ext2;  /* 1  */
    int32_t wb;        /* 10, adaptive band: w = wb + floor(wf * qlen); wb < 0 disables banding */
    int32_t remain_rule; /* VGA_REMAIN_*: which path the diagonal term  qlen - remain[row]  of the adaptive band follows
                          * (ABI 4; it occupies what was padding before `wf`, so sizes and offsets are unchanged) */
    double wf;         /* 0.01 */
} vga_poa_params;
/* remain[row] = graph bases after the row on one path to the sink.  abPOA's source is not in the reference tree, so which
 * path it takes is unverified; both readings are implemented and parity-tested (oracle/og_poa.c):
 *   LONGEST_PATH   the longest path to the sink (the default of rounds 1-3 of this library);
 *   FIRST_OUT_EDGE the path that follows the heaviest out-edge, the first on a tie -- abPOA's abpoa_BFS_set_node_remain
 *                  as remembered; with the unit weights of a graph built from node strings + an edge list that is the
 *                  first out-edge in edge-list order.  vga_poa_default_params sets this one since round 4: it is the
 *                  reading most likely to reproduce the reference's scores and CIGARs. */
#define VGA_REMAIN_LONGEST_PATH 0
#define VGA_REMAIN_FIRST_OUT_EDGE 1
void vga_poa_default_params(vga_poa_params *p);

/* The fields of ab_poa's AbpoaAlignmentResult that the reference consumes
 * (src/align.rs:205-206, 1107, 1152-1165), for n problems. */
typedef struct {
    uint64_t n;
    uint8_t *ok;                /* 0: placeholder / no alignment inside the band */
    int32_t *best_score;
    uint64_t *path_off;         /* n+1: per problem, range of graph-consuming alignment columns */
    uint32_t *abpoa_nodes;      /* AbpoaAlignmentResult.abpoa_nodes: 1-based base-row id per column */
    uint32_t *graph_nodes;      /* AbpoaAlignmentResult.graph_nodes: index of the node string per column */
    uint32_t *aln_start_offset;
    uint32_t *aln_end_offset;
    uint32_t *n_aligned_bases;
    uint64_t *cigar_off;        /* n+1 */
    char *cigar;                /* concatenated, each NUL terminated inside its range */
    uint64_t *cs_off;           /* n+1 */
    char *cs;                   /* "cs:Z:..." */
    uint64_t *n_rows;           /* N of the byte model: graph bases in the subgraph */
    uint64_t *n_cells;          /* C of the byte model: sum of band widths */
    uint64_t *n_value_cells;    /* cells of the rows whose values are kept in HBM (last base of each node) */
    float ms_dp, ms_traceback, ms_total;
} vga_poa_result;
void vga_poa_result_free(vga_poa_result *r);

/* The reference's one real FFI seam:
 *   AbpoaAligner::create_align_safe(&Vec<&str> nodes, &Vec<(usize,usize)> edges, &str query, Global)
 * (src/align.rs:173-203), batched over n independent problems.
 * Problem p owns nodes node_ptr[p] .. node_ptr[p+1]-1; node v is nodes_concat[node_off[v] .. node_off[v+1])
 * (node_off holds node_ptr[n]+1 absolute offsets: node strings are laid out back to back);
 * edges edge_ptr[p]..edge_ptr[p+1] are 0-based (src,dst) pairs with src < dst; the query is
 * queries_concat[query_off[p] .. query_off[p+1]). */
int vga_poa_batch(vga_ctx *ctx, uint64_t n, const uint64_t *node_ptr, const uint64_t *node_off,
                  const char *nodes_concat, const uint64_t *edge_ptr, const uint32_t *edge_src,
                  const uint32_t *edge_dst, const uint64_t *query_off, const char *queries_concat,
                  const vga_poa_params *params, vga_poa_result **out);

/* One alignment record per read: best_alignment_for_query (src/align.rs:34-55) over the chains of
 * vga_map_batch, i.e. find_range_chain + extend_range_chain_2 + find_nodes_edges_for_abpoa +
 * create_align_safe + the fields generate_alignment needs (src/align.rs:267-402, 523-665, 670-724,
 * 202, 1096-1168). */
typedef struct {
    uint64_t n_reads;
    uint8_t *aligned;            /* 0 => placeholder record (src/align.rs:913-930) */
    uint64_t *path_off;          /* n_reads+1 */
    uint64_t *path_handles;      /* packed handles of the node path after dedup (src/align.rs:1114-1123) */
    uint32_t *path_length;       /* abpoa_nodes.len()  (src/align.rs:1152) */
    uint32_t *path_start;        /* aln_start_offset   (src/align.rs:1155) */
    uint32_t *path_end;          /* aln_end_offset     (src/align.rs:1156) */
    uint32_t *block_length;      /* n_aligned_bases    (src/align.rs:1158) */
    int32_t *best_score;
    uint64_t *cigar_off;
    char *cigar;
    uint64_t *cs_off;
    char *cs;
    uint64_t poa_rows, poa_cells, poa_value_cells, poa_problems; /* totals for the byte model */
    float ms_subgraph, ms_dp, ms_traceback, ms_total;
    uint64_t result_bytes;       /* what crossed PCIe for cs / CIGAR / node paths: their text (K4c) or the raw traceback operations (ABI 6) */
} vga_align_result;

int vga_align_batch(vga_batch *b, const vga_map_result *chains, uint32_t align_best_n,
                    const vga_poa_params *params, vga_align_result **out);
void vga_align_result_free(vga_align_result *r);
/* Optional, returns at once.  The first vga_align_batch of a context allocates its traceback memory before its first kernel
 * (tens of GB of HBM; on memory another process has used the driver clears what it hands out, 0.2 s and more).  A caller that
 * knows it is going to align n_reads reads of up to max_read_len bases says so early -- before vga_map_batch, say -- and the
 * allocation runs on a thread of its own meanwhile.  No counterpart in the reference (its abPOA allocates per call on the
 * host, src/align.rs:1032-1040). */
int vga_align_prepare(vga_ctx *ctx, uint64_t n_reads, uint32_t max_read_len);

/* ---- coverage: how many reported alignments cover every base, node and edge of the graph ----------
 * Stands in for nothing in the reference, whose map.rs ends at the GAF writer: it is what a reader of the alignments GAF
 * (vg pack, gafpack and their like) computes from the text, counted here while the alignments are still on the GPU.
 * Coverage is defined on the record vga_align_batch reports for a read (the winner of best_alignment_for_query); a read
 * with a placeholder record adds nothing.  Along the record's path, from path_start inside its first node:
 *   an M operation (cs ":N" per base, "*gq")  adds one to base_depth of its graph base;
 *   a D operation (cs "-g..") skips its graph bases, an I operation (cs "+q..") touches none.
 *   base_depth[p], p in [0, seq_length): position node_seq_idx[id - 1] + offset of seq_fwd;
 *   node_reads[id - 1]: reported alignments whose path holds node id (a node crossed only by a deletion counts);
 *   edge_reads[e], e in [0, n_edges), laid out as vga_index_desc.edges: for each consecutive pair (a, b) of a path one is
 *     added at the slot of b in the OUTGOING part of a's slice (node_edge_idx[a-1] + node_edges_to[a-1] ...); incoming slots stay 0;
 *   n_alignments: aligned records counted.
 * The counters are 32-bit, exact and independent of the order of the additions; they belong to the context's index: uploading
 * or building another index drops them and turns counting off.
 *   vga_coverage_begin  needs an index (VGA_ERR_NO_INDEX); allocates and zeroes; every later vga_align_batch on ctx adds its
 *                       reported alignments.  VGA_SUBGRAPH=host is refused by vga_align_batch while counting is on.
 *   vga_coverage_read   any pointer may be NULL; does not reset.  VGA_ERR_ARG without _begin; VGA_ERR_UNSUPPORTED once
 *                       n_alignments has reached 2^32 - 1 (a counter may have wrapped).
 *   vga_coverage_reset  zero, keep counting (VGA_ERR_ARG without _begin).
 *   vga_coverage_end    free, stop counting.
 * With counting off vga_align_batch does what it did before these calls existed: no extra launch, no extra allocation.
 * vga_poa_batch has no graph coordinates and never counts. */
int vga_coverage_begin(vga_ctx *ctx);
int vga_coverage_read(vga_ctx *ctx, uint32_t *base_depth /* seq_length */, uint32_t *node_reads /* n_nodes */,
                      uint32_t *edge_reads /* n_edges */, uint64_t *n_alignments);
int vga_coverage_reset(vga_ctx *ctx);
int vga_coverage_end(vga_ctx *ctx);

/* ---- path support: how well every reported alignment fits every haplotype path (P line) of the graph ----------
 * Stands in for nothing in the reference, whose map.rs ends at the GAF writer: it is the input of allele typing, a reads x
 * paths table computed while the alignments are still on the GPU.  It is defined on the text of the alignments GAF plus the
 * GFA's S and P lines and on nothing else (tests/path_support_ref.py recomputes it from them).  For the record vga_align_batch
 * reports for read r (path >w0>w1.., path_start, cs) and path p (steps "id+" / "id-"):
 *   bases[r][p]  graph bases under r's M operations (cs ":N" and "*gq": coverage's notion of covered) that lie in a node p
 *                visits as "id+".  A node p visits twice counts once; an "id-" step sets nothing.
 *   edges[r][p]  consecutive pairs (w_i, w_i+1) of r's path for which p has the step w_i+ immediately followed by w_i+1+
 *                (bases alone cannot tell an allele from its deletion variant, whose nodes are a subset).
 *   top paths of r: the paths whose key (bases, edges) is the lexicographic maximum, unless that maximum is (0, 0).
 * A read with a placeholder record has a zero row and adds nothing.  With VGA_STRANDS_BOTH a '-' record carries the forward
 * path, so the same rule applies.  Per path, accumulated over calls like coverage (64-bit, exact, order-independent):
 *   sum_bases[p], sum_edges[p]; top[p]: alignments with p among their top paths; top_alone[p]: alignments whose only top path
 *   is p; and the scalars n_alignments and n_unplaced (alignments whose keys are all (0, 0)).
 * The state belongs to the context's index: uploading or building another index drops it and turns path support off.
 *   vga_path_support_begin  needs an index (VGA_ERR_NO_INDEX).  steps[step_off[p] .. step_off[p+1]) are the packed handles
 *                           (id << 1 | is_reverse) of path p.  VGA_ERR_ARG: n_paths == 0, a step_off that decreases, a handle
 *                           whose id is outside 1..n_nodes.  VGA_ERR_UNSUPPORTED: more than 4096 paths.  A step pair "a+,b+"
 *                           without an edge a -> b in the index (no L line) can never match a record and sets nothing;
 *                           *n_pairs_without_edge (may be NULL) says how many there were.  Every later vga_align_batch on ctx
 *                           scores its reported alignments; VGA_SUBGRAPH=host is refused by it while path support is on.  A
 *                           second begin starts over with the new paths.
 *   vga_path_support_read   the accumulators, n_paths values each; any pointer may be NULL; does not reset.
 *   vga_path_support_last   the n_reads x n_paths matrices (row-major) of the most recent vga_align_batch on ctx; either may
 *                           be NULL.  VGA_ERR_ARG if n_reads is not that batch's or there has been none since begin.
 *   vga_path_support_reset  zero the accumulators, stay on.        vga_path_support_end  free, turn off.
 *   vga_path_support_lists  the kernel seam, as vga_poa_batch is for POA: scores n explicit lists -- node ids in path order
 *                           (list i: node_ids[node_off[i] .. node_off[i+1])) and, per node, how many of its bases are covered
 *                           (at most its length, VGA_ERR_ARG otherwise) -- through the same kernel into bases_out / edges_out
 *                           (n x n_paths), and does not touch the accumulators.  A pair that is no edge of the index scores 0.
 * read, last, reset and lists return VGA_ERR_ARG while path support is off.  With it off vga_align_batch does what it did
 * before these calls existed: no extra launch, no extra allocation. */
int vga_path_support_begin(vga_ctx *ctx, uint32_t n_paths, const uint64_t *step_off /* n_paths + 1 */, const uint64_t *steps,
                           uint64_t *n_pairs_without_edge);
int vga_path_support_read(vga_ctx *ctx, uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *top, uint64_t *top_alone,
                          uint64_t *n_alignments, uint64_t *n_unplaced);
int vga_path_support_last(vga_ctx *ctx, uint64_t n_reads, uint32_t *bases, uint32_t *edges);
int vga_path_support_reset(vga_ctx *ctx);
int vga_path_support_end(vga_ctx *ctx);
int vga_path_support_lists(vga_ctx *ctx, uint64_t n, const uint64_t *node_off /* n + 1 */, const uint32_t *node_ids,
                           const uint32_t *node_bases, uint32_t *bases_out, uint32_t *edges_out);

/* ---- pileup: what the reported alignments say at every base of the graph ----------
 * Stands in for nothing in the reference, whose map.rs ends at the GAF writer: it is the table a SNP / indel caller, a consensus
 * polisher or novel-allele discovery builds from the cs strings of the alignments GAF, counted here while the alignments are still
 * on the GPU.  It is defined on that text alone (tests/pileup_ref.py recomputes it).  Along the record reported for a read, from
 * path_start inside its first node, with seven counters per graph base in the order A C G T N del ins:
 *   cs ":N"    adds one, at each of its N graph bases, to the column of that base's own letter;
 *   cs "*gq"   adds one, at its graph base, to the column of q (N for any read letter other than a c g t);
 *   cs "-g.."  adds one to del at each of its graph bases;
 *   cs "+q.."  adds one to ins at the graph base consumed most recently before it, covered or deleted; an insertion before the
 *              first consumed base belongs to no base and adds one to leading_ins.
 * So A + C + G + T + N at a base is coverage's base_depth there.  A read with a placeholder record adds nothing.  With
 * VGA_STRANDS_BOTH a '-' record carries the forward path and the cs of the reverse complement: alleles are on the graph's forward
 * strand.  The counters are 32-bit, exact and independent of the order of the additions; they belong to the context's index:
 * uploading or building another index drops them and turns counting off.
 *   vga_pileup_begin  needs an index (VGA_ERR_NO_INDEX); VGA_ERR_UNSUPPORTED for a graph of 2^29 bases or more; allocates and
 *                     zeroes; every later vga_align_batch on ctx adds its reported alignments.  VGA_SUBGRAPH=host is refused
 *                     by vga_align_batch while counting is on.
 *   vga_pileup_read   counts: seq_length x 7, row-major, a row per base of seq_fwd; any pointer may be NULL; does not reset.
 *                     VGA_ERR_ARG without _begin; VGA_ERR_UNSUPPORTED once n_alignments has reached 2^32 - 1.
 *   vga_pileup_reset  zero, keep counting (VGA_ERR_ARG without _begin).
 *   vga_pileup_end    free, stop counting.
 * With counting off vga_align_batch does what it did before these calls existed: no extra launch, no extra allocation.
 * vga_poa_batch has no graph coordinates and never counts. */
int vga_pileup_begin(vga_ctx *ctx);
int vga_pileup_read(vga_ctx *ctx, uint32_t *counts /* seq_length * 7 */, uint64_t *n_alignments, uint64_t *leading_ins);
int vga_pileup_reset(vga_ctx *ctx);
int vga_pileup_end(vga_ctx *ctx);

/* ---- genotype: which pair of haplotype paths explains the reported alignments best ----------
 * Stands in for nothing in the reference.  It is the diploid reading of path support: a read from a region two alleles share
 * votes for both, so the second allele of a heterozygous sample is not the second line of the per-path totals; the pair of
 * paths that together explains the reads best is.  Defined on the two n_reads x n_paths matrices of one vga_align_batch (what
 * vga_path_support_last returns) and on nothing else (tests/genotype_ref.py recomputes it).  With key[r][p] = (bases[r][p],
 * edges[r][p]) compared lexicographically, for every pair p <= q and every row r:
 *   take_q = key[r][q] > key[r][p]                (a full tie takes p)
 *   sum_bases[p,q] += bases[r][take_q ? q : p]    sum_edges[p,q] += edges[r][take_q ? q : p]
 *                                                 (the maximum is taken on the tuple, the components are summed apart: it is
 *                                                 not a sum of packed keys)
 *   prefer_a[p,q] += 1 if key[r][p] > key[r][q]   prefer_b[p,q] += 1 if key[r][q] > key[r][p]     (both stay 0 for p == q)
 * Every row takes part: a placeholder or unplaced row is all zeros, adds 0 to the sums and ties everywhere.  The four
 * accumulators are 64-bit, exact and independent of the order of the additions, and accumulate over calls until reset.
 * The pair (p, q) sits at  p * n_paths - p * (p - 1) / 2 + (q - p)  of each array: the upper triangle, row-major,
 * n_pairs = n_paths * (n_paths + 1) / 2 entries.  Ranking the pairs (by sum_bases, then sum_edges, both descending, then the
 * homozygous pair first, then p, then q; pairs whose sums are (0, 0) are not ranked) is the caller's: sum[p,q] >= sum[p,p]
 * always, so a homozygous sample ties its own heterozygous pairs and prefer_a / prefer_b tell them apart.
 * The state belongs to path support's, which belongs to the context's index: vga_path_support_end, a second
 * vga_path_support_begin, uploading or building another index drop it and turn genotyping off.
 *   vga_genotype_begin  needs path support on (VGA_ERR_ARG otherwise).  Allocates and zeroes the n_pairs x 4 64-bit table --
 *                       32 n_pairs bytes of device memory: 2.5 KB at 12 paths, 268 MB at 4096 -- VGA_ERR_NOMEM when that fails.
 *                       Every later vga_align_batch on ctx adds the pairs of its matrices, right after it has scored them.
 *   vga_genotype_read   n_pairs values each; any pointer may be NULL; VGA_ERR_ARG if n_pairs is not the table's; does not reset.
 *   vga_genotype_reset  zero the table, stay on.               vga_genotype_end  free, turn off (no error when it is off).
 *   vga_genotype_pairs  the kernel seam, as vga_path_support_lists is for the scoring: explicit n_reads x n_paths host matrices
 *                       (row-major, n_paths 1..4096, VGA_ERR_ARG otherwise or for a NULL matrix with n_reads > 0) through the
 *                       same kernel into a table of its own.  Needs a context only: no index, no path support, and it touches
 *                       no accumulator.  n_reads = 0 gives zeros.
 * read and reset return VGA_ERR_ARG while genotyping is off.  With it off vga_align_batch tests one pointer and does what it
 * did before these calls existed: no extra launch, no extra allocation, no entry in vga_last_kernel_times. */
int vga_genotype_begin(vga_ctx *ctx);
int vga_genotype_read(vga_ctx *ctx, uint64_t n_pairs, uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *prefer_a,
                      uint64_t *prefer_b);
int vga_genotype_reset(vga_ctx *ctx);
int vga_genotype_end(vga_ctx *ctx);
int vga_genotype_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges,
                       uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *prefer_a, uint64_t *prefer_b);

/* ---- genotype likelihood: the diploid read likelihood of every pair of haplotype paths ----------
 * Stands in for nothing in the reference.  The standard model of HLA typers: each read is explained by one of the two alleles
 * with probability 1/2 each.  Defined, in integers only, on the two n_reads x n_paths matrices of one vga_align_batch (what
 * vga_path_support_last returns) and on nothing else (tests/genotype_lik_ref.py recomputes it).  With lambda in 1..4096, the cost
 * of one unit of deficit in 1/256 bit, and cap in 1..255, for every row r:
 *   s[r][p] = bases[r][p] + edges[r][p]                      (64 bits)
 *   d[r][p] = min(max over p' of s[r][p'] - s[r][p], cap)    (the capped deficit, a byte; an all-zero row has d = 0 everywhere)
 *   cost[p,q] += lambda min(d[r][p], d[r][q]) + T[|d[r][p] - d[r][q]|]     for every pair p <= q, in uint64
 *   n_scored  += 1 if some s[r][p] > 0
 * with T[x] = round(256 (1 - log2(1 + 2^(-lambda x / 256)))), x = 0..cap: T[0] = 0, T never decreases, T <= 256.  This is
 * -log2(1/2 2^(-lambda d_p) + 1/2 2^(-lambda d_q)) in 1/256 bit.  The cost is additive over reads, calls and contexts (the row
 * maximum lies within the row) and independent of their order.  cost sits at p P - p (p - 1) / 2 + (q - p), as the genotype
 * table does.  Ranking is the caller's: cost ascending, then the homozygous pair first, then p, then q; n_scored = 0 is no call.
 * It does not need vga_genotype_begin and does not change it: either, both or neither may be on.  The state belongs to path
 * support's, like the genotype table: vga_path_support_end, a second vga_path_support_begin, uploading or building another index
 * drop it.
 *   vga_genotype_lik_table  no context: out[0..cap] = T.  VGA_ERR_ARG for lambda or cap out of range or a NULL out.  The one
 *                           definition of T: the kernels receive this table and never evaluate a logarithm.
 *   vga_genotype_lik_begin  needs path support on (VGA_ERR_ARG otherwise, and for lambda or cap out of range).  Allocates and
 *                           zeroes the table, 8 n_pairs bytes of device memory (and 8 for n_scored) -- VGA_ERR_NOMEM when that
 *                           fails.  Every later vga_align_batch on ctx adds the cost of its matrices, right after scoring them.
 *   vga_genotype_lik_read   n_pairs values; either pointer may be NULL; VGA_ERR_ARG if n_pairs is not the table's; does not reset.
 *   vga_genotype_lik_reset  zero the table, stay on.           vga_genotype_lik_end  free, turn off (no error when it is off).
 *   vga_genotype_lik_pairs  the kernel seam: explicit n_reads x n_paths host matrices (row-major, n_paths 1..4096; VGA_ERR_ARG
 *                           otherwise, for lambda or cap out of range, or for a NULL matrix with n_reads > 0) through the same
 *                           two kernels into a table of its own.  deficit_out (n_reads x n_paths bytes), cost_out and n_scored
 *                           may each be NULL.  Needs a context only.  n_reads = 0 gives zeros.
 * read and reset return VGA_ERR_ARG while it is off.  With it off vga_align_batch tests one pointer and does what it did before
 * these calls existed: no extra launch, no extra allocation, no entry in vga_last_kernel_times. */
int vga_genotype_lik_table(uint32_t lambda, uint32_t cap, uint32_t *out /* cap + 1 */);
int vga_genotype_lik_begin(vga_ctx *ctx, uint32_t lambda, uint32_t cap);
int vga_genotype_lik_read(vga_ctx *ctx, uint64_t n_pairs, uint64_t *cost, uint64_t *n_scored);
int vga_genotype_lik_reset(vga_ctx *ctx);
int vga_genotype_lik_end(vga_ctx *ctx);
int vga_genotype_lik_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges,
                           uint32_t lambda, uint32_t cap, uint8_t *deficit_out, uint64_t *cost_out, uint64_t *n_scored);

/* ---- path edit: the edit distance of every reported alignment's read to every haplotype path ----------
 * Stands in for nothing in the reference.  Path support counts what the alignment happened to walk over; this is what allele
 * typers use: the unit-cost edit distance of the read to the allele's sequence.  Defined on the alignments GAF, the GFA's S and P
 * lines and the read sequences and on nothing else (tests/path_edit_ref.py recomputes it from them).  For the record reported for
 * read r, with query Q of m letters (the read; its reverse complement for a '-' record under VGA_STRANDS_BOTH) and node path
 * w0..wn, and path p with sequence seq_p (its steps' node sequences in order, an "id-" step reverse-complemented, N stays N;
 * pos_p(i) the offset of step i):
 *   letters  compared upper-cased; A, C, G and T equal themselves, any other letter on either side matches nothing;
 *   anchor   a = the first node of w that p visits as "id+", i = the FIRST such step of p;
 *            b = the last node of w that p visits as "id+",  j = the LAST such step of p;
 *            no such node, or j < i: e[r][p] = NONE (0xFFFFFFFF);
 *   window   lo = max(0, pos_p(i) - m), hi = min(|seq_p|, pos_p(j) + len(b) + m): every placement of Q that overlaps the anchor span;
 *   e[r][p]  the minimum of edit(Q, seq_p[s:t]) over lo <= s <= t <= hi (Sellers' infix distance: the top row is 0, the answer the
 *            minimum of the bottom row, column 0 included), so e <= m.
 * A read with a placeholder record has a NONE row; so has a read of more than 16 384 letters, which the kernel does not serve:
 * it is counted in n_too_long.  Per path, accumulated over calls like path support (64-bit, exact, order-independent):
 *   n_scored[p]: alignments with e[r][p] != NONE; sum_edit[p]: the sum of those e; best[p]: alignments for which p attains the
 *   minimum of the row over its scored paths; best_alone[p]: those where no other path does; and the scalars n_alignments
 *   (aligned records seen) and n_too_long.
 * The state belongs to path support's, like the genotype tables: vga_path_support_end, a second vga_path_support_begin, uploading
 * or building another index drop it.
 *   vga_path_edit_begin  needs path support on (VGA_ERR_ARG otherwise).  Builds the path sequences (one byte per base) and each
 *                        path's sorted (node, step) array on the device.  VGA_ERR_UNSUPPORTED when the paths hold 2^32 bases or
 *                        more, VGA_ERR_NOMEM when an allocation fails.  Every later vga_align_batch on ctx scores its reported
 *                        alignments.  A second begin starts over.
 *   vga_path_edit_read   the accumulators, n_paths values each; any pointer may be NULL; does not reset.
 *   vga_path_edit_last   the n_reads x n_paths matrix (row-major) of the most recent vga_align_batch on ctx.  VGA_ERR_ARG if
 *                        n_reads is not that batch's or there has been none since begin.
 *   vga_path_edit_reset  zero the accumulators, stay on.        vga_path_edit_end  free, turn off (no error when it is off).
 *   vga_path_edit_pairs  the kernel seam: n explicit pairs -- query i is q[q_off[i] .. q_off[i+1]), text i is
 *                        t[t_off[i] .. t_off[i+1]) -- through the same distance kernel with lo = 0, hi = |text|, into out[i].
 *                        A query of more than 16 384 letters gives NONE, an empty query 0, an empty text m.  Needs a context
 *                        only: no index, no path support, and it touches no accumulator.
 *   vga_genotype_lik_source  which matrices the likelihood reads from now on: VGA_GL_FROM_SUPPORT (the default: path support's
 *                        bases and edges) or VGA_GL_FROM_EDIT, which needs vga_path_edit_begin as well (VGA_ERR_ARG otherwise, for
 *                        any other value, and while the likelihood is off): after every batch the same two kernels get
 *                        bases' = m_r - e[r][p] (0 for NONE) and edges' = 0, so d = min(e - min e, cap), a NONE pair gets the
 *                        deficit of e = m, and an all-NONE row costs nothing.  A deficit is then a count of edits.
 * read, last and reset return VGA_ERR_ARG while it is off.  With it off vga_align_batch tests one pointer and does what it did
 * before these calls existed: no extra launch, no extra allocation, no entry in vga_last_kernel_times. */
#define VGA_GL_FROM_SUPPORT 0u
#define VGA_GL_FROM_EDIT 1u
int vga_path_edit_begin(vga_ctx *ctx);
int vga_path_edit_read(vga_ctx *ctx, uint64_t *n_scored, uint64_t *sum_edit, uint64_t *best, uint64_t *best_alone,
                       uint64_t *n_alignments, uint64_t *n_too_long);
int vga_path_edit_last(vga_ctx *ctx, uint64_t n_reads, uint32_t *edit);
int vga_path_edit_reset(vga_ctx *ctx);
int vga_path_edit_end(vga_ctx *ctx);
int vga_path_edit_pairs(vga_ctx *ctx, uint64_t n, const uint64_t *q_off /* n + 1 */, const char *q, const uint64_t *t_off /* n + 1 */,
                        const char *t, uint32_t *out /* n */);
int vga_genotype_lik_source(vga_ctx *ctx, uint32_t source);

/* ---- variant call: where the reads disagree with the graph, called from the pileup on the GPU ----------
 * Stands in for nothing in the reference.  It is the first consumer of the pileup table that stays on the device: an
 * integer-only diploid call at every graph base, the sites compacted there, so that only the calls cross PCIe.  Defined on the
 * pileup table and the graph's letters and on nothing else (tests/variant_ref.py recomputes it, from the alignments GAF too).
 * Costs are in 1/256 bit, like the genotype likelihood's.
 *   inputs     for base i its pileup row A C G T N del ins, exactly as vga_pileup_read returns it, and its letter;
 *              r = the column of the letter (A C G T in either case 0..3, anything else N);  depth = A + C + G + T + N + del.
 *              The alleles are A < C < G < T < D, D a deleted base with n_D = del.  The N column counts towards depth only.
 *   parameters E, the cost of an observation that neither allele of the genotype explains (257..8192; 1280 in the CLI),
 *              min_depth (at least 1; 4) and min_qual (512).  The defaults are choices, not measurements.
 *   tested     a base with r < 4 and depth >= min_depth.  A base whose own letter is not A C G T is never tested.
 *   genotype   for every unordered pair x <= y of the five alleles (15 pairs) cost(x, y) = sum over a of n_a w(a; x, y) in 64 bits:
 *              w = 0 for a == x under a homozygous pair, 256 for a == x or a == y under a heterozygous one, E for any other
 *              observation.  The pairs are enumerated as (r, r), then the four pairs that hold r by their other allele ascending,
 *              then the remaining ten by (x, y) ascending; the first minimum in that order is the genotype, so the reference
 *              genotype wins every tie.  qual = the smallest cost among the other fourteen pairs minus the best, saturated at
 *              2^32 - 1.
 *   insertion  behind the base, with k = min(ins, depth): none costs ins E, het 256 depth, hom (depth - k) E; the first minimum
 *              in that order wins, ins_qual = the second smallest cost minus the best (64 bits, not saturated).
 *   reported   a tested base whose genotype is not (r, r) with qual >= min_qual, or whose insertion state is not none with
 *              ins_qual >= min_qual.
 * The calls come in base order as parallel arrays: pos (the base), gt (x | y << 3 | state << 6, alleles 0..4 = A C G T D, state
 * 0 none, 1 het, 2 hom), qual, ins_qual, depth and -- what a caller needs to print a site without fetching the table -- counts,
 * the base's seven counters widened to 64 bits (cap x 7, row-major; may be NULL).  The first min(n_calls, cap) are written,
 * *n_calls is the total and *n_tested the tested bases (either may be NULL); the arrays may be NULL when cap is 0.  A counter of
 * 2^32 - 1 is an ordinary value.  The inserted letters are not called here (the insertion call below), the sites are independent, and a base on one arm of a
 * bubble sees only the reads that went through that arm.
 *   vga_variant_call        from the context's own counters, after the prefix pass vga_pileup_read does too.  Needs
 *                           vga_pileup_begin (VGA_ERR_ARG otherwise, and for E or min_depth out of range or a NULL array with
 *                           cap > 0); VGA_ERR_UNSUPPORTED where vga_pileup_read refuses.  Does not reset the counters.
 *   vga_variant_call_table  the kernel seam, and the route of several contexts whose tables were added in 64 bits: an explicit
 *                           table of n rows (counts_in: n x 7, letters: n) through the same kernels.  Needs a context only: no
 *                           index, no counters touched.  VGA_ERR_UNSUPPORTED for a counter of 2^40 or more (found on the
 *                           device) and for n of 2^31 or more.  n = 0 gives no call.
 * Neither is called by vga_align_batch: with no call made nothing is launched or allocated. */
int vga_variant_call(vga_ctx *ctx, uint32_t E, uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *pos, uint8_t *gt,
                     uint32_t *qual, uint64_t *ins_qual, uint64_t *depth, uint64_t *counts /* cap * 7 */, uint64_t *n_tested,
                     uint64_t *n_calls);
int vga_variant_call_table(vga_ctx *ctx, uint64_t n, const uint64_t *counts_in /* n * 7 */, const char *letters /* n */, uint32_t E,
                           uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *pos, uint8_t *gt, uint32_t *qual,
                           uint64_t *ins_qual, uint64_t *depth, uint64_t *counts /* cap * 7 */, uint64_t *n_tested, uint64_t *n_calls);

/* ---- insertion call: what the reads insert behind a graph base ----------
 * Stands in for nothing in the reference.  The pileup says that reads insert behind a base and the variant call reports the base
 * as ins = het or hom; this table keeps the letters.  It is defined on the alignments GAF text alone (tests/insertion_ref.py
 * recomputes it).  Along the record reported for a read, walked exactly as the pileup walks it, a cs token "+q.." of L letters
 * belongs to the graph base consumed most recently before it, covered or deleted; one before the first consumed base belongs to
 * no base, adds one to n_leading and touches no counter.  Per graph base 49 counters, row-major:
 *   len[1] .. len[8], len_more   (columns 0 .. 8)   the insertions at this base of exactly l letters, and of more than 8;
 *   let[j][A C G T N], j = 0..7  (column 9 + 5 j + c) the insertions at this base of more than j letters whose j-th letter is
 *                                that one: lower case equals upper case, anything but a c g t is N; an insertion of more than 8
 *                                letters adds its first 8.
 * So len[1] + .. + len[8] + len_more at a base is the pileup's ins there, the five let[j][.] add up to the insertions longer than
 * j, and n_leading is the pileup's leading_ins.  With VGA_STRANDS_BOTH the letters are on the graph's forward strand.  The
 * counters are 32-bit, exact and independent of the order of the additions; they belong to the context's index: uploading or
 * building another index drops them and turns counting off.  The 8 is a choice, not a measurement.
 *   the call   for one row, integer-only and without parameters: length = the bin with the most reads among 1 .. 8, more (the
 *              shorter on a tie, more being the longest; reported as 9 for more; 0 for a row whose bins are all zero),
 *              length_reads that bin's count; for j < min(length, 8) seq[j] = the letter with the largest let[j][.] (A < C < G < T
 *              < N on a tie) and seq_reads[j] its count; seq[j] = 0 and seq_reads[j] = 0 behind them.  The letter counts at j mix
 *              the insertions of every length above j, two insertions of one length at a site are not told apart
 *              (seq_reads below length_reads is the sign), and an insertion of more than 8 letters is cut to its first 8.
 *   vga_insertion_begin       needs an index (VGA_ERR_NO_INDEX); VGA_ERR_UNSUPPORTED for a graph of 2^26 bases or more (a
 *                             position shares a word with the bin, and the table is indexed in 32 bits); allocates and zeroes
 *                             seq_length x 49 counters; every later vga_align_batch on ctx adds its reported alignments.
 *                             VGA_SUBGRAPH=host is refused by vga_align_batch while counting is on.
 *   vga_insertion_read        counts: seq_length x 49; n_events: the insertions counted; any pointer may be NULL; does not reset.
 *                             VGA_ERR_ARG without _begin; VGA_ERR_UNSUPPORTED once n_alignments has reached 2^32 - 1.
 *   vga_insertion_reset       zero, keep counting (VGA_ERR_ARG without _begin).
 *   vga_insertion_end         free, stop counting.
 *   vga_insertion_call        the call at the n bases pos[0 .. n) from the context's own counters: the rows are gathered on the
 *                             device, the table stays there.  length: n; length_reads: n; seq: n x 8 (letters A C G T N, or 0);
 *                             seq_reads: n x 8; rows: n x 49, the counters widened to 64 bits (may be NULL).  VGA_ERR_ARG without
 *                             _begin, for a pos >= seq_length and for a NULL array with n > 0.  Does not reset.  n = 0 is
 *                             accepted.
 *   vga_insertion_call_table  the kernel seam, and the route of several contexts whose tables were added in 64 bits: explicit
 *                             rows (rows_in: n x 49) through the same kernel.  Needs a context only: no index, no counters
 *                             touched.  VGA_ERR_UNSUPPORTED for a counter of 2^40 or more (found on the device).
 * With counting off vga_align_batch does what it did before these calls existed: no extra launch, no extra allocation. */
int vga_insertion_begin(vga_ctx *ctx);
int vga_insertion_read(vga_ctx *ctx, uint32_t *counts /* seq_length * 49 */, uint64_t *n_alignments, uint64_t *n_events,
                       uint64_t *n_leading);
int vga_insertion_reset(vga_ctx *ctx);
int vga_insertion_end(vga_ctx *ctx);
int vga_insertion_call(vga_ctx *ctx, uint64_t n, const uint32_t *pos /* n */, uint8_t *length /* n */, uint64_t *length_reads /* n */,
                       uint8_t *seq /* n * 8 */, uint64_t *seq_reads /* n * 8 */, uint64_t *rows /* n * 49 */);
int vga_insertion_call_table(vga_ctx *ctx, uint64_t n, const uint64_t *rows_in /* n * 49 */, uint8_t *length /* n */,
                             uint64_t *length_reads /* n */, uint8_t *seq /* n * 8 */, uint64_t *seq_reads /* n * 8 */,
                             uint64_t *rows /* n * 49 */);

/* ---- deletion call: deletions of several graph bases as one event each ----------
 * Stands in for nothing in the reference.  The pileup counts a deleted base where it lies and the variant call calls every base
 * alone: a deletion of ten bases is ten D calls.  Here a deletion is one event.  It is defined on the alignments GAF text, the
 * node starts and the pileup table alone (tests/deletion_ref.py recomputes it).
 *   run        one "-g.." token of the cs string of the record reported for a read (a maximal sequence of D operations): len its
 *              letters, first and last the positions on the linearised graph of its first and last deleted base.
 *   end run    a run with no ":" or "*" token before it in the record, or none behind it.  The alignment is global over its
 *              subgraph, so such a run is where the subgraph ends, not a deletion of the sample: it is counted in n_end_runs and
 *              otherwise ignored (it still counts in the pileup and in the variant call).
 *   event      every other run, as the three 32-bit words (first, len, last).  last - first != len - 1 means the run crosses
 *              nodes; the same (first, len) may have two values of last through a bubble, so last is part of the identity.
 *   store      while it is on, every vga_align_batch appends the events of its reported alignments to a grow-only store on the
 *              device, in the order of the reported alignments and then along the alignment.  It doubles; VGA_ERR_NOMEM, with the
 *              alignments kept, when it cannot grow or would pass 2^32 - 1 words.
 *   call       the events sorted by (first, len, last) ascending and grouped: reads is the size of a group, depth the sum
 *              A + C + G + T + N + del of the pileup row at first (the depth of the variant call, end runs of other reads
 *              included).  With k = min(reads, depth) and the error cost E: none costs k E, het 256 depth, hom (depth - k) E; the
 *              first minimum in that order is the state (0 none, 1 het, 2 hom) and qual the second smallest cost minus the
 *              smallest, saturated at 2^32 - 1: the insertion-state rule of the variant call.  vga_deletion_state is that rule.
 *   reported   a group with depth >= min_depth, a state other than none and qual >= min_qual; the calls come in sort order.
 *   not done   no haplotype is attributed, a run split by one spurious match is two events, nearly identical events (a start
 *              shifted by one) are not merged, and the depth is taken at the first base only.
 *   vga_deletion_begin       after vga_pileup_begin (VGA_ERR_ARG without it; VGA_ERR_NO_INDEX without an index); empties the store.
 *   vga_deletion_read        events: 3 x n_events words (ask with NULL first); n_alignments counted since _begin / _reset; any
 *                            pointer may be NULL; does not reset.
 *   vga_deletion_reset       empty, keep storing (VGA_ERR_ARG without _begin).
 *   vga_deletion_end         free, stop storing.  vga_pileup_end and a new index drop the store as well.
 *   vga_deletion_call        from the context's own store and pileup counters.  E, min_depth and min_qual as in vga_variant_call.
 *                            Per reported group first, len, last, state, qual, depth, reads: the first min(n_calls, cap) of them;
 *                            n_distinct (the groups) and n_calls always.  When cap < n_calls nothing is written beyond cap and the
 *                            caller asks again.  VGA_ERR_ARG for a NULL array with cap > 0.  Does not reset.
 *   vga_deletion_call_table  the kernel seam, and the route of several contexts: explicit events (3 x n_events words) and an
 *                            explicit pileup table (n_bases x 7 counters of 64 bits).  Needs a context only.  Every event is
 *                            checked before anything is launched: first and last below n_bases and len >= 1, else VGA_ERR_ARG.
 *                            VGA_ERR_UNSUPPORTED for 2^32 - 1 events or more, for 2^31 bases or more and for a counter of 2^40 or
 *                            more (found on the device).
 * With the store off vga_align_batch does what it did before these calls existed: no extra launch, no extra allocation. */
int vga_deletion_begin(vga_ctx *ctx);
int vga_deletion_read(vga_ctx *ctx, uint32_t *events /* 3 * n_events */, uint64_t *n_alignments, uint64_t *n_events, uint64_t *n_end_runs);
int vga_deletion_reset(vga_ctx *ctx);
int vga_deletion_end(vga_ctx *ctx);
int vga_deletion_call(vga_ctx *ctx, uint32_t error, uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *first /* cap */,
                      uint32_t *len /* cap */, uint32_t *last /* cap */, uint8_t *state /* cap */, uint32_t *qual /* cap */,
                      uint64_t *depth /* cap */, uint64_t *reads /* cap */, uint64_t *n_distinct, uint64_t *n_calls);
int vga_deletion_call_table(vga_ctx *ctx, uint64_t n_events, const uint32_t *events /* 3 * n_events */, uint64_t n_bases,
                            const uint64_t *counts /* n_bases * 7 */, uint32_t error, uint64_t min_depth, uint64_t min_qual, uint64_t cap,
                            uint32_t *first /* cap */, uint32_t *len /* cap */, uint32_t *last /* cap */, uint8_t *state /* cap */,
                            uint32_t *qual /* cap */, uint64_t *depth /* cap */, uint64_t *reads /* cap */, uint64_t *n_distinct,
                            uint64_t *n_calls);
/* the rule alone, no context: the state for `reads` alignments that hold an event at a base of `depth`; *qual (may be NULL) */
uint32_t vga_deletion_state(uint64_t reads, uint64_t depth, uint32_t error, uint32_t *qual);

/* ---- phase: which alleles of the heterozygous calls travel together on the reads ----------
 * Stands in for nothing in the reference.  The variant call reports independent diploid sites; this is the read-backed linkage
 * between the heterozygous ones.  It is defined on the alignments GAF text, the node starts, the graph's letters and the sites
 * alone (tests/phase_ref.py recomputes it).
 *   sites        H graph bases pos[0] < pos[1] < .. with two alleles x[h] < y[h] in A < C < G < T < D (0 .. 4).
 *   observation  of the record reported for a read at site h, the record walked exactly as the pileup walks it: a ":N" that
 *                covers the base observes the base's own letter, "*gq" observes q (a q that is not a c g t observes "other"),
 *                "-g.." observes D, a "+q.." observes nothing.  A record can consume a base more than once (a self-loop):
 *                sx = some observation equals x, sy likewise; obs = 0 for sx and not sy, 1 for sy and not sx, 2 when the base
 *                is consumed otherwise, 3 when it is not consumed.
 *   site_reads   [h][0 .. 2]: the records with obs 0, 1 and 2 at site h.
 *   links        [h][d - 1][2 a + b], 1 <= d <= 8 (the window: a choice, not a measurement), h + d < H, a, b in {0, 1}: the
 *                records with obs a at site h and obs b at site h + d; rows with h + d >= H are zero.
 *   the store    one record per reported alignment, three words {off, n_runs, n_sparse}, and its words from word `off` on:
 *                  n_runs run-event words, in pairs:  position << 1  where a run of matched bases starts (the word covers that
 *                    position),  (position behind the run's last base) << 1 | 1  where it ends (the word does not cover it);
 *                  n_sparse sparse words  position << 3 | column:  0 .. 3 the read shows A C G T at the base, 4 another letter,
 *                    5 the base is deleted, 6 an insertion behind the base (no observation).
 *                These are the pileup's lists (k_pu_events), kept as they are.
 *   vga_phase_begin        needs vga_pileup_begin on ctx (VGA_ERR_ARG otherwise; VGA_ERR_NO_INDEX without an index).  From then on
 *                          every vga_align_batch copies the pileup lists of its reported alignments into a grow-only device store
 *                          of the context (k_ph_keep), device-made and host-made lists alike.  The store starts at
 *                          VGA_PHASE_STORE_WORDS words (2^20) and doubles; when it cannot grow or would pass 2^32 - 1 words
 *                          vga_align_batch fails with VGA_ERR_NOMEM and says how many reads were kept.  Calling it again empties
 *                          the store.  The store belongs to the context's index and to its pileup: a new index or
 *                          vga_pileup_end drops it.
 *   vga_phase_read         recs: n_reads x 3, words: n_words; *n_reads and *n_words are always written, so a first call with NULL
 *                          arrays sizes the second.  VGA_ERR_ARG without _begin.  Does not reset.
 *   vga_phase_reset        empties the store, keeps it on (VGA_ERR_ARG without _begin).
 *   vga_phase_end          frees the store and stops keeping.
 *   vga_phase_links        links (n_sites x 8 x 4) and site_reads (n_sites x 3) from the context's own store and the letters of
 *                          its index, *n_reads the stored records (k_ph_obs and k_ph_link over tiles of reads; the tile's read
 *                          count is a multiple of 64 sized from 64 MiB and n_sites, VGA_PHASE_READ_TILE overrides it).
 *                          VGA_ERR_ARG without _begin, for sites that do not ascend strictly inside the graph, for alleles that
 *                          are not x < y <= 4, and for a NULL array with n_sites > 0; VGA_ERR_UNSUPPORTED above 2^24 sites.
 *                          n_sites = 0 is accepted.  Does not reset.
 *   vga_phase_links_lists  the kernel seam, and the route of several contexts whose stores were concatenated: explicit records
 *                          and words on a graph of n_bases bases, and ref[h] the own letter of site h: 0 .. 3 for A C G T, 4 for
 *                          any other letter (a run of matches observes "other" there).  Needs a context only: no index, no
 *                          store touched.  Everything a kernel follows is checked first: a record inside the n_words words, run
 *                          words in start / end pairs with end above start and at most n_bases, sparse positions below n_bases
 *                          and columns below 7, the sites as above, ref <= 4; a violation is VGA_ERR_ARG and launches nothing.
 *   vga_phase_chain        no context, on the host, integer-only; the one definition (csrc/vga_phase.hpp).  For h in order the
 *                          smallest d in 1 .. min(8, h) whose l = links[h - d][d - 1] has cis = l[0] + l[3] and trans = l[1] +
 *                          l[2] that differ, by at least min_links (1 .. 65535; the command line's default is 2: a choice, not a
 *                          measurement), gives ps[h] = ps[h - d], flip[h] = flip[h - d] xor (trans > cis), link_d[h] = d;
 *                          otherwise h opens a set: ps[h] = h + 1 (its own line among the sites), flip 0, link_d 0.  Haplotype a
 *                          carries flip ? y : x, haplotype b the other allele.  VGA_ERR_ARG for min_links out of range or a NULL
 *                          array with n_sites > 0.
 *   haplotype tags         which stored reads go with which haplotype of which phase set; integers only.  With ps and flip as
 *                          vga_phase_chain returns them, site h votes in read r when obs(r, h) <= 1, and its vote is obs xor
 *                          flip[h]: 0 for haplotype a (which carries flip ? y : x), 1 for haplotype b.  votes_a and votes_b of
 *                          (r, p) count the votes of the sites with ps[h] = p.  A row {read, ps, votes_a, votes_b} (four uint32)
 *                          exists for every (r, p) with a vote; rows are ordered by read (the index of the record in the store),
 *                          then by ps ascending.  The read goes with a when votes_a > votes_b, with b when votes_b > votes_a, and
 *                          with neither on a tie.  There is no "best set per read" rule: every set a read votes in has its row.
 *   vga_phase_tags         the rows from the context's own store at the sites pos, x, y (as vga_phase_links takes them) under
 *                          ps and flip; *n_reads the stored records (may be NULL).  At most cap rows are written and *n_rows, the
 *                          number there are, is always written: a caller that finds *n_rows > cap asks again with that cap (as
 *                          with vga_variant_call).  Per tile of reads k_ph_obs, then k_ph_tag (count), k_ph_tag_scan (exclusive
 *                          scan; the running total goes from tile to tile in a device word) and k_ph_tag (emit): the rows do not
 *                          depend on the tile size.  VGA_ERR_ARG for everything vga_phase_links refuses, for ps[h] outside 1 ..
 *                          h + 1, for ps[ps[h] - 1] != ps[h] (the named site must open its set), for flip[h] > 1, for a NULL
 *                          array with n_sites > 0, a NULL n_rows, and NULL rows with cap > 0.  n_sites = 0 or an empty store:
 *                          0 rows.  Does not reset.
 *   vga_phase_tags_lists   the kernel seam, and the route of several contexts: the same from explicit records and words, with
 *                          every check of vga_phase_links_lists and the ones above; a violation launches nothing and leaves rows
 *                          and *n_rows as they were.
 * With the store off vga_align_batch does what it did before these calls existed: no k_ph_* launch, no extra allocation. */
int vga_phase_begin(vga_ctx *ctx);
int vga_phase_read(vga_ctx *ctx, uint32_t *recs /* n_reads * 3 */, uint32_t *words /* n_words */, uint64_t *n_reads, uint64_t *n_words);
int vga_phase_reset(vga_ctx *ctx);
int vga_phase_end(vga_ctx *ctx);
int vga_phase_links(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos /* n_sites */, const uint8_t *x, const uint8_t *y,
                    uint32_t *links /* n_sites * 32 */, uint32_t *site_reads /* n_sites * 3 */, uint64_t *n_reads);
int vga_phase_links_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs /* n_reads * 3 */, uint64_t n_words,
                          const uint32_t *words, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y,
                          const uint8_t *ref, uint32_t *links /* n_sites * 32 */, uint32_t *site_reads /* n_sites * 3 */);
int vga_phase_chain(uint64_t n_sites, const uint32_t *links /* n_sites * 32 */, uint32_t min_links, uint32_t *ps, uint8_t *flip,
                    uint8_t *link_d);
int vga_phase_tags(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos /* n_sites */, const uint8_t *x, const uint8_t *y, const uint32_t *ps,
                   const uint8_t *flip, uint64_t cap, uint32_t *rows /* cap * 4 */, uint64_t *n_rows, uint64_t *n_reads);
int vga_phase_tags_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs /* n_reads * 3 */, uint64_t n_words,
                         const uint32_t *words, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint8_t *ref,
                         const uint32_t *ps, const uint8_t *flip, uint64_t cap, uint32_t *rows /* cap * 4 */, uint64_t *n_rows);

/* ---- haplotype counts: what the reads of each haplotype of a phase set show at every reported call ----------
 * Stands in for nothing in the reference.  The consumer of the haplotype tags: per phase set and per reported call inside the
 * set's span, what the reads tagged a show there and what the reads tagged b show there, and a haploid call on each.  Integers
 * only; defined on the alignments GAF, the node starts, the graph's letters, the rows of <out>-variants.tsv and the chain's ps and
 * flip alone (tests/haplotype_calls_ref.py recomputes it).
 *   calls        C graph bases cpos[0] < cpos[1] < .. (the rows of <out>-variants.tsv) and cref[c], the base's own letter: 0 .. 3
 *                for A C G T, 4 for anything else.  The sites pos, x, y with ps and flip are those of vga_phase_tags; they need not
 *                be a subset of the calls.
 *   shows        read r shows column k at base p (0 .. 3 A C G T, 4 other, 5 deleted, 6 inserts behind it) when it has a sparse
 *                word p << 3 | k, or, for k = cref (0 .. 4), when one of its runs [start, end) covers p.  A read shows a column at
 *                a base at most once, however often it consumes the base (a self-loop), and may show several columns there:
 *                these are counts of reads, not of events, and can lie below the pileup's on a base one read consumes twice.
 *   tag          tag(r, S) is a when votes_a > votes_b of the haplotag row (r, S), b when votes_b > votes_a; with a tie or no
 *                row there is none.  The rule of vga_phase_tags, on the same observation tile (k_ph_obs).
 *   jobs         first[S] and last[S] are the smallest and largest pos of the sites of set S.  A job (c, S) for every call with
 *                first[S] <= cpos[c] <= last[S] -- for every set: a set of one site has the one job at its own base if that base
 *                is a call.  Ordered by c, then by ps ascending; J is their number.
 *   counts       row j = (c, S) is 16 uint32: c, ps, a[0 .. 6], b[0 .. 6]; a[k] the kept reads with tag(r, S) = a that show
 *                column k at cpos[c], b[k] the same for b.
 *   haploid call of seven counts n, obs = n[0] + .. + n[5]: "." for obs = 0; else the first maximum of n[A], n[C], n[G], n[T],
 *                n[del] in the order A < C < G < T < D, which must hold 2 n > obs, else "?"; "+" is appended when obs > 0 and
 *                2 n[6] > obs.  No parameters: the strict majority is a choice, not a measurement.
 *   vga_haplotype_counts        the rows from the context's own store and the letters of its index; *n_reads the stored records
 *                               (may be NULL).  *n_rows = J is always written; with cap < J nothing is launched and no row is
 *                               written, and the caller asks again.  Per tile of reads k_ph_obs, k_hc_tags (a byte per set and
 *                               read), k_hc_cols (a byte per call and read) and k_hc_count (a workgroup per job); the tile's read
 *                               count is a multiple of 64 sized from 64 MiB and n_sites + sets + n_calls, VGA_PHASE_READ_TILE
 *                               overrides it, and the rows do not depend on it.  VGA_ERR_ARG for everything vga_phase_tags
 *                               refuses, for cpos not strictly ascending or not inside the graph, and for a NULL array with a
 *                               non-zero count; VGA_ERR_UNSUPPORTED for C or J above 2^24.  C = 0, n_sites = 0 or an empty
 *                               store: 0 rows.  Does not reset the store.
 *   vga_haplotype_counts_lists  the kernel seam, and the route of several contexts: the same from explicit records and words on
 *                               a graph of n_bases bases, with every check of vga_phase_tags_lists (the same code) and, on top,
 *                               cref <= 4; a violation is VGA_ERR_ARG, launches nothing and leaves rows and *n_rows as they
 *                               were.  Needs a context only.
 *   vga_haplotype_jobs          no context, on the host: the one definition of the job rule (csrc/vga_hapcall.hpp).  *n_jobs = J
 *                               always; the first cap jobs as pairs (c, ps).  VGA_ERR_ARG for cpos or pos not strictly ascending,
 *                               for a ps vga_phase_tags refuses, and for a NULL array it needs.
 *   vga_haplotype_call          no context: the one definition of the haploid call.  counts: 7; text: 3 bytes, "A" "C" "G" "T"
 *                               "-" "?" or ".", then "+" or nothing, then 0.
 * Without these calls nothing changes: no k_hc_* launch, no extra allocation. */
int vga_haplotype_counts(vga_ctx *ctx, uint64_t n_calls, const uint32_t *cpos /* n_calls */, uint64_t n_sites, const uint32_t *pos,
                         const uint8_t *x, const uint8_t *y, const uint32_t *ps, const uint8_t *flip, uint64_t cap,
                         uint32_t *rows /* cap * 16 */, uint64_t *n_rows, uint64_t *n_reads);
int vga_haplotype_counts_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs /* n_reads * 3 */, uint64_t n_words,
                               const uint32_t *words, uint64_t n_calls, const uint32_t *cpos, const uint8_t *cref, uint64_t n_sites,
                               const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint8_t *ref, const uint32_t *ps,
                               const uint8_t *flip, uint64_t cap, uint32_t *rows /* cap * 16 */, uint64_t *n_rows);
int vga_haplotype_jobs(uint64_t n_calls, const uint32_t *cpos, uint64_t n_sites, const uint32_t *pos, const uint32_t *ps, uint64_t cap,
                       uint32_t *jobs /* cap * 2 */, uint64_t *n_jobs);
int vga_haplotype_call(const uint32_t *counts /* 7 */, char *text /* 3 */);

/* ---- phase join: which phase sets of the chain the reads hold together ---------------------------------------
 * Stands in for nothing in the reference.  The chain links sites at most eight apart in site order and joins nothing again; a long
 * read is tagged in several sets at once, which is direct evidence about how the sets' haplotypes go together.  Integers only;
 * defined on the alignments GAF, the rows of <out>-variants.tsv and the chain's ps and flip alone (tests/phase_join_ref.py
 * recomputes it).
 *   sets         the S sets of ps in ascending ps (a set is named by the site that opens it), numbered 0 .. S - 1.
 *   tag          as for the haplotype counts: a for votes_a > votes_b of the haplotag row (r, s), b for votes_b > votes_a, none on a
 *                tie or without a row.  The rule of vga_phase_tags, on the same observation tile (k_ph_obs, k_hc_tags).
 *   table        for s <= t four uint32 n[2 i + j], i, j in 0 = a, 1 = b: the kept reads with tag(r, s) = i and tag(r, t) = j.  The
 *                S (S + 1) / 2 rows lie in the upper triangle, row-major: row s S - s (s - 1) / 2 + (t - s), the order of the
 *                genotype tables.  On the diagonal n[0] and n[3] are the reads tagged a and b in the set, n[1] = n[2] = 0.
 *   join rule    for s < t: cis = n[0] + n[3], trans = n[1] + n[2], diff = |cis - trans|; a link when diff >= min_reads (1 ..
 *                65 535; cis = trans is never one).  Links are taken by diff descending, then s, then t ascending.  A link whose
 *                sets are in different components at its turn joins them, the haplotypes related trans when trans > cis, else
 *                cis; a link inside one component joins nothing and is counted as agreeing or conflicting with the orientation the
 *                component already implies.  The smallest set of a component names it and keeps its orientation.
 *   vga_phase_set_links        the table from the context's own store; *n_reads the stored records (may be NULL).  *n_sets = S is
 *                              always written (0 without a site or with an empty store: zero rows); with cap_rows < S (S + 1) / 2
 *                              nothing is launched and no row is written, and the caller asks again.  Per tile of reads k_ph_obs,
 *                              k_hc_tags, k_sj_bits (two bit rows per set, 64 reads to a word) and k_sj_pairs (a workgroup per tile
 *                              of 32 x 32 set pairs); the table stays on the device across the tiles.  The tile's read count is a
 *                              multiple of 64 sized from 64 MiB, VGA_PHASE_READ_TILE overrides it, and the table does not depend on
 *                              it.  VGA_ERR_ARG for everything vga_phase_tags refuses; VGA_ERR_UNSUPPORTED for more than 4096 sets
 *                              (the table is 134 MB there), before anything is launched.  A refusal leaves the outputs as they
 *                              were.  Does not reset the store.
 *   vga_phase_set_links_lists  the kernel seam, and the route of several contexts: the same from explicit records and words on a
 *                              graph of n_bases bases, with every check of vga_phase_tags_lists (the same code).  Needs a context
 *                              only.
 *   vga_phase_join             no context, on the host: the one definition of the join rule (csrc/vga_phase_join.hpp).  set_root[s]:
 *                              the set that names the component of s; set_flip[s]: the parity of s against it; joins: the accepted
 *                              links in order as s, t, cis, trans (at most S - 1 of them; room for S - 1); *n_agree and *n_conflict:
 *                              the links inside a component.  Per site ps'[h] is the name of set_root of the set of h and flip'[h]
 *                              = flip[h] xor set_flip of it: what vga_phase_tags and vga_haplotype_counts take in the place of ps
 *                              and flip.  VGA_ERR_ARG for min_reads outside 1 .. 65 535, more than 4096 sets or a NULL array it needs.
 * Without these calls nothing changes: no k_sj_* launch, no extra allocation. */
int vga_phase_set_links(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint32_t *ps,
                        const uint8_t *flip, uint64_t cap_rows, uint32_t *table /* cap_rows * 4 */, uint64_t *n_sets, uint64_t *n_reads);
int vga_phase_set_links_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs /* n_reads * 3 */, uint64_t n_words,
                              const uint32_t *words, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y,
                              const uint8_t *ref, const uint32_t *ps, const uint8_t *flip, uint64_t cap_rows,
                              uint32_t *table /* cap_rows * 4 */, uint64_t *n_sets);
int vga_phase_join(uint64_t n_sets, const uint32_t *table /* n_sets (n_sets + 1) / 2 * 4 */, uint32_t min_reads, uint32_t *set_root /* n_sets */,
                   uint8_t *set_flip /* n_sets */, uint32_t *joins /* (n_sets - 1) * 4 */, uint64_t *n_joins, uint64_t *n_agree,
                   uint64_t *n_conflict);

/* ---- haplotype paths: which P line each haplotype of each phase set looks like -----------------------------
 * Stands in for nothing in the reference.  The path stages rank pairs of P lines from all reads at once; the phase stages separate
 * the reads of the two haplotypes without knowing a path.  Here each haplotype of each phase set gets a haploid ranking of the P
 * lines from its own reads.  Integers only; defined on the alignments GAF, the GFA's S and P lines, the rows of
 * <out>-variants.tsv and ps and flip alone (tests/haplotype_paths_ref.py recomputes it).
 *   kept reads   the records of the phase store, in store order (vga_phase_read).
 *   score        s[r][p], a 64-bit sum: bases[r][p] + edges[r][p] of the read's path-support row (source 0, support), or m - e of
 *                the edit distance, 0 for NONE (source 1, edit: the matrices the likelihood takes from it).
 *   deficit      d[r][p] = min(max_p' s[r][p'] - s[r][p], cap), one byte (the rule of the likelihood's deficits); cap 1 .. 255.
 *                Read r is scored when max_p' s[r][p'] > 0; an unscored read has an all-zero row and is in no group.
 *   sets, tag    as for the set links: the S sets in ascending ps; tag(r, s) the byte of k_hc_tags.
 *   groups       g = 2 s + h, h: 0 = a, 1 = b: the scored kept reads with tag(r, s) = h.  reads[g] their number; table[g][p] =
 *                (cost, best): cost = sum d[r][p], best = #{r : d[r][p] = 0}, uint64.  Exact; independent of read order, tile size
 *                and the store's row pitch.
 *   rank rule    a group is ranked when reads[g] > 0: its paths by cost ascending, then in P-line order; margin: the cost above
 *                rank 1; tied: the paths that attain the minimum.
 *   vga_haplotype_paths_begin  turns the deficit store on: from now on every vga_align_batch keeps a row of n_paths bytes (at a
 *                              pitch of whole 32-bit words) and a scored byte per kept read, beside the phase store (k_hp_keep, a
 *                              wave per winner).  After vga_path_support_begin and vga_phase_begin, and vga_path_edit_begin for
 *                              source 1: VGA_ERR_ARG otherwise, and for cap outside 1 .. 255.  The store grows by doubling
 *                              (VGA_HAP_PATHS_STORE_ROWS: its first size in rows); VGA_ERR_NOMEM from vga_align_batch, with the
 *                              reads kept, when it cannot.  vga_phase_begin / _reset empty it; vga_phase_end, vga_pileup_end,
 *                              vga_path_support_end and a new index drop it.
 *   vga_haplotype_paths_end    frees it and stops keeping.
 *   vga_haplotype_paths_store  deficits[n_reads * n_paths] dense and scored[n_reads]; the counts are always written, so a call
 *                              with NULL arrays sizes the next.
 *   vga_haplotype_paths        from the context's own stores and the letters of its index.  *n_sets = S is always written (0
 *                              without a site or with an empty store); with cap_groups < 2 S nothing is launched or written, and
 *                              the caller asks again.  Per tile of reads k_ph_obs, k_hc_tags and k_hp_sums (a workgroup per set
 *                              and 256 paths); reads and table stay on the device across the tiles.  VGA_ERR_UNSUPPORTED, with
 *                              *n_sets, before anything is launched, for more than 4096 sets or 2 S n_paths above 2^23 entries
 *                              (the table is 134 MB there).  VGA_ERR_ARG for everything vga_phase_tags refuses, and when the
 *                              store's rows are not the phase store's reads (it was turned on behind kept reads): every reader
 *                              refuses then.  A refusal leaves reads and table as they were.  Does not reset the stores.
 *   vga_haplotype_paths_lists  the kernel seam, and the route of several contexts: the same from explicit records, words, dense
 *                              deficits and scored bytes, with every check of vga_phase_tags_lists (the same code), n_paths
 *                              1 .. 4096 and scored <= 1.  Needs a context only.
 *   vga_haplotype_paths_rank   no context, on the host: the one definition of the rank rule (csrc/vga_hap_paths.hpp) on the
 *                              n_paths entries (cost, best) of one group.  VGA_ERR_ARG for n_paths outside 1 .. 4096 or a NULL.
 * Without vga_haplotype_paths_begin nothing changes: no k_hp_* launch, no extra allocation. */
#define VGA_HP_FROM_SUPPORT 0u
#define VGA_HP_FROM_EDIT 1u
int vga_haplotype_paths_begin(vga_ctx *ctx, uint32_t cap, uint32_t source);
int vga_haplotype_paths_end(vga_ctx *ctx);
int vga_haplotype_paths_store(vga_ctx *ctx, uint8_t *deficits /* n_reads * n_paths */, uint8_t *scored /* n_reads */, uint64_t *n_reads,
                              uint32_t *n_paths);
int vga_haplotype_paths(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint32_t *ps,
                        const uint8_t *flip, uint64_t cap_groups, uint64_t *reads /* cap_groups */,
                        uint64_t *table /* cap_groups * n_paths * 2 */, uint64_t *n_sets, uint64_t *n_reads);
int vga_haplotype_paths_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs /* n_reads * 3 */, uint64_t n_words,
                              const uint32_t *words, uint32_t n_paths, const uint8_t *deficits /* n_reads * n_paths */,
                              const uint8_t *scored /* n_reads */, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y,
                              const uint8_t *ref, const uint32_t *ps, const uint8_t *flip, uint64_t cap_groups, uint64_t *reads,
                              uint64_t *table, uint64_t *n_sets);
int vga_haplotype_paths_rank(uint32_t n_paths, const uint64_t *cost_best /* n_paths * 2 */, uint32_t *order /* n_paths */, uint32_t *tied);

/* ---- path abundance: the share of the reads that each P line explains, by expectation-maximisation ----------
 * Stands in for nothing in the reference.  The other path stages call a pair of P lines; this one fits a mixture over all paths at
 * once, which is what a mixed, pooled, contaminated or copy-number-variable sample needs.  Integers only (but for the table W,
 * which the library evaluates once on the host); defined on the alignments GAF and the GFA's S and P lines alone
 * (tests/path_abundance_ref.py recomputes it).
 *   rows      one per reported alignment of every vga_align_batch while the store is on, in the order they are reported:
 *             d[r][p] = min(max_p' s[r][p'] - s[r][p], cap), a byte, s as for the haplotype paths (source 0: bases + edges of path
 *             support; source 1: m - e of the edit distance, 0 for NONE); scored[r] = (max_p' s[r][p'] > 0).  Unscored rows take
 *             no part.  n: the scored rows; n >= 2^23 is VGA_ERR_UNSUPPORTED.
 *   table     W[d] = max(1, floor(65536 2^(-lambda d / 256) + 0.5)), d = 0 .. cap, forced non-increasing, W[0] = 65536; entries
 *             past cap repeat W[cap].  lambda 1 .. 4096 in 1/256 bit per unit of deficit, cap 1 .. 255.
 *   state     theta[p], uint32 in units of 2^-24; floor(2^24 / n_paths) for every path at the start.
 *   iteration for every scored row term[p] = theta[p] W[d[r][p]], z = sum_p term[p], resp[p] = floor((term[p] << 16) / z);
 *             S[p] = sum_r resp[p], total = sum_p S[p], theta'[p] = floor((S[p] << 24) / total), diff = max_p |theta'[p] - theta[p]|.
 *             The estimate stops after the first iteration with diff <= tol (converged) or after iters iterations.  iters
 *             1 .. 100 000, tol 0 .. 2^24.
 *   outputs   theta[n_paths]; reads_q16[n_paths], the S of the last iteration (expected reads x 65 536); best[n_paths], the scored
 *             rows with d = 0 on the path; n_scored, iterations, converged.  Any pointer may be NULL.  With n = 0: all zeros, 0
 *             iterations, not converged ("no call").  ppm(theta) = (theta * 1 000 000) >> 24.  Exact; independent of row order,
 *             batch split and row pitch.  A path whose theta reaches 0 stays at 0.
 *   vga_path_abundance_table  no context: out[0 .. 255] = W.  VGA_ERR_ARG for lambda or cap out of range or a NULL out.  The one
 *                             definition (csrc/vga_abundance.hpp).
 *   vga_path_abundance_begin  turns the store on: from now on every vga_align_batch keeps a row of n_paths bytes (at a pitch of
 *                             whole 32-bit words) and a scored byte per reported alignment (k_ab_keep, a wave per winner).  After
 *                             vga_path_support_begin, and vga_path_edit_begin for source 1: VGA_ERR_ARG otherwise, and for cap
 *                             outside 1 .. 255.  The store grows by doubling (VGA_PATH_ABUNDANCE_STORE_ROWS: its first size in
 *                             rows); VGA_ERR_NOMEM from vga_align_batch, with the reads kept, when it cannot.  A second begin
 *                             starts over; vga_path_support_end and a new index drop it.
 *   vga_path_abundance_reset  empties the store, keeps it on (VGA_ERR_ARG without _begin).
 *   vga_path_abundance_end    frees it and stops keeping (no error when it is off).
 *   vga_path_abundance_store  deficits[n_rows * n_paths] dense and scored[n_rows].  *n_rows is always written; with cap_rows below
 *                             it nothing is copied, and the caller asks again.
 *   vga_path_abundance        the estimate from the context's own store (k_ab_count once, then k_ab_estep and k_ab_mstep per
 *                             iteration, enqueued 32 iterations at a time; the result does not depend on that number).
 *                             VGA_ERR_ARG without _begin or for lambda, iters or tol out of range.  Does not reset the store.
 *   vga_path_abundance_rows   the kernel seam, and the route of several contexts: the same from explicit dense rows.  Needs a
 *                             context but no index.  Checked before anything is launched: a NULL array with n_rows > 0, n_paths
 *                             outside 1 .. 4096, lambda, iters or tol out of range, a scored byte above 1 (VGA_ERR_ARG).
 * vga_last_kernel_times names the launches of the first 32 iterations only.  Without vga_path_abundance_begin nothing changes: no
 * k_ab_* launch, no extra allocation. */
#define VGA_AB_FROM_SUPPORT 0u
#define VGA_AB_FROM_EDIT 1u
int vga_path_abundance_table(uint32_t lambda, uint32_t cap, uint32_t *out /* 256 */);
int vga_path_abundance_begin(vga_ctx *ctx, uint32_t cap, uint32_t source);
int vga_path_abundance_reset(vga_ctx *ctx);
int vga_path_abundance_end(vga_ctx *ctx);
int vga_path_abundance_store(vga_ctx *ctx, uint64_t cap_rows, uint8_t *deficits /* cap_rows * n_paths */, uint8_t *scored /* cap_rows */, uint64_t *n_rows);
int vga_path_abundance(vga_ctx *ctx, uint32_t lambda, uint32_t iters, uint32_t tol, uint32_t *theta /* n_paths */, uint64_t *reads_q16 /* n_paths */,
                       uint64_t *best /* n_paths */, uint64_t *n_scored, uint32_t *iterations, uint32_t *converged);
int vga_path_abundance_rows(vga_ctx *ctx, uint64_t n_rows, uint32_t n_paths, const uint8_t *deficits /* n_rows * n_paths */,
                            const uint8_t *scored /* n_rows */, uint32_t lambda, uint32_t iters, uint32_t tol, uint32_t *theta, uint64_t *reads_q16,
                            uint64_t *best, uint64_t *n_scored, uint32_t *iterations, uint32_t *converged);

/* Per-kernel timing of the most recent vga_map_batch / vga_poa_batch / vga_align_batch on this ctx:
 * name[i] / total milliseconds / launches, measured with hipEvents on the stream each launch ran on.
 * The POA sub-batches run two at a time on two streams: `ms` sums every launch's own duration (what
 * rocprofv3 --kernel-trace --stats reports), `busy_ms` is the wall time during which at least one launch
 * of that kernel was executing (the union of the launch intervals; equal to `ms` when nothing overlaps).
 * Returns the number of kernels (at most cap entries are written). */
typedef struct {
    const char *name;
    float ms;
    uint32_t launches;
    uint64_t algorithmic_bytes; /* byte model of DESIGN.md for the units those launches processed */
    float busy_ms;
    uint32_t reserved;
} vga_kernel_time;
int vga_last_kernel_times(const vga_ctx *ctx, vga_kernel_time *out, int cap);

#ifdef __cplusplus
}
#endif
#endif
