// vga_poa_launch.hpp -- what the POA host code (vga_poa_run.hip, vga_poa_pool.hip) and the POA kernels (vga_poa.hip) share: the
// records that cross between host and device, and one typed launcher per kernel group.  The kernels themselves are visible
// in vga_poa.hip only.
#pragma once

#include "vga_common.hpp"
#include "vga_poa_shape.hpp"
#include "vga_subgraph.hpp"

#define POA_CHUNK (1ull << 20)
#define POA_RING_SPAN 32  // value rows read within this many nodes live in the per-problem ring, the others are kept
#define POA_SLOTS 4  // most sub-batches in flight (VGA_POA_SLOTS; default 2): own stream, pool segment and staging buffers each

#define POA_ST_OK 0
#define POA_ST_POOL 1
#define POA_ST_NOALN 2
#define POA_ST_TRACE 3
#define POA_ST_RETRY 5  // a specialised DP kernel hands the problem back: it is re-run by the general one (k_poa_dp_t4)

struct poa_prob {
    uint64_t node0;  // first entry of the node table (entry 0 of a problem is the virtual source)
    uint64_t pred0;  // first entry of the predecessor list (row ids)
    uint64_t sink0;  // first entry of the sink predecessor list
    uint64_t q0;     // first query byte
    uint64_t ops0;   // first entry of the traceback output
    uint64_t row0;   // first entry of the per-row arrays (rows 0..N)
    uint64_t seq0;   // first byte of the node sequences (row r is byte r-1)
    uint32_t n_sink;
    uint32_t qlen;
    uint32_t N;
    uint32_t w;      // adaptive band half-width: wb + floor(wf * qlen), computed on the host in double
    uint32_t n_nodes;  // node-table entries incl. the source
    uint32_t ring_rows;  // value rows of node-end rows live in a ring of this many worst-case rows
    uint32_t flags;      // bit 0: too large for an arena (reported as POA_ST_POOL at once)
    uint32_t pad;
};

struct poa_row {          // per DP row, 48 B
    int32_t beg, end;     // band
    uint64_t doff, voff;  // direction row / value row in the pool
    int32_t lmax, rmax;   // leftmost / rightmost column of the row maximum
    // the last four words form one aligned 16-byte group
    uint32_t pred, npred; // predecessor row or predecessor-list slice; npred != 0 only on the first row of a node
    int32_t base, hmax;   // base: k_poa_dp_t5 marks the rows whose value row is kept (its epilogue counts their cells), k_poa_dp_t4
                          // writes 0; hmax: unused
};
static_assert(sizeof(poa_row) == 48 && offsetof(poa_row, pred) == 32, "poa_row layout");

struct poa_out {          // per problem, 56 B
    int32_t score;
    uint32_t row;         // sink predecessor the traceback starts from
    int32_t status;
    uint32_t maxw;        // widest row (storage columns)
    uint64_t cells, vcells;
    uint32_t nops, pad;
    uint64_t t_begin, t_end;  // s_memrealtime (100 MHz) when the DP workgroup started / finished: occupancy diagnostics
};

struct poa_dev_params {
    int32_t match, mismatch, o1, e1, o2, e2, banded;
};

// The traceback pool of k_poa_dp_t5 (vga_poa_pool.hpp: poa_ws owns it).  Direction rows -- nine tenths of a problem's footprint, and
// unknown in size until the rows have been computed, because the band is adaptive -- come out of 1 MiB CHUNKS that a
// workgroup pops from a device-wide lock-free free list when it needs one and pushes back, all at once, when its traceback
// is done: what the pool has to hold is what the resident workgroups have written SO FAR, not a worst-case arena for each
// (rounds 1-2: 2 000 arenas of 128 MB = 257 GB of HBM for problems that use 20-55 MB; allocating and freeing that much
// dominated a 10 000-read run of the command line tool).  The chunks live in SEGMENTS that the host allocates on a thread
// of its own while launches already run (a chunk's address: seg_base[chunk >> cps_log2] + ((chunk & mask) << 20), the table
// in device memory, an entry written before its chunks are listed).  What must be contiguous -- the value-row ring, the two wide-row scratch rows, kept value rows --
// sits in a small fixed STATE region per resident workgroup, taken like an arena before (flag 0 -> 1).
// Offsets stored in the row records are absolute device addresses in this mode (pool base 0).
#define POA_NIL 0xFFFFFFFFu
#define POA_LISTS 64        // the free list is sharded: workgroups of a launch start together and run in step, so they ask for
#define POA_LIST_STRIDE 16  // chunks at the same moments -- one list head would serialise 2 000 compare-and-swap loops
struct poa_chunk_pool {
    unsigned long long *head;    // [POA_LISTS * POA_LIST_STRIDE] free lists: change counter << 32 | first free chunk (POA_NIL: none)
    uint32_t *next;              // per chunk: the next chunk of the list it is in (a free list, or its owner's)
    const uint64_t *seg_base;    // device address of every segment
    uint32_t cps_log2;           // chunks per segment, log2
    uint32_t n_slots;            // state regions (0: classic mode, no chunk pool)
    uint8_t *state_base;         // n_slots regions of state_size bytes
    uint64_t state_size;
    uint32_t *slot_flag;         // 0 free / 1 taken
    unsigned long long *stats;   // [0] requests that found every list empty (the host adds segments when it grows)
    uint32_t *owner;             // VGA_POOL_CHECK=1 (diagnostics, else null): per chunk, who holds it (0: a free list) -- a chunk popped while
                                 // held, or pushed by somebody else, counts in stats[4] / stats[5] and fails the call
    uint32_t *short_flag;        // pinned host memory: set to 1 with stats[0] -- the host's keeper thread reads (and clears) it
                                 // without any GPU work of its own (a copy of stats[0] waited 0.1-0.2 s for a slot on a full GPU)
};

// The launch arguments as one by-value struct: the row loop copies the few it needs into scalars of their own, and the
// epilogue reads the rest again through the kernarg pointer, so that nothing of it has to stay in registers over the rows.
struct poa_t5_args {
    const poa_prob *probs;
    const char *queries;
    const uint4 *node_tab;
    const uint32_t *seq32, *preds;
    poa_row *rows;
    uint8_t *pool;
    unsigned long long *pool_next;
    uint64_t pool_size;
    poa_out *outs;
    uint8_t *tb_ops;
    uint32_t *tb_orow;
    poa_chunk_pool cp;  // cp.n_slots != 0: direction rows out of the chunk pool, the rest out of a state region
    uint32_t lds_cols, hg_cols, win_mask;
    poa_dev_params P;
    uint32_t prio;  // != 0: the waves of this launch run at raised issue priority (the launch of a call's longest problems: their
                    // sequential rows decide how long the call takes, so they should not share issue slots evenly with the bulk)
};

struct poa_text_out {  // per problem, 48 B
    uint32_t cs_off, cs_len;      // bytes in the arena ("cs:Z:" included)
    uint32_t cg_off, cg_len;
    uint32_t runs_off, n_runs;    // byte offset (4-aligned) of n_runs node indices
    uint32_t n_path;              // graph-consuming alignment columns (abpoa_nodes.len())
    uint32_t start_off, end_off;  // aln_start_offset / aln_end_offset (align.rs:1155-1156)
    uint32_t aligned;             // n_aligned_bases
    uint32_t flags;               // 1: written; 2: no room in the arena (the host falls back to the operations)
    uint32_t pad;
};

// k_sg_gather: one part of the device store of vga_subgraph.hip
struct sg_gather_src {
    const uint4 *ntab;
    const uint32_t *preds, *sinks;
    const char *seq;
    uint32_t p0;
};

// ---- launchers (vga_poa.hip).  Each enqueues on `st` and returns the launch's own status (an older, ignored status is cleared first).
// The per-slot device buffers of a sub-batch as the kernels see them
struct poa_launch_bufs {
    const poa_prob *probs;
    const char *q;
    const uint4 *ntab;
    const uint32_t *seq32, *preds, *sink;
    poa_row *rows;
    poa_out *outs;
    uint8_t *ops;
    uint32_t *orow;
};

// k_sg_gather: one workgroup per staged problem copies its pieces out of the device store
hipError_t poa_launch_gather(hipStream_t st, uint32_t nb, const uint32_t *ids, const poa_prob *probs, const sg_off *offs, uint32_t split,
                             const sg_gather_src &s0, const sg_gather_src &s1, const char *reads, uint4 *ntab, uint32_t *preds, uint32_t *sinks,
                             char *seq, char *q);
// the DP kernel `sh` names, one workgroup per problem.  `a` carries every argument (k_poa_dp_lds and k_poa_dp_t4 take them one
// by one, and k_poa_dp_lds the sink rows besides); an uninstantiated workgroup size is hipErrorInvalidValue
hipError_t poa_launch_dp(int device, hipStream_t st, const poa_shape &sh, uint32_t nb, const poa_t5_args &a, const uint32_t *sink);
// the traceback as a kernel of its own (VGA_POA_TB=wave, k_poa_dp_lds), in the direction-code encoding of the DP kernel that ran
void poa_launch_traceback(hipStream_t st, poa_kernel dp, uint32_t nb, const poa_launch_bufs &b, const uint8_t *pool);
// k_poa_text: cs / CIGAR / node path of every problem into `arena`
hipError_t poa_launch_text(hipStream_t st, uint32_t nb, const poa_launch_bufs &b, char *arena, uint32_t arena_bytes, unsigned long long *cursor,
                           poa_text_out *touts);
// k_poa_text_to_host: n16 16-byte words from device memory to mapped host memory
hipError_t poa_launch_text_to_host(hipStream_t st, const uint4 *src, uint4 *dst, uint64_t n16);
// k_poa_chunks_add: chunks [first, first + count) of a new segment join the free lists
void poa_launch_chunks_add(hipStream_t st, const poa_chunk_pool &cp, uint32_t first, uint32_t count);
