// vga_path_edit.hpp -- the edit distance of every reported alignment's read to every haplotype path (vga_path_edit.hip): the
// letter codes, the window rule, the block counts and the limits that host and device share, and what vga_path_support.hip and
// vga_genotype_lik.hip see of the state.  The CPU tests compile this header alone with a host compiler.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  The measure is defined on the alignments GAF,
// the GFA's S and P lines and the read sequences (include/vga_hip.h; tests/path_edit_ref.py recomputes it from them):
//   query    Q, m letters: the read, or its reverse complement for a '-' record; its node path w
//   anchor   a: the first node of w that path p visits as "id+", i: the FIRST such step of p;
//            b: the last node of w that p visits as "id+",       j: the LAST such step of p;   none, or j < i: NONE
//   window   lo = max(0, pos_p(i) - m), hi = min(|seq_p|, pos_p(j) + len(b) + m)
//   e[r][p]  min over lo <= s <= t <= hi of edit(Q, seq_p[s:t]), unit costs (Sellers: top row 0, minimum of the bottom row)
//
// Three kernels per vga_align_batch.  k_pe_jobs gives a wave an alignment and its lanes the paths: a lane scans the alignment's
// node list (what k_cov_runs left for path support) from both ends against bit p of the per-node path bitsets of k_ps_build, finds
// i and j with two binary searches in path p's sorted (node, step) array, and writes the job (query, lo, hi, path).  k_pe_dist<R>
// gives a wave a job and runs Myers' bit-vector algorithm in 64-row blocks with a carried horizontal delta, systolic over the
// lanes: lane l owns the R consecutive blocks l R .. l R + R - 1 of the query (Pv, Mv and the four match masks of each, in
// registers), at step t it takes text column t - l through its R blocks, and hands the horizontal delta that leaves its last
// block, with the column's letter, to lane l + 1 (one DPP wave shift).  A lane ahead of its first column sees a letter that
// matches nothing with delta 0, which leaves Pv = ~0, Mv = 0 as they are; the lane that owns row m follows the score from bit
// (m - 1) & 63 of its block's horizontal deltas and is at its last column when the loop ends, after n + lanes - 1 steps.
// k_pe_rows gives a wave a row of the matrix: the minimum over the scored paths and the per-path accumulators.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VGA_PE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define VGA_PE_HD inline
#endif

// e[r][p] of a pair that is not scored: no anchor, a placeholder record, a read longer than PE_MAX_QUERY
#define PE_NONE 0xFFFFFFFFu
// the blocks a lane of k_pe_dist owns: instantiated for 1, 2 and 4
#define PE_MAX_R 4u
// the longest query: 64 lanes of PE_MAX_R blocks of 64 rows
#define PE_MAX_QUERY (64u * 64u * PE_MAX_R)
// a letter that matches nothing, on either side
#define PE_CODE_OTHER 4u

// A C G T in either case -> 0..3, anything else -> PE_CODE_OTHER
VGA_PE_HD uint32_t pe_code(unsigned char c)
{
    const unsigned char u = (unsigned char)(c & 0xDFu);
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : PE_CODE_OTHER;
}
// the code of the complement
VGA_PE_HD uint32_t pe_code_complement(uint32_t code) { return code < 4u ? 3u - code : PE_CODE_OTHER; }

// 64-row blocks of a query of m letters
VGA_PE_HD uint32_t pe_blocks(uint32_t m) { return (m >> 6) + ((m & 63u) ? 1u : 0u); }
// the blocks per lane a query of m letters is served with: the smallest of 1, 2, 4 whose 64 lanes hold it; 0: too long
VGA_PE_HD uint32_t pe_blocks_per_lane(uint32_t m)
{
    const uint32_t nb = pe_blocks(m);
    return nb <= 64u ? 1u : nb <= 128u ? 2u : nb <= 256u ? 4u : 0u;
}
// the lanes in use (m >= 1, R = pe_blocks_per_lane(m) != 0), and the steps of a job over n text columns
VGA_PE_HD uint32_t pe_lanes(uint32_t m, uint32_t R) { return (pe_blocks(m) + R - 1u) / R; }
VGA_PE_HD uint64_t pe_steps(uint32_t m, uint32_t R, uint32_t n) { return n ? (uint64_t)n + pe_lanes(m, R) - 1u : 0u; }

// the window of path p for a query of m letters: pos_i, pos_j the offsets of steps i and j in seq_p, len_b the length of node b
struct pe_window { uint32_t lo, hi; };
VGA_PE_HD pe_window pe_window_of(uint32_t pos_i, uint32_t pos_j, uint32_t len_b, uint32_t m, uint32_t seq_len)
{
    const uint64_t end = (uint64_t)pos_j + len_b + m;
    pe_window w;
    w.lo = pos_i > m ? pos_i - m : 0u;
    w.hi = end < seq_len ? (uint32_t)end : seq_len;
    return w;
}

struct vga_ctx;
struct ps_state;
struct pe_state;
struct cov_win_view;
// the queries of the winners of a vga_align_batch: winner i is the len[i] letters at d_reads + off[i]
struct pe_queries {
    const char *d_reads;
    const uint64_t *off;
    const uint32_t *len;
};
// the context's path edit state while it is on (vga_path_edit_begin), else null
pe_state *pe_active(vga_ctx *ctx);
// the three kernels over the nw staged winners of the call that just ended (d_rows[i]: the read winner i is reported for), on the
// context's stream, not waited for; the call's n_reads x n_paths matrix is kept on the device for vga_path_edit_last.  with_gl:
// the matrices pe_gl_bases / pe_gl_edges (m - e, 0 for NONE; all zeros) are written for k_gl_deficit as well.
int pe_add_call(vga_ctx *ctx, ps_state *ps, const cov_win_view &v, const uint32_t *d_rows, uint64_t nw, uint64_t n_reads, const pe_queries &q, bool with_gl);
const uint32_t *pe_gl_bases(const pe_state *pe);
const uint32_t *pe_gl_edges(const pe_state *pe);
