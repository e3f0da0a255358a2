// vga_genotype.hpp -- which pair of haplotype paths explains the reads best (vga_genotype.hip), as vga_align_batch sees it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  The measure is defined on the two reads x paths
// matrices path support leaves on the device after every vga_align_batch (vga_path_support.hpp) and on nothing else
// (tests/genotype_ref.py recomputes it from them).  With key[r][p] = (bases[r][p], edges[r][p]), compared lexicographically, the
// table holds for every pair p <= q
//   sum_bases, sum_edges   the components of max(key[r][p], key[r][q]) summed over the reads (a full tie takes p),
//   prefer_a, prefer_b     the reads with key[r][p] > key[r][q], and with key[r][q] > key[r][p],
// in 64 bits, at vga_pair_index(n_paths, p, q) of four arrays of vga_pair_count(n_paths) words laid out one after the other.
//
// k_gt_pairs is a product of the two matrices in the (max, +) semiring with a triangular output, and is tiled like one (the frame
// it shares with k_gl_pairs is vga_pair_tile.hpp).  A workgroup of 256 threads owns a tile of GT_TILE x GT_TILE pairs of the upper triangle (tiles below the diagonal are not
// launched; a tile on it computes the whole square and stores p <= q) and a range of reads.  It stages the keys of its two path
// ranges through LDS, GT_READS reads at a time, so a matrix element is read from HBM once per tile; a thread keeps the four
// accumulators of its 4 x 4 pairs (p = ty + 16 i, q = tx + 16 j) in registers over all its reads and adds them to the table with
// one 64-bit atomic each at the end.  With few tiles the reads are split over workgroups (vga_split_reads), which the atomics combine:
// integer sums do not depend on the order.  LDS rows are [read][path] with one 64-bit key (bases << 32 | edges) per path: the 16 lanes that share
// ty read 16 consecutive q keys (32 consecutive banks) and one broadcast p key, so no access conflicts.
#pragma once

#include "vga_common.hpp"
#include "vga_pair_index.hpp"

// the paths on a side of a workgroup's tile, and the reads whose keys it stages in LDS at a time (2 x GT_READS x GT_TILE x 8 bytes)
#define GT_TILE 64u
#define GT_READS 32u
// a workgroup takes at least this many chunks of GT_READS reads before the reads are split over more workgroups
#define GT_MIN_CHUNKS 4u
#define GT_MAX_PATHS 4096u

struct gt_state;
// the context's pair table while genotyping is on (vga_genotype_begin), else null
gt_state *gt_active(vga_ctx *ctx);
// k_gt_pairs over the n_reads x n_paths matrices of the call that just ended, added into the context's pair table; launched on the
// context's stream and not waited for
int gt_add_call(vga_ctx *ctx, gt_state *gt, uint64_t n_reads, const uint32_t *d_bases, const uint32_t *d_edges);
