// vga_genotype_lik.hpp -- the diploid read likelihood of every pair of haplotype paths (vga_genotype_lik.hip), as vga_align_batch
// sees it.
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  Like the pair table of vga_genotype.hpp, the
// cost is defined on the two reads x paths matrices path support leaves on the device after every vga_align_batch and on nothing
// else (tests/genotype_lik_ref.py recomputes it from them), in integers only.  With lambda in 1..4096 (the cost of one unit of
// deficit, in 1/256 bit) and cap in 1..255:
//   s[r][p] = bases[r][p] + edges[r][p]                     in 64 bits
//   d[r][p] = min(max over p' of s[r][p'] - s[r][p], cap)   the capped deficit: 0..255, a byte; an all-zero row has d = 0 everywhere
//   cost[p,q] += lambda min(d[r][p], d[r][q]) + T[|d[r][p] - d[r][q]|]     for every pair p <= q and every row r, in 64 bits
// which is -log2(1/2 2^(-lambda d_p) + 1/2 2^(-lambda d_q)) in 1/256 bit: either allele explains a read with probability 1/2.
// T is vga_gl_table below, the only place a logarithm is evaluated; the kernels receive the table.  n_scored counts the rows that
// have some s > 0.  The table of costs sits at vga_pair_index(n_paths, p, q), one 64-bit word per pair.
//
// Two kernels.  k_gl_deficit gives a wave a row: the lanes stride over the row's paths (coalesced along the path axis), reduce
// the maximum of s across the wave, and write the row's byte deficits.  k_gl_pairs stands on the frame of vga_pair_tile.hpp: a workgroup of 256
// threads owns a GL_TILE x GL_TILE tile of pairs of the upper triangle and a range of reads, stages the deficits of its two path
// ranges through LDS GL_READS reads at a time, keeps one 32-bit accumulator per pair in registers (8 x 8 pairs per thread,
// p = ty + 16 i, q = tx + 16 j), looks T up in LDS, and ends with one 64-bit atomic per pair.
#pragma once

#include <math.h>
#include <stdint.h>

// the paths on a side of a workgroup's tile, and the reads whose deficits it stages in LDS at a time
#define GL_TILE 128u
#define GL_READS 32u
// a workgroup takes at least this many chunks of GL_READS reads before the reads are split over more workgroups
#define GL_MIN_CHUNKS 4u
// ... and at most this many reads: the 32-bit accumulators of k_gl_pairs hold twice the cost (see the kernel), a read costs a pair
// at most 4096 * 255 + 256 = 1 044 736, and floor((2^32 - 1) / (2 * 1 044 736)) = 2055 reads fit; 2048 is 64 whole chunks
#define GL_MAX_GROUP_READS 2048u
#define GL_MAX_PATHS 4096u
#define GL_MAX_LAMBDA 4096u
#define GL_MAX_CAP 255u

// T[x] = round(256 (1 - log2(1 + 2^(-lambda x / 256)))) for x = 0..cap: what the second allele is worth, in 1/256 bit, when it
// fits the read x units worse.  T[0] = 0, T never decreases, T <= 256.  The one definition: vga_genotype_lik_table exports it, the
// library's kernels and the Python reference both take the table from there.
inline void vga_gl_table(uint32_t lambda, uint32_t cap, uint32_t *out)
{
    uint32_t prev = 0;
    for (uint32_t x = 0; x <= cap; x++) {
        const double y = exp2(-(double)lambda * (double)x / 256.0);
        const double v = floor(256.0 * (1.0 - log2(1.0 + y)) + 0.5);
        uint32_t t = x == 0 || v <= 0.0 ? 0u : v >= 256.0 ? 256u : (uint32_t)v;
        if (t < prev) t = prev;
        out[x] = prev = t;
    }
}

struct vga_ctx;
struct gl_state;
// the context's cost table while the likelihood is on (vga_genotype_lik_begin), else null
gl_state *gl_active(vga_ctx *ctx);
// k_gl_deficit and k_gl_pairs over the n_reads x n_paths matrices of the call that just ended, added into the context's cost table;
// launched on the context's stream and not waited for
int gl_add_call(vga_ctx *ctx, gl_state *gl, uint64_t n_reads, const uint32_t *d_bases, const uint32_t *d_edges);
// which matrices vga_align_batch hands to gl_add_call: VGA_GL_FROM_SUPPORT (path support's) or VGA_GL_FROM_EDIT (m - e and zeros,
// vga_path_edit.hpp); set by vga_genotype_lik_source
uint32_t gl_source(const gl_state *gl);
