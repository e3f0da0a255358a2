// vga_pair_index.hpp -- where the pair of paths (p, q), p <= q < n_paths, sits in a genotype table: the upper triangle, row-major;
// and how the reads of a call are split over the workgroups of a pair kernel.
//
// The one definition host and device code share: vga_genotype.hip and vga_genotype_lik.hip write their tables with it (k_gt_pairs,
// k_gl_pairs) and size their grids with it, the host library ranks the table with it (vgh_map.cpp), and the CPU tests compile this
// header alone with a host compiler.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VGA_PAIR_HD __host__ __device__ __forceinline__
#else
#define VGA_PAIR_HD inline
#endif

// P (P + 1) / 2: the pairs of a table over n_paths paths
VGA_PAIR_HD uint64_t vga_pair_count(uint64_t n_paths) { return n_paths * (n_paths + 1) / 2; }

// p P - p (p - 1) / 2 + (q - p): row p of the triangle starts after the P + (P - 1) + .. + (P - p + 1) pairs of the rows above it
VGA_PAIR_HD uint64_t vga_pair_index(uint64_t n_paths, uint64_t p, uint64_t q) { return p * n_paths - (p ? p * (p - 1) / 2 : 0) + (q - p); }

// How the reads of a call are split over the y dimension of a pair kernel's grid: enough workgroups to fill the device when there
// are few tiles (four per CU), never fewer than min_chunks chunks of reads_per_chunk reads per workgroup (each workgroup ends with
// one atomic per pair and accumulator), at most 65 535 workgroups, and never more than max_group_reads reads per workgroup (a
// multiple of the chunk; VGA_SPLIT_NO_LIMIT: none).  n_reads >= 1; no workgroup is empty: (groups - 1) reads_per_group < n_reads.
#define VGA_SPLIT_NO_LIMIT 0xFFFFFFFFu
struct vga_read_split { uint32_t groups, reads_per_group; };
VGA_PAIR_HD vga_read_split vga_split_reads(uint32_t n_reads, uint32_t n_tiles, int n_cu, uint32_t reads_per_chunk, uint32_t min_chunks,
                                           uint32_t max_group_reads)
{
    const uint32_t chunks = (n_reads + reads_per_chunk - 1u) / reads_per_chunk;
    const uint32_t want = (4u * (uint32_t)(n_cu > 1 ? n_cu : 1) + n_tiles - 1u) / n_tiles;
    const uint32_t most = chunks / min_chunks;
    uint32_t groups = want < most ? want : most;
    groups = groups > 65535u ? 65535u : groups < 1u ? 1u : groups;
    const uint32_t even = (chunks + groups - 1u) / groups, cap = max_group_reads / reads_per_chunk;
    const uint32_t per = even < cap ? even : cap;
    vga_read_split s;
    s.groups = (chunks + per - 1u) / per;
    s.reads_per_group = per * reads_per_chunk;
    return s;
}
