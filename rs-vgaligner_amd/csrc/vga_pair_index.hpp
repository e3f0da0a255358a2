// vga_pair_index.hpp -- where the pair of paths (p, q), p <= q < n_paths, sits in a genotype table: the upper triangle, row-major.
//
// The one definition host and device code share: vga_genotype.hip writes the table with it (k_gt_pairs), the host library ranks
// the table with it (vgh_map.cpp), and the CPU tests compile this header alone with a host compiler.
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
