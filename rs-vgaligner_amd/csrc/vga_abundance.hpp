// vga_abundance.hpp -- the share of the reads that every haplotype path explains, fitted over all paths at once by
// expectation-maximisation (vga_path_abundance*, k_ab_keep, k_ab_count, k_ab_estep and k_ab_mstep in vga_abundance.hip).
//
// Nothing in the reference stands behind this: its map.rs ends at the GAF writer.  The other path stages call a pair of P lines;
// this one estimates a mixture.  While the store is on, k_ab_keep writes for every reported alignment r of every vga_align_batch a
// row of bytes d[r][p] = min(max_p' s[r][p'] - s[r][p], cap), s the 64-bit sum of the call's two reads x paths matrices (bases +
// edges of path support, or m - e and 0 of the edit distance: k_gl_deficit's rule), and a byte scored[r] = (max_p' s[r][p'] > 0).
// Unscored rows take no part; n is the number of scored rows (n >= 2^23: VGA_ERR_UNSUPPORTED).  Integers only from here on:
//   W[d]      = max(1, floor(65536 2^(-lambda d / 256) + 0.5)), d = 0 .. cap, forced non-increasing, W[0] = 65536; entries past
//               cap repeat W[cap] (vga_ab_table below: the only place a power is evaluated; the kernels receive the table)
//   theta[p]  uint32 in units of 2^-24, floor(2^24 / n_paths) for every path at the start
//   one iteration, over the scored rows r:
//     term[p]   = theta[p] W[d[r][p]]                        <= 2^40
//     z         = sum_p term[p]                              1 .. 2^40
//     resp[p]   = floor((term[p] << 16) / z)                 the numerator is <= 2^56
//     S[p]      = sum_r resp[p],  total = sum_p S[p]         total >= 16 n for n_paths <= 4096
//     theta'[p] = floor((S[p] << 24) / total)                S[p] << 24 < 2^64 because n < 2^23
//     diff      = max_p |theta'[p] - theta[p]|
//   the estimate stops after the first iteration with diff <= tol (converged) or after `iters` iterations.
// Outputs: theta, reads_q16 (the S of the last iteration: expected reads x 65 536), n_scored, iterations, converged; with n = 0
// all zeros, 0 iterations, not converged ("no call").  Sums of integers: exact, and independent of row order, batch split,
// workgroup size and row pitch.  A path whose theta reaches 0 stays at 0.
//
// The constants, the table, ppm and one iteration on the host are shared by host and device code; this header is plain C++ and
// compiles alone with a host compiler (tests/test_path_abundance_cpu.py does that).
#pragma once

#include <math.h>
#include <stdint.h>

// --abundance-lambda / -cap / -iters / -tol: choices, not measurements (README, "Path abundance")
#define AB_LAMBDA_DEFAULT 512u
#define AB_LAMBDA_MAX 4096u
#define AB_CAP_DEFAULT 64u
#define AB_CAP_MAX 255u
#define AB_ITERS_DEFAULT 1000u
#define AB_ITERS_MAX 100000u
#define AB_TOL_DEFAULT 16u
#define AB_TOL_MAX (1u << 24)
#define AB_MAX_PATHS 4096u
// the scored rows of one estimate: (S[p] << 24) stays below 2^64
#define AB_MAX_ROWS (1ull << 23)
// theta and resp are fixed point: 24 and 16 fractional bits
#define AB_THETA_BITS 24u
#define AB_RESP_BITS 16u
// the two matrices a score is summed from (vga_path_abundance_begin)
#define AB_FROM_SUPPORT 0u
#define AB_FROM_EDIT 1u
// k_ab_estep: a workgroup of AB_THREADS threads takes AB_GROUP_ROWS rows (times a whole factor of at most AB_MAX_ROW_FACTOR once
// there are more than AB_GROUP_ROWS AB_MAX_GROUPS rows) and AB_CHUNK_PATHS paths, AB_LANE_PATHS per lane
#define AB_THREADS 256u
#define AB_GROUP_ROWS 256u
#define AB_MAX_GROUPS 4096u
#define AB_MAX_ROW_FACTOR 8u
#define AB_LANE_PATHS 16u
#define AB_CHUNK_PATHS (64u * AB_LANE_PATHS)
// the host enqueues this many iterations before it reads the state record
#define AB_BLOCK_ITERS 32u
// the grow-only store's first size in rows
#define AB_STORE_ROWS0 4096ull

static inline bool vga_ab_params_ok(uint32_t lambda, uint32_t iters, uint32_t tol)
{
    return lambda >= 1u && lambda <= AB_LAMBDA_MAX && iters >= 1u && iters <= AB_ITERS_MAX && tol <= AB_TOL_MAX;
}

// The table, the one definition: vga_path_abundance_table exports it, the kernels and the Python reference take it from there.
// out: 256 entries.
static inline void vga_ab_table(uint32_t lambda, uint32_t cap, uint32_t *out)
{
    uint32_t prev = 1u << AB_RESP_BITS;
    for (uint32_t d = 0; d < 256u; d++) {
        if (d <= cap) {
            const double v = floor(65536.0 * exp2(-(double)lambda * (double)d / 256.0) + 0.5);
            uint32_t w = d == 0 || v >= 65536.0 ? 65536u : v <= 1.0 ? 1u : (uint32_t)v;
            if (w > prev) w = prev;
            prev = w;
        }
        out[d] = prev;
    }
}

// parts per million of a theta
static inline uint32_t vga_ab_ppm(uint32_t theta) { return (uint32_t)(((uint64_t)theta * 1000000ull) >> AB_THETA_BITS); }

// the lanes that serve a row: the smallest power of two >= min(n_paths, 64)
static inline uint32_t vga_ab_row_lanes(uint32_t n_paths)
{
    uint32_t g = 1;
    while (g < 64u && g < n_paths) g *= 2u;
    return g;
}

// the rows of a workgroup of k_ab_estep for n_rows rows: AB_GROUP_ROWS, times the whole factor that leaves at most AB_MAX_GROUPS
// workgroups, at most AB_MAX_ROW_FACTOR (more rows than that make more workgroups)
static inline uint32_t vga_ab_group_rows(uint64_t n_rows)
{
    const uint64_t per = (uint64_t)AB_GROUP_ROWS * AB_MAX_GROUPS;
    uint64_t f = n_rows > per ? (n_rows + per - 1u) / per : 1u;
    if (f > AB_MAX_ROW_FACTOR) f = AB_MAX_ROW_FACTOR;
    return (uint32_t)(f * AB_GROUP_ROWS);
}

// One iteration on the host, the definition restated for a stand-alone program: deficits: n_rows x n_paths dense; theta is
// replaced, S written.  -> diff.  (0 when no row is scored: theta stays.)
static inline uint32_t vga_ab_iterate_host(uint64_t n_rows, uint32_t n_paths, const uint8_t *deficits, const uint8_t *scored, const uint32_t *W, uint32_t *theta,
                                           uint64_t *S)
{
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_paths; p++) S[p] = 0;
    for (uint64_t r = 0; r < n_rows; r++) {
        if (!scored[r]) continue;
        const uint8_t *d = deficits + r * n_paths;
        uint64_t z = 0;
        for (uint32_t p = 0; p < n_paths; p++) z += (uint64_t)theta[p] * W[d[p]];
        if (!z) continue;
        for (uint32_t p = 0; p < n_paths; p++) S[p] += (((uint64_t)theta[p] * W[d[p]]) << AB_RESP_BITS) / z;
    }
    for (uint32_t p = 0; p < n_paths; p++) total += S[p];
    if (!total) return 0;
    uint32_t diff = 0;
    for (uint32_t p = 0; p < n_paths; p++) {
        const uint32_t t = (uint32_t)((S[p] << AB_THETA_BITS) / total);
        const uint32_t dd = t > theta[p] ? t - theta[p] : theta[p] - t;
        diff = dd > diff ? dd : diff;
        theta[p] = t;
    }
    return diff;
}

#ifdef __HIPCC__
#include "vga_common.hpp"

struct ab_state;
struct ps_state;
// the context's store while it is on (vga_path_abundance_begin, with path support on), else null
ab_state *ab_active(vga_ctx *ctx);
// the store reads the edit matrices: pe_add_call has to write them (ps_score_winners asks)
bool ab_from_edit(const ab_state *ab);
// k_ab_keep: the rows of the nw winners of the call that ps_score_winners has just scored (d_rows[i]: the read winner i is reported
// for, a row of the call's n_reads x n_paths matrices) join the store, on the context's stream; not waited for.  VGA_ERR_NOMEM when
// the store cannot grow.
int ab_keep_winners(vga_ctx *ctx, ab_state *ab, ps_state *ps, const uint32_t *d_rows, size_t nw);
#endif
