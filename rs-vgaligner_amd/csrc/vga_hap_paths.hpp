// vga_hap_paths.hpp -- which haplotype path each haplotype of each phase set looks like, from that haplotype's own reads
// (vga_haplotype_paths*, k_hp_keep and k_hp_sums in vga_hap_paths.hip, run on the tile frame of vga_phase.hip).
//
// Nothing in the reference stands behind this.  The path stages (vga_path_support.hpp, vga_genotype_lik.hpp) score every reported
// alignment against every P line and call a pair of paths from all reads at once; the phase stages (vga_phase.hpp,
// vga_phase_join.hpp) separate the reads of the two haplotypes without knowing a path.  Here the two meet.  While the deficit
// store is on, k_hp_keep writes for every kept read r of the phase store a row of bytes d[r][p] = min(max_p' s[r][p'] - s[r][p],
// cap), s the 64-bit sum of the call's two reads x paths matrices (bases + edges of path support, or m - e and 0 of the edit
// distance: k_gl_deficit's rule), and a byte scored[r] = (max_p' s[r][p'] > 0).  An unscored read has an all-zero row and is in no
// group.  tag(r, s) is the byte k_hc_tags writes, unchanged: a for votes_a > votes_b, b for votes_b > votes_a, nothing otherwise.
// Group g = 2 s + h (the S sets in ascending ps; h: 0 = a, 1 = b) holds the scored kept reads with tag(r, s) = h:
//   reads[g] their number, cost[g][p] = sum d[r][p], best[g][p] = #{r : d[r][p] = 0},
// sums of integers in 64 bits: exact, and independent of read order, tile size and row pitch.  The table holds (cost, best) per
// (group, path).  The measure is defined on the alignments GAF, the GFA's S and P lines, the rows of <out>-variants.tsv and ps and
// flip alone (tests/haplotype_paths_ref.py recomputes it).
//
// The constants, the store's row pitch and the rank rule are shared by host and device code; this header is plain C++ and compiles
// alone with a host compiler (tests/test_haplotype_paths_cpu.py does that).
#pragma once

#include <stdint.h>

// --haplotype-paths-cap: a choice, not a measurement (README, "Haplotype paths")
#define HP_CAP_DEFAULT 64u
#define HP_CAP_MAX 255u
// the two matrices a score is summed from (vga_haplotype_paths_begin)
#define HP_FROM_SUPPORT 0u
#define HP_FROM_EDIT 1u
// the paths of one call (PS_MAX_PATHS), its sets (PJ_MAX_SETS) and its table entries 2 S n_paths: the table is 134 MB there
#define HP_MAX_PATHS 4096u
#define HP_MAX_SETS 4096u
#define HP_MAX_ENTRIES (1ull << 23)
// an entry of the table: cost, best
#define HP_COLS 2u
// k_hp_sums: a workgroup owns one set and HP_CHUNK_PATHS paths, a lane four neighbouring ones (one 32-bit load of a row);
// its waves split the tile's 64-read words
#define HP_SUM_BLOCK 256u
#define HP_LANE_PATHS 4u
#define HP_CHUNK_PATHS (64u * HP_LANE_PATHS)
// the grow-only store's first size in rows
#define HP_STORE_ROWS0 4096ull

// the bytes from one row of the store to the next: whole 32-bit words, the bytes behind the last path zero
static inline uint32_t hp_pitch(uint32_t n_paths) { return (n_paths + 3u) & ~3u; }

// The rank rule, integer-only: the one definition (vga_haplotype_paths_rank exports it, Tables::write prints from it).
// cost_best: the n_paths entries (cost, best) of one group.  order: the paths by cost ascending, then in P-line order.  -> tied:
// the number of paths that attain the minimum cost (0 without a path).  The margin of a path is its cost above order[0]'s.
static inline uint32_t hp_rank(uint32_t n_paths, const uint64_t *cost_best, uint32_t *order)
{
    // a stable insertion by binary search: n_paths <= 4096, and the costs of one group are mostly distinct
    for (uint32_t p = 0; p < n_paths; p++) {
        const uint64_t c = cost_best[(uint64_t)p * HP_COLS];
        uint32_t lo = 0, hi = p;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cost_best[(uint64_t)order[mid] * HP_COLS] <= c) lo = mid + 1u; else hi = mid;
        }
        for (uint32_t k = p; k > lo; k--) order[k] = order[k - 1u];
        order[lo] = p;
    }
    uint32_t tied = 0;
    while (tied < n_paths && cost_best[(uint64_t)order[tied] * HP_COLS] == cost_best[(uint64_t)order[0] * HP_COLS]) tied++;
    return tied;
}

#ifdef __HIPCC__
#include "vga_common.hpp"

struct hp_state;
struct ps_state;
// the context's deficit store while it is on (vga_haplotype_paths_begin, with path support and the phase store on), else null
hp_state *hp_active(vga_ctx *ctx);
// the store reads the edit matrices: pe_add_call has to write them (ps_score_winners asks)
bool hp_from_edit(const hp_state *hp);
// k_hp_keep: the rows of the nw winners of the call that ps_score_winners has just scored (d_rows[i]: the read winner i is reported
// for, a row of the call's n_reads x n_paths matrices) join the store, on the context's stream; not waited for.  VGA_ERR_NOMEM when
// the store cannot grow.
int hp_keep_winners(vga_ctx *ctx, hp_state *hp, ps_state *ps, const uint32_t *d_rows, size_t nw);
// the store empties with the phase store (vga_phase_begin, vga_phase_reset)
void hp_empty(hp_state *hp);
// what a reader of the store takes: n_rows rows of pitch bytes for n_paths paths, and the scored bytes
struct hp_view {
    uint64_t n_rows;
    uint32_t n_paths, pitch;
    const uint8_t *d_deficits, *d_scored;
};
hp_view hp_view_of(const hp_state *hp);
// k_hp_sums over the n reads of one tile of the frame (tile_reads to a tag row, d_tags: S rows; rows: the store from the tile's
// first read on), added into d_reads (2 S words) and d_table (2 S n_paths entries), which the launch's workgroups own
int hp_sums_tile(vga_ctx *ctx, uint32_t n, uint32_t tile_reads, uint32_t n_sets, uint32_t n_paths, uint32_t pitch, const uint8_t *d_tags, const uint8_t *d_deficits,
                 const uint8_t *d_scored, unsigned long long *d_reads, unsigned long long *d_table);

// The row code of k_hp_keep, which the store of the path abundance (k_ab_keep, vga_abundance.hip) keeps its rows with as well.  A wave
// per winner i: row rows[i] of the call's two matrices, lanes over the paths as in k_gl_deficit (a path past the end is never
// loaded: 0 is the identity of an unsigned maximum), the maximum reduced over the wave, then the byte row and the scored byte of
// store row i.  The bytes behind the last path are written as zero.
__device__ __forceinline__ void hp_keep_row(uint32_t i, uint32_t lane, uint32_t n_paths, uint32_t pitch, uint32_t cap, const uint32_t *__restrict__ rows,
                                            const uint32_t *__restrict__ bases, const uint32_t *__restrict__ edges, uint8_t *__restrict__ deficits,
                                            uint8_t *__restrict__ scored)
{
    const size_t row = (size_t)rows[i] * n_paths;
    unsigned long long m = 0;
    for (uint32_t p = lane; p < n_paths; p += 64u) m = max(m, (unsigned long long)bases[row + p] + edges[row + p]);
#pragma unroll
    for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
    uint8_t *out = deficits + (size_t)i * pitch;
    for (uint32_t p = lane; p < pitch; p += 64u) {
        unsigned long long d = 0;
        if (p < n_paths) d = min(m - ((unsigned long long)bases[row + p] + edges[row + p]), (unsigned long long)cap);
        out[p] = (uint8_t)d;
    }
    if (lane == 0) scored[i] = m != 0 ? 1u : 0u;
}

// A grow-only store of deficit rows and scored bytes makes room for `at` rows: it doubles from first_rows on, and what is stored
// (n_rows rows) moves on the context's stream.  `what` names the store in the messages.  VGA_ERR_NOMEM, with the rows kept, when it
// cannot grow.
int hp_store_grow(vga_ctx *ctx, const char *what, uint8_t *&d_deficits, uint8_t *&d_scored, uint64_t &cap_rows, uint64_t n_rows, uint64_t first_rows,
                  uint32_t pitch, uint64_t at);
#endif
