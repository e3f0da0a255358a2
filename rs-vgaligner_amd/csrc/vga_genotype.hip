// vga_genotype.hip -- the pair table of genotyping: k_gt_pairs and the five C entry points vga_genotype_begin / _read / _reset /
// _end / _pairs.  See vga_genotype.hpp for the measure, the shape of the kernel and the lane mapping.
//
// Overflow: bases can reach 2^18 per read and a call 32 768 reads, and the seam takes any 32-bit value, so no 32-bit running sum
// is safe.  The two sums are kept in 64 bits in registers from the first read on (an add and an add-with-carry per sum and
// pair-read) rather than flushed from 32-bit partials: a flush interval that is safe for 0xFFFFFFFF is one read.  The two counters
// count reads of one call and stay 32-bit until they are added to the table.
#include "vga_genotype.hpp"
#include "vga_pair_tile.hpp"
#include "vga_path_support.hpp"

namespace {

constexpr uint32_t GT_THREADS = PAIR_TILE_THREADS, GT_SUB = 4u;  // a thread's pairs: GT_SUB x GT_SUB, GT_TILE / GT_SUB = 16 threads on a side
static_assert(GT_TILE == 16u * GT_SUB && GT_THREADS == 16u * 16u, "a 16 x 16 thread grid covers the tile");
static_assert((GT_READS * GT_TILE) % GT_THREADS == 0, "staging: whole rounds per path range");

// The tile and the reads of a workgroup: pair_tile_open (vga_pair_tile.hpp).  table: four arrays of n_pairs words.
__global__ __launch_bounds__(256) void k_gt_pairs(uint32_t n_reads, uint32_t n_paths, uint32_t n_side, uint32_t reads_per_group,
                                                   const uint32_t *__restrict__ bases, const uint32_t *__restrict__ edges,
                                                   unsigned long long *__restrict__ table, unsigned long long n_pairs)
{
    __shared__ unsigned long long key_p[GT_READS][GT_TILE], key_q[GT_READS][GT_TILE];  // bases << 32 | edges of the tile's p range and q range
    const pair_tile T = pair_tile_open<GT_TILE>(n_reads, n_paths, n_side, reads_per_group);
    const uint32_t tid = threadIdx.x, tx = T.tx, ty = T.ty, r_end = T.r_end;

    unsigned long long sum_b[GT_SUB][GT_SUB], sum_e[GT_SUB][GT_SUB];
    uint32_t pref_a[GT_SUB][GT_SUB], pref_b[GT_SUB][GT_SUB];
#pragma unroll
    for (uint32_t i = 0; i < GT_SUB; i++)
#pragma unroll
        for (uint32_t j = 0; j < GT_SUB; j++) { sum_b[i][j] = 0; sum_e[i][j] = 0; pref_a[i][j] = 0; pref_b[i][j] = 0; }

    for (uint32_t r0 = T.r_begin; r0 < r_end; r0 += GT_READS) {
        // a read or path past the end is staged as (0, 0), which adds nothing and ties (pair_tile_slot).  One path range after
        // the other: the loads of both at once cost the registers that keep a third wave off the SIMD.
        constexpr uint32_t ROUNDS = GT_READS * GT_TILE / GT_THREADS;  // per path range
#pragma unroll
        for (uint32_t side = 0; side < 2u; side++) {
            unsigned long long v[ROUNDS];
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot s = pair_tile_slot<GT_TILE>(T, n_paths, k, tid, r0, side);
                const size_t at = s.have ? (size_t)s.read * n_paths + s.path : 0;
                const uint32_t b = bases[at], e = edges[at];
                v[k] = s.have ? ((unsigned long long)b << 32) | e : 0ull;
            }
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot s = pair_tile_slot<GT_TILE>(T, n_paths, k, tid, r0, side);
                (side ? key_q : key_p)[s.row][s.col] = v[k];
            }
        }
        __syncthreads();
        if (T.live) {
            const uint32_t nr = min(GT_READS, r_end - r0);
            for (uint32_t rr = 0; rr < nr; rr++) {
                unsigned long long kp[GT_SUB], kq[GT_SUB];
#pragma unroll
                for (uint32_t i = 0; i < GT_SUB; i++) {
                    kp[i] = key_p[rr][ty + 16u * i];
                    kq[i] = key_q[rr][tx + 16u * i];
                }
#pragma unroll
                for (uint32_t i = 0; i < GT_SUB; i++)
#pragma unroll
                    for (uint32_t j = 0; j < GT_SUB; j++) {
                        const bool take_q = kq[j] > kp[i], take_p = kp[i] > kq[j];
                        const unsigned long long m = take_q ? kq[j] : kp[i];
                        sum_b[i][j] += m >> 32;
                        sum_e[i][j] += (uint32_t)m;
                        pref_a[i][j] += take_p ? 1u : 0u;
                        pref_b[i][j] += take_q ? 1u : 0u;
                    }
            }
        }
        __syncthreads();
    }
    if (!T.live) return;
    pair_tile_each<GT_SUB>(T, n_paths, [&](uint32_t i, uint32_t j, unsigned long long at) {
        if (sum_b[i][j]) atomicAdd(table + at, sum_b[i][j]);
        if (sum_e[i][j]) atomicAdd(table + n_pairs + at, sum_e[i][j]);
        if (pref_a[i][j]) atomicAdd(table + 2ull * n_pairs + at, (unsigned long long)pref_a[i][j]);
        if (pref_b[i][j]) atomicAdd(table + 3ull * n_pairs + at, (unsigned long long)pref_b[i][j]);
    });
}

void gt_launch(vga_ctx *ctx, uint32_t n_reads, uint32_t n_paths, const uint32_t *d_bases, const uint32_t *d_edges, unsigned long long *d_table)
{
    const uint32_t n_side = (n_paths + GT_TILE - 1u) / GT_TILE, n_tiles = (uint32_t)vga_pair_count(n_side);
    const vga_read_split s = vga_split_reads(n_reads, n_tiles, ctx->n_cu, GT_READS, GT_MIN_CHUNKS, VGA_SPLIT_NO_LIMIT);
    const int t = vga_timer_begin(ctx, "k_gt_pairs", 0, ctx->stream);
    hipLaunchKernelGGL(k_gt_pairs, dim3(n_tiles, s.groups), dim3(GT_THREADS), 0, ctx->stream, n_reads, n_paths, n_side, s.reads_per_group, d_bases, d_edges,
                       d_table, (unsigned long long)vga_pair_count(n_paths));
    vga_timer_end(ctx, t);
}

}  // namespace

// sum_bases, sum_edges, prefer_a, prefer_b: n_pairs words each
struct gt_state { pair_table table; };

gt_state *gt_active(vga_ctx *ctx)
{
    ps_state *ps = ps_active(ctx);
    return ps ? ps->gt.get() : nullptr;
}

int gt_add_call(vga_ctx *ctx, gt_state *gt, uint64_t n_reads, const uint32_t *d_bases, const uint32_t *d_edges)
{
    if (n_reads == 0) return VGA_OK;
    if (n_reads >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "genotype: too many reads in one call");
    gt_launch(ctx, (uint32_t)n_reads, gt->table.n_paths, d_bases, d_edges, gt->table.d.p);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_genotype_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_begin(ctx, "vga_genotype_begin", &ps_state::gt, [&](ps_state *ps, gt_state *gt) {
        const int rc = gt->table.alloc(ctx, ps->n_paths, 4, 0);
        return rc == VGA_OK ? gt->table.zero(ctx) : rc;
    });
}

extern "C" int vga_genotype_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    gt_state *gt = gt_active(ctx);
    return ps_child_reset(ctx, gt != nullptr, "vga_genotype_reset: genotyping is off (vga_genotype_begin)", [&]() { return gt->table.zero(ctx); });
}

extern "C" int vga_genotype_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_end(ctx, &ps_state::gt);
}

extern "C" int vga_genotype_read(vga_ctx *ctx, uint64_t n_pairs, uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *prefer_a, uint64_t *prefer_b)
{
    if (!ctx) return VGA_ERR_ARG;
    gt_state *gt = gt_active(ctx);
    if (!gt) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_read: genotyping is off (vga_genotype_begin)");
    const int rc = gt->table.check(ctx, "vga_genotype_read", n_pairs);
    if (rc != VGA_OK) return rc;
    (void)hipSetDevice(ctx->device);
    uint64_t *const dst[4] = {sum_bases, sum_edges, prefer_a, prefer_b};
    return gt->table.read(ctx, dst, nullptr);
}

// The kernel seam: explicit matrices through k_gt_pairs into a table of its own.
static int gt_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges, uint64_t *const dst[4])
{
    pair_table table;
    vga_dbuf<uint32_t> d_b, d_e;
    int rc = table.alloc(ctx, n_paths, 4, 0);
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, table.clear(ctx->stream));
    vga_timers_reset(ctx);
    if (n_reads) {
        if ((rc = pair_upload(ctx, (size_t)n_reads * n_paths, bases, edges, d_b, d_e)) != VGA_OK) return rc;
        gt_launch(ctx, (uint32_t)n_reads, n_paths, d_b.p, d_e.p, table.d.p);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) (void)hipStreamSynchronize(ctx->stream);  // (the two matrices are on their way)
        VGA_HIP_CHECK(ctx, e);
    }
    if ((rc = table.read(ctx, dst, nullptr)) != VGA_OK) return rc;
    vga_timers_collect(ctx);
    return VGA_OK;
}

extern "C" int vga_genotype_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges, uint64_t *sum_bases,
                                  uint64_t *sum_edges, uint64_t *prefer_a, uint64_t *prefer_b)
{
    if (!ctx) return VGA_ERR_ARG;
    if (n_paths == 0 || n_paths > GT_MAX_PATHS)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_pairs: %u paths, 1 to %u are paired", n_paths, GT_MAX_PATHS);
    if (n_reads && (!bases || !edges)) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_pairs: null matrix");
    if (n_reads >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_genotype_pairs: too many reads");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    uint64_t *const dst[4] = {sum_bases, sum_edges, prefer_a, prefer_b};
    return gt_pairs(ctx, n_reads, n_paths, bases, edges, dst);
}
