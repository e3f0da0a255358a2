// vga_genotype.hip -- the pair table of genotyping: k_gt_pairs and the five C entry points vga_genotype_begin / _read / _reset /
// _end / _pairs.  See vga_genotype.hpp for the measure, the shape of the kernel and the lane mapping.
//
// Overflow: bases can reach 2^18 per read and a call 32 768 reads, and the seam takes any 32-bit value, so no 32-bit running sum
// is safe.  The two sums are kept in 64 bits in registers from the first read on (an add and an add-with-carry per sum and
// pair-read) rather than flushed from 32-bit partials: a flush interval that is safe for 0xFFFFFFFF is one read.  The two counters
// count reads of one call and stay 32-bit until they are added to the table.
#include "vga_genotype.hpp"
#include "vga_path_support.hpp"

#include <algorithm>
#include <new>

namespace {

constexpr uint32_t GT_THREADS = 256u, GT_SUB = 4u;  // a thread's pairs: GT_SUB x GT_SUB, GT_TILE / GT_SUB = 16 threads on a side
static_assert(GT_TILE == 16u * GT_SUB && GT_THREADS == 16u * 16u, "a 16 x 16 thread grid covers the tile");
static_assert((GT_READS * GT_TILE) % GT_THREADS == 0, "staging: whole rounds per path range");

// blockIdx.x: the tile (tp, tq), tp <= tq, of the n_side x n_side tile grid in vga_pair_index order; blockIdx.y: the range of
// reads [y reads_per_group, (y + 1) reads_per_group) cut at n_reads.  table: four arrays of n_pairs words.
__global__ __launch_bounds__(256) void k_gt_pairs(uint32_t n_reads, uint32_t n_paths, uint32_t n_side, uint32_t reads_per_group,
                                                   const uint32_t *__restrict__ bases, const uint32_t *__restrict__ edges,
                                                   unsigned long long *__restrict__ table, unsigned long long n_pairs)
{
    __shared__ unsigned long long key_p[GT_READS][GT_TILE], key_q[GT_READS][GT_TILE];  // bases << 32 | edges of the tile's p range and q range
    uint32_t t = blockIdx.x, tp = 0;
    while (t >= n_side - tp) { t -= n_side - tp; tp++; }
    const uint32_t p0 = tp * GT_TILE, q0 = (tp + t) * GT_TILE;
    const uint32_t tid = threadIdx.x, tx = tid & 15u, ty = tid >> 4;
    const uint32_t r_begin = blockIdx.y * reads_per_group;
    const uint32_t r_end = min(n_reads, r_begin + reads_per_group);
    // a thread whose first p or first q is past the last path has no pair to store (few paths: most of the tile)
    const bool live = p0 + ty < n_paths && q0 + tx < n_paths;

    unsigned long long sum_b[GT_SUB][GT_SUB], sum_e[GT_SUB][GT_SUB];
    uint32_t pref_a[GT_SUB][GT_SUB], pref_b[GT_SUB][GT_SUB];
#pragma unroll
    for (uint32_t i = 0; i < GT_SUB; i++)
#pragma unroll
        for (uint32_t j = 0; j < GT_SUB; j++) { sum_b[i][j] = 0; sum_e[i][j] = 0; pref_a[i][j] = 0; pref_b[i][j] = 0; }

    for (uint32_t r0 = r_begin; r0 < r_end; r0 += GT_READS) {
        // 64 consecutive lanes read 64 consecutive paths of one read; a read or path past the end is staged as (0, 0), which
        // adds nothing and ties (its load goes to element 0, so that the rounds' loads are issued together, without branches).
        // One path range after the other: the loads of both at once cost the registers that keep a third wave off the SIMD.
        constexpr uint32_t ROUNDS = GT_READS * GT_TILE / GT_THREADS;  // per path range
#pragma unroll
        for (uint32_t side = 0; side < 2u; side++) {
            unsigned long long v[ROUNDS];
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const uint32_t idx = k * GT_THREADS + tid;
                const uint32_t r = r0 + idx / GT_TILE, path = (side ? q0 : p0) + idx % GT_TILE;
                const bool have = r < r_end && path < n_paths;
                const size_t at = have ? (size_t)r * n_paths + path : 0;
                const uint32_t b = bases[at], e = edges[at];
                v[k] = have ? ((unsigned long long)b << 32) | e : 0ull;
            }
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const uint32_t idx = k * GT_THREADS + tid;
                (side ? key_q : key_p)[idx / GT_TILE][idx % GT_TILE] = v[k];
            }
        }
        __syncthreads();
        if (live) {
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
    if (!live) return;
#pragma unroll
    for (uint32_t i = 0; i < GT_SUB; i++)
#pragma unroll
        for (uint32_t j = 0; j < GT_SUB; j++) {
            const uint32_t p = p0 + ty + 16u * i, q = q0 + tx + 16u * j;
            if (p > q || q >= n_paths) continue;
            const unsigned long long at = vga_pair_index(n_paths, p, q);
            if (sum_b[i][j]) atomicAdd(table + at, sum_b[i][j]);
            if (sum_e[i][j]) atomicAdd(table + n_pairs + at, sum_e[i][j]);
            if (pref_a[i][j]) atomicAdd(table + 2ull * n_pairs + at, (unsigned long long)pref_a[i][j]);
            if (pref_b[i][j]) atomicAdd(table + 3ull * n_pairs + at, (unsigned long long)pref_b[i][j]);
        }
}

// how the reads of a call are split: enough workgroups to fill the device when there are few tiles, never fewer than
// GT_MIN_CHUNKS chunks of GT_READS reads per workgroup (each workgroup ends with one atomic per pair and accumulator)
struct gt_split { uint32_t groups, reads_per_group; };
gt_split gt_groups(uint32_t n_reads, uint32_t n_tiles, int n_cu)
{
    const uint32_t chunks = (n_reads + GT_READS - 1u) / GT_READS;
    const uint32_t want = (4u * (uint32_t)std::max(n_cu, 1) + n_tiles - 1u) / n_tiles;
    const uint32_t most = std::max(1u, chunks / GT_MIN_CHUNKS);
    const uint32_t groups = std::max(1u, std::min({want, most, 65535u}));
    const uint32_t per = (chunks + groups - 1u) / groups;
    return {(chunks + per - 1u) / per, per * GT_READS};
}

void gt_launch(vga_ctx *ctx, uint32_t n_reads, uint32_t n_paths, const uint32_t *d_bases, const uint32_t *d_edges, unsigned long long *d_table)
{
    const uint32_t n_side = (n_paths + GT_TILE - 1u) / GT_TILE, n_tiles = (uint32_t)vga_pair_count(n_side);
    const gt_split s = gt_groups(n_reads, n_tiles, ctx->n_cu);
    const int t = vga_timer_begin(ctx, "k_gt_pairs", 0, ctx->stream);
    hipLaunchKernelGGL(k_gt_pairs, dim3(n_tiles, s.groups), dim3(GT_THREADS), 0, ctx->stream, n_reads, n_paths, n_side, s.reads_per_group, d_bases, d_edges,
                       d_table, (unsigned long long)vga_pair_count(n_paths));
    vga_timer_end(ctx, t);
}

// a device array of exactly n words (the table is 268 MB at 4096 paths: no slack)
int gt_table_alloc(vga_ctx *ctx, vga_dbuf<unsigned long long> &d, size_t n)
{
    vga_alloc_urgent urgent;
    VGA_HIP_CHECK_OOM(ctx, hipMalloc((void **)&d.p, n * sizeof(unsigned long long)));
    d.cap = n;
    return VGA_OK;
}

}  // namespace

struct gt_state {
    uint32_t n_paths = 0;
    uint64_t n_pairs = 0;
    vga_dbuf<unsigned long long> d_table;  // sum_bases, sum_edges, prefer_a, prefer_b: n_pairs words each
};

gt_state *gt_active(vga_ctx *ctx)
{
    ps_state *ps = ps_active(ctx);
    return ps ? ps->gt : nullptr;
}

int gt_add_call(vga_ctx *ctx, gt_state *gt, uint64_t n_reads, const uint32_t *d_bases, const uint32_t *d_edges)
{
    if (n_reads == 0) return VGA_OK;
    if (n_reads >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "genotype: too many reads in one call");
    gt_launch(ctx, (uint32_t)n_reads, gt->n_paths, d_bases, d_edges, gt->d_table.p);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
static void gt_release(ps_state *ps)
{
    if (ps->gt && ps->gt_free) ps->gt_free(ps->gt);
    ps->gt = nullptr;
    ps->gt_free = nullptr;
}

static int gt_zero(vga_ctx *ctx, gt_state *gt)
{
    VGA_HIP_CHECK(ctx, hipMemsetAsync(gt->d_table.p, 0, 4 * (size_t)gt->n_pairs * sizeof(unsigned long long), ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

extern "C" int vga_genotype_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_begin: path support is off (vga_path_support_begin)");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    gt_release(ps);  // (a second begin starts over)
    gt_state *gt = new (std::nothrow) gt_state();
    if (!gt) return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_genotype_begin: out of host memory");
    ps->gt = gt;
    ps->gt_free = [](gt_state *g) { delete g; };
    gt->n_paths = ps->n_paths;
    gt->n_pairs = vga_pair_count(ps->n_paths);
    int rc = gt_table_alloc(ctx, gt->d_table, 4 * (size_t)gt->n_pairs);
    if (rc == VGA_OK) rc = gt_zero(ctx, gt);
    if (rc != VGA_OK) gt_release(ps);
    return rc;
}

extern "C" int vga_genotype_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    gt_state *gt = gt_active(ctx);
    if (!gt) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_reset: genotyping is off (vga_genotype_begin)");
    (void)hipSetDevice(ctx->device);
    return gt_zero(ctx, gt);
}

extern "C" int vga_genotype_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return VGA_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    gt_release(ps);
    return VGA_OK;
}

extern "C" int vga_genotype_read(vga_ctx *ctx, uint64_t n_pairs, uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *prefer_a, uint64_t *prefer_b)
{
    if (!ctx) return VGA_ERR_ARG;
    gt_state *gt = gt_active(ctx);
    if (!gt) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_read: genotyping is off (vga_genotype_begin)");
    if (n_pairs != gt->n_pairs)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_read: the table has %llu pairs (%u paths), not %llu", (unsigned long long)gt->n_pairs, gt->n_paths,
                             (unsigned long long)n_pairs);
    (void)hipSetDevice(ctx->device);
    uint64_t *const dst[4] = {sum_bases, sum_edges, prefer_a, prefer_b};
    for (int k = 0; k < 4; k++)
        if (dst[k])
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(dst[k], gt->d_table.p + (size_t)k * gt->n_pairs, (size_t)gt->n_pairs * sizeof(uint64_t), hipMemcpyDeviceToHost,
                                              ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

// The kernel seam: explicit matrices through k_gt_pairs into a table of its own.
static int gt_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges, uint64_t *const dst[4])
{
    const size_t n_pairs = vga_pair_count(n_paths), cells = (size_t)n_reads * n_paths;
    hipStream_t st = ctx->stream;
    vga_dbuf<unsigned long long> d_table;
    vga_dbuf<uint32_t> d_b, d_e;
    int rc = gt_table_alloc(ctx, d_table, 4 * n_pairs);
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_table.p, 0, 4 * n_pairs * sizeof(unsigned long long), st));
    vga_timers_reset(ctx);
    if (n_reads) {
        VGA_HIP_CHECK_OOM(ctx, d_b.reserve(cells));
        VGA_HIP_CHECK_OOM(ctx, d_e.reserve(cells));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_b.p, bases, cells * 4, hipMemcpyHostToDevice, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_e.p, edges, cells * 4, hipMemcpyHostToDevice, st));
        gt_launch(ctx, (uint32_t)n_reads, n_paths, d_b.p, d_e.p, d_table.p);
        VGA_HIP_CHECK(ctx, hipGetLastError());
    }
    for (int k = 0; k < 4; k++)
        if (dst[k]) VGA_HIP_CHECK(ctx, hipMemcpyAsync(dst[k], d_table.p + (size_t)k * n_pairs, n_pairs * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
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
