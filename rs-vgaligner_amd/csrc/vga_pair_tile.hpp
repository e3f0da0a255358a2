// vga_pair_tile.hpp -- what the two pair stages share: genotyping's k_gt_pairs (vga_genotype.hip) and the read likelihood's
// k_gl_pairs (vga_genotype_lik.hip) are products of reads x paths matrices with a triangular output, and are tiled alike.  Here is
// the one copy of the frame of such a kernel (which tile and which reads a workgroup owns, which element a thread stages, which
// pairs it stores at the end) and of the host's table of pairs with the upload of a seam's two matrices.  Each kernel keeps what is
// its own: the staged type and its LDS layout, the arithmetic of a pair and a read, its accumulators and the pairs per thread.
// (The split of the reads over workgroups is vga_split_reads, vga_pair_index.hpp: the CPU tests compile it.)
#pragma once

#include "vga_common.hpp"
#include "vga_pair_index.hpp"

// ---------------------------------------------------------------------------------------------------------- device: the frame
// A workgroup of 256 threads, 16 on a side, owns a TILE x TILE tile of pairs and a range of reads; thread (ty, tx) owns the
// SUB x SUB pairs p = p0 + ty + 16 i, q = q0 + tx + 16 j, SUB = TILE / 16.
#define PAIR_TILE_THREADS 256u

// blockIdx.x: the tile (tp, tq), tp <= tq, of the n_side x n_side tile grid in vga_pair_index order; blockIdx.y: the range of
// reads [y reads_per_group, (y + 1) reads_per_group) cut at n_reads
struct pair_tile {
    uint32_t p0, q0, tx, ty, r_begin, r_end;
    bool live;  // false: the thread's first p or first q is past the last path, it has no pair to store (few paths: most of the tile)
};
template <uint32_t TILE>
__device__ __forceinline__ pair_tile pair_tile_open(uint32_t n_reads, uint32_t n_paths, uint32_t n_side, uint32_t reads_per_group)
{
    uint32_t t = blockIdx.x, tp = 0;
    while (t >= n_side - tp) { t -= n_side - tp; tp++; }
    pair_tile T;
    T.p0 = tp * TILE;
    T.q0 = (tp + t) * TILE;
    T.tx = threadIdx.x & 15u;
    T.ty = threadIdx.x >> 4;
    T.r_begin = blockIdx.y * reads_per_group;
    T.r_end = min(n_reads, T.r_begin + reads_per_group);
    T.live = T.p0 + T.ty < n_paths && T.q0 + T.tx < n_paths;
    return T;
}

// What thread tid stages in round k of a path range (side 0: the p range, 1: the q range) for the reads from r0 on: 64 consecutive
// lanes take 64 consecutive paths of one read.  row, col: the read within the chunk and the path within the range.  have false: the
// read or the path is past the end; the kernel then loads element 0 (so that the rounds' loads are issued together, without
// branches) and stages zero.
struct pair_slot {
    uint32_t row, col, read, path;
    bool have;
};
template <uint32_t TILE>
__device__ __forceinline__ pair_slot pair_tile_slot(const pair_tile &T, uint32_t n_paths, uint32_t k, uint32_t tid, uint32_t r0, uint32_t side)
{
    const uint32_t idx = k * PAIR_TILE_THREADS + tid;
    pair_slot s;
    s.row = idx / TILE;
    s.col = idx % TILE;
    s.read = r0 + s.row;
    s.path = (side ? T.q0 : T.p0) + s.col;
    s.have = s.read < T.r_end && s.path < n_paths;
    return s;
}

// f(i, j, at) for every pair of the thread that is in the table: at = vga_pair_index(n_paths, p, q).  A tile on the diagonal
// computes the whole square and stores p <= q.
template <uint32_t SUB, class F>
__device__ __forceinline__ void pair_tile_each(const pair_tile &T, uint32_t n_paths, F &&f)
{
#pragma unroll
    for (uint32_t i = 0; i < SUB; i++) {
        const uint32_t p = T.p0 + T.ty + 16u * i;
        const uint64_t row = vga_pair_index(n_paths, p, p);  // the diagonal opens row p of the triangle
#pragma unroll
        for (uint32_t j = 0; j < SUB; j++) {
            const uint32_t q = T.q0 + T.tx + 16u * j;
            if (p > q || q >= n_paths) continue;
            f(i, j, row + (q - p));
        }
    }
}

// ------------------------------------------------------------------------------------------------------ host: the pair table
// a device array of exactly n elements (the genotype table is 268 MB at 4096 paths: no slack)
template <typename T>
int pair_exact_alloc(vga_ctx *ctx, vga_dbuf<T> &d, size_t n)
{
    vga_alloc_urgent urgent;
    VGA_HIP_CHECK_OOM(ctx, hipMalloc((void **)&d.p, n * sizeof(T)));
    d.cap = n;
    return VGA_OK;
}

// `columns` arrays of n_pairs 64-bit words, one after the other, then `tail` words: what a stage holds while it is on, and what a
// seam holds for one call
struct pair_table {
    uint32_t n_paths = 0, columns = 0, tail = 0;
    uint64_t n_pairs = 0;
    vga_dbuf<unsigned long long> d;
    size_t words() const { return (size_t)columns * n_pairs + tail; }
    int alloc(vga_ctx *ctx, uint32_t paths, uint32_t n_columns, uint32_t tail_words)
    {
        n_paths = paths; columns = n_columns; tail = tail_words;
        n_pairs = vga_pair_count(paths);
        return pair_exact_alloc(ctx, d, words());
    }
    hipError_t clear(hipStream_t st) { return hipMemsetAsync(d.p, 0, words() * sizeof(unsigned long long), st); }
    // ... and waits for it
    int zero(vga_ctx *ctx)
    {
        VGA_HIP_CHECK(ctx, clear(ctx->stream));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        return VGA_OK;
    }
    // the caller of `who` sized its arrays for this table
    int check(vga_ctx *ctx, const char *who, uint64_t caller_pairs) const
    {
        if (caller_pairs == n_pairs) return VGA_OK;
        return vga_set_error(ctx, VGA_ERR_ARG, "%s: the table has %llu pairs (%u paths), not %llu", who, (unsigned long long)n_pairs, n_paths,
                             (unsigned long long)caller_pairs);
    }
    // column k to dst[k] where dst[k] is not null, the tail to tail_dst likewise; waits for the stream, also when a copy failed
    int read(vga_ctx *ctx, uint64_t *const *dst, uint64_t *tail_dst)
    {
        hipError_t e = hipSuccess;
        for (uint32_t k = 0; k < columns; k++)
            if (dst[k] && e == hipSuccess)
                e = hipMemcpyAsync(dst[k], d.p + (size_t)k * n_pairs, (size_t)n_pairs * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
        if (tail_dst && tail && e == hipSuccess)
            e = hipMemcpyAsync(tail_dst, d.p + (size_t)columns * n_pairs, tail * sizeof(uint64_t), hipMemcpyDeviceToHost, ctx->stream);
        const hipError_t es = hipStreamSynchronize(ctx->stream);
        VGA_HIP_CHECK(ctx, e);
        VGA_HIP_CHECK(ctx, es);
        return VGA_OK;
    }
};

// The two n_reads x n_paths host matrices of a seam (cells words each) to the device, on the context's stream.  The caller's host
// arrays are on their way from the first copy on: any failure drains the stream before it returns.
inline int pair_upload(vga_ctx *ctx, size_t cells, const uint32_t *bases, const uint32_t *edges, vga_dbuf<uint32_t> &d_b, vga_dbuf<uint32_t> &d_e)
{
    hipStream_t st = ctx->stream;
    hipError_t e = d_b.reserve(cells);
    if (e == hipSuccess) e = d_e.reserve(cells);
    if (e != hipSuccess) (void)hipStreamSynchronize(st);  // (what the caller enqueued before)
    VGA_HIP_CHECK_OOM(ctx, e);
    e = hipMemcpyAsync(d_b.p, bases, cells * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_e.p, edges, cells * 4, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) (void)hipStreamSynchronize(st);
    VGA_HIP_CHECK(ctx, e);
    return VGA_OK;
}
