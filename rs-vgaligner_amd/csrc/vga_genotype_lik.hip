// vga_genotype_lik.hip -- the diploid read likelihood of every pair of paths: k_gl_deficit, k_gl_pairs and the C entry points
// vga_genotype_lik_begin / _read / _reset / _end / _pairs / _table.  See vga_genotype_lik.hpp for the cost, the shape of the
// kernels and the lane mapping.
//
// Overflow.  k_gl_pairs keeps TWICE the cost of a pair in one 32-bit register: LDS holds 2 d and 2 T, so that the absolute
// difference of two staged values is the byte offset of its table entry and no shift is needed per pair-read.  One read adds at
// most 2 (lambda cap + T[cap]) <= 2 (4096 * 255 + 256) = 2 089 472 to a register, so floor((2^32 - 1) / 2 089 472) = 2055 reads
// fit; a workgroup takes at most GL_MAX_GROUP_READS = 2048 (vga_split_reads), which makes the flush interval the workgroup's own end:
// there it halves the register (exact: every addend is even) and adds it to the 64-bit table with one atomic.  A call of more
// reads is split over more workgroups, and the atomics combine them in 64 bits.
#include "vga_genotype_lik.hpp"
#include "vga_pair_tile.hpp"
#include "vga_path_edit.hpp"
#include "vga_path_support.hpp"

#include <algorithm>

namespace {

constexpr uint32_t GL_THREADS = PAIR_TILE_THREADS, GL_SUB = 8u;  // a thread's pairs: GL_SUB x GL_SUB, GL_TILE / GL_SUB = 16 threads on a side
static_assert(GL_TILE == 16u * GL_SUB && GL_THREADS == 16u * 16u, "a 16 x 16 thread grid covers the tile");
static_assert((GL_READS * GL_TILE) % GL_THREADS == 0, "staging: whole rounds per path range");
static_assert(2ull * (GL_MAX_LAMBDA * GL_MAX_CAP + 256ull) * GL_MAX_GROUP_READS <= 0xFFFFFFFFull, "a workgroup's reads fit the 32-bit accumulators");
static_assert(GL_MAX_GROUP_READS % GL_READS == 0, "a workgroup takes whole chunks");

// A wave per row, the rows dealt round the waves of the grid.  Lane l takes the paths l, l + 64, ..: a path past the end is never
// loaded, so it cannot enter the maximum (0 is the identity of an unsigned maximum: a lane without a path holds it).
__global__ __launch_bounds__(256) void k_gl_deficit(uint32_t n_reads, uint32_t n_paths, uint32_t cap, const uint32_t *__restrict__ bases,
                                                     const uint32_t *__restrict__ edges, uint8_t *__restrict__ deficit, unsigned long long *__restrict__ n_scored)
{
    const uint32_t lane = threadIdx.x & 63u, n_waves = gridDim.x * (GL_THREADS / 64u);
    uint32_t scored = 0;
    for (uint32_t r = blockIdx.x * (GL_THREADS / 64u) + (threadIdx.x >> 6); r < n_reads; r += n_waves) {
        const size_t row = (size_t)r * n_paths;
        unsigned long long m = 0;
        for (uint32_t p = lane; p < n_paths; p += 64u) m = max(m, (unsigned long long)bases[row + p] + edges[row + p]);
#pragma unroll
        for (int off = 32; off; off >>= 1) m = max(m, __shfl_xor(m, off));
        scored += m != 0 ? 1u : 0u;
        for (uint32_t p = lane; p < n_paths; p += 64u) {
            const unsigned long long s = (unsigned long long)bases[row + p] + edges[row + p];
            deficit[row + p] = (uint8_t)min(m - s, (unsigned long long)cap);
        }
    }
    if (lane == 0 && scored) atomicAdd(n_scored, (unsigned long long)scored);
}

// The tile and the reads of a workgroup: pair_tile_open (vga_pair_tile.hpp), reads_per_group <= GL_MAX_GROUP_READS.  table2: 256
// entries, 2 T[x] (x past cap repeats T[cap] and is never indexed: both deficits are <= cap).  cost: n_pairs words.
__global__ __launch_bounds__(256) void k_gl_pairs(uint32_t n_reads, uint32_t n_paths, uint32_t n_side, uint32_t reads_per_group, uint32_t lambda,
                                                   const uint8_t *__restrict__ deficit, const uint16_t *__restrict__ table2,
                                                   unsigned long long *__restrict__ cost)
{
    // 2 d of the tile's p range and q range.  The path at offset o of its range sits at (o % 16) * 8 + o / 16 of its row, so the
    // eight paths ty + 16 i of a thread are 16 consecutive bytes
    __shared__ __attribute__((aligned(16))) uint16_t d_p[GL_READS][GL_TILE];
    __shared__ __attribute__((aligned(16))) uint16_t d_q[GL_READS][GL_TILE];
    __shared__ uint16_t t2[256];
    const pair_tile T = pair_tile_open<GL_TILE>(n_reads, n_paths, n_side, reads_per_group);
    const uint32_t tid = threadIdx.x, tx = T.tx, ty = T.ty, r_end = T.r_end;
    t2[tid] = table2[tid];  // (the first barrier of the loop below comes before its first use)

    uint32_t acc[GL_SUB][GL_SUB];  // twice the cost of the thread's pairs over the workgroup's reads
#pragma unroll
    for (uint32_t i = 0; i < GL_SUB; i++)
#pragma unroll
        for (uint32_t j = 0; j < GL_SUB; j++) acc[i][j] = 0;

    for (uint32_t r0 = T.r_begin; r0 < r_end; r0 += GL_READS) {
        // a read or path past the end is staged as 0 (pair_tile_slot) and is never stored to the table
        constexpr uint32_t ROUNDS = GL_READS * GL_TILE / GL_THREADS;  // per path range
#pragma unroll
        for (uint32_t side = 0; side < 2u; side++) {
            uint32_t v[ROUNDS];
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot s = pair_tile_slot<GL_TILE>(T, n_paths, k, tid, r0, side);
                const uint32_t d = deficit[s.have ? (size_t)s.read * n_paths + s.path : 0];
                v[k] = s.have ? 2u * d : 0u;
            }
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot s = pair_tile_slot<GL_TILE>(T, n_paths, k, tid, r0, side);
                (side ? d_q : d_p)[s.row][(s.col & 15u) * GL_SUB + (s.col >> 4)] = (uint16_t)v[k];
            }
        }
        __syncthreads();
        if (T.live) {
            const uint32_t nr = min(GL_READS, r_end - r0);
            for (uint32_t rr = 0; rr < nr; rr++) {
                const uint4 wp = *reinterpret_cast<const uint4 *>(&d_p[rr][ty * GL_SUB]);
                const uint4 wq = *reinterpret_cast<const uint4 *>(&d_q[rr][tx * GL_SUB]);
                const uint32_t a[GL_SUB] = {wp.x & 0xFFFFu, wp.x >> 16, wp.y & 0xFFFFu, wp.y >> 16, wp.z & 0xFFFFu, wp.z >> 16, wp.w & 0xFFFFu, wp.w >> 16};
                const uint32_t b[GL_SUB] = {wq.x & 0xFFFFu, wq.x >> 16, wq.y & 0xFFFFu, wq.y >> 16, wq.z & 0xFFFFu, wq.z >> 16, wq.w & 0xFFFFu, wq.w >> 16};
                // a row of eight pairs at a time: the eight table entries are asked for together, and the products that do not
                // need them are computed while they are on their way (the two barriers hold that order: 2.5 to 5 % faster than
                // the compiler's own)
#pragma unroll
                for (uint32_t i = 0; i < GL_SUB; i++) {
                    uint32_t tt[GL_SUB];
#pragma unroll
                    for (uint32_t j = 0; j < GL_SUB; j++)  // 2 |d_p - d_q| is the byte offset of 2 T[|d_p - d_q|]
                        tt[j] = *reinterpret_cast<const uint16_t *>(reinterpret_cast<const char *>(t2) + __builtin_amdgcn_sad_u16(a[i], b[j], 0u));
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (uint32_t j = 0; j < GL_SUB; j++) acc[i][j] += __umul24(min(a[i], b[j]), lambda);
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (uint32_t j = 0; j < GL_SUB; j++) acc[i][j] += tt[j];
                }
            }
        }
        __syncthreads();
    }
    if (!T.live) return;
    pair_tile_each<GL_SUB>(T, n_paths, [&](uint32_t i, uint32_t j, unsigned long long at) {
        if (acc[i][j]) atomicAdd(cost + at, (unsigned long long)(acc[i][j] >> 1));
    });
}

// the reads of one call: the y dimension of k_gl_pairs' grid holds 65 535 workgroups of GL_MAX_GROUP_READS reads
constexpr uint64_t GL_MAX_CALL_READS = 65535ull * GL_MAX_GROUP_READS;

// d_cost: n_pairs words of cost, then the word of n_scored
void gl_launch(vga_ctx *ctx, uint32_t n_reads, uint32_t n_paths, uint32_t lambda, uint32_t cap, const uint32_t *d_bases, const uint32_t *d_edges,
               uint8_t *d_deficit, const uint16_t *d_table2, unsigned long long *d_cost)
{
    const uint32_t waves = GL_THREADS / 64u;
    const uint32_t blocks = std::min((n_reads + waves - 1u) / waves, 8u * (uint32_t)std::max(ctx->n_cu, 1));
    int t = vga_timer_begin(ctx, "k_gl_deficit", 0, ctx->stream);
    hipLaunchKernelGGL(k_gl_deficit, dim3(blocks), dim3(GL_THREADS), 0, ctx->stream, n_reads, n_paths, cap, d_bases, d_edges, d_deficit,
                       d_cost + vga_pair_count(n_paths));
    vga_timer_end(ctx, t);
    const uint32_t n_side = (n_paths + GL_TILE - 1u) / GL_TILE, n_tiles = (uint32_t)vga_pair_count(n_side);
    const vga_read_split s = vga_split_reads(n_reads, n_tiles, ctx->n_cu, GL_READS, GL_MIN_CHUNKS, GL_MAX_GROUP_READS);
    t = vga_timer_begin(ctx, "k_gl_pairs", 0, ctx->stream);
    hipLaunchKernelGGL(k_gl_pairs, dim3(n_tiles, s.groups), dim3(GL_THREADS), 0, ctx->stream, n_reads, n_paths, n_side, s.reads_per_group, lambda, d_deficit,
                       d_table2, d_cost);
    vga_timer_end(ctx, t);
}

bool gl_params_ok(uint32_t lambda, uint32_t cap) { return lambda >= 1u && lambda <= GL_MAX_LAMBDA && cap >= 1u && cap <= GL_MAX_CAP; }

// 2 T[x] for x = 0..255, the entries past cap repeating the last; h2 must outlive the copy (the callers synchronise the stream)
int gl_table_upload(vga_ctx *ctx, uint32_t lambda, uint32_t cap, uint16_t *h2, vga_dbuf<uint16_t> &d_table2)
{
    uint32_t t[256];
    vga_gl_table(lambda, cap, t);
    for (uint32_t x = 0; x < 256u; x++) h2[x] = (uint16_t)(2u * t[std::min(x, cap)]);
    int rc = pair_exact_alloc(ctx, d_table2, 256);
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_table2.p, h2, 256 * sizeof(uint16_t), hipMemcpyHostToDevice, ctx->stream));
    return VGA_OK;
}

}  // namespace

struct gl_state {
    uint32_t lambda = 0, cap = 0;
    uint32_t source = VGA_GL_FROM_SUPPORT;
    uint16_t h_table2[256] = {};
    vga_dbuf<uint16_t> d_table2;
    pair_table cost;              // n_pairs words of cost, then n_scored
    vga_dbuf<uint8_t> d_deficit;  // the byte deficits of the last call, n_reads x n_paths (grow-only)
};

gl_state *gl_active(vga_ctx *ctx)
{
    ps_state *ps = ps_active(ctx);
    return ps ? ps->gl.get() : nullptr;
}

uint32_t gl_source(const gl_state *gl) { return gl->source; }

int gl_add_call(vga_ctx *ctx, gl_state *gl, uint64_t n_reads, const uint32_t *d_bases, const uint32_t *d_edges)
{
    if (n_reads == 0) return VGA_OK;
    if (n_reads > GL_MAX_CALL_READS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "genotype likelihood: too many reads in one call");
    VGA_HIP_CHECK_OOM(ctx, gl->d_deficit.reserve((size_t)n_reads * gl->cost.n_paths));
    gl_launch(ctx, (uint32_t)n_reads, gl->cost.n_paths, gl->lambda, gl->cap, d_bases, d_edges, gl->d_deficit.p, gl->d_table2.p, gl->cost.d.p);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_genotype_lik_table(uint32_t lambda, uint32_t cap, uint32_t *out)
{
    if (!gl_params_ok(lambda, cap) || !out) return VGA_ERR_ARG;
    vga_gl_table(lambda, cap, out);
    return VGA_OK;
}

extern "C" int vga_genotype_lik_begin(vga_ctx *ctx, uint32_t lambda, uint32_t cap)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!gl_params_ok(lambda, cap))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_begin: lambda %u, cap %u: lambda is 1 to %u and cap 1 to %u", lambda, cap, GL_MAX_LAMBDA, GL_MAX_CAP);
    return ps_child_begin(ctx, "vga_genotype_lik_begin", &ps_state::gl, [&](ps_state *ps, gl_state *gl) {
        gl->lambda = lambda;
        gl->cap = cap;
        int rc = gl->cost.alloc(ctx, ps->n_paths, 1, 1);
        if (rc == VGA_OK) rc = gl_table_upload(ctx, lambda, cap, gl->h_table2, gl->d_table2);
        return rc == VGA_OK ? gl->cost.zero(ctx) : rc;
    });
}

extern "C" int vga_genotype_lik_source(vga_ctx *ctx, uint32_t source)
{
    if (!ctx) return VGA_ERR_ARG;
    gl_state *gl = gl_active(ctx);
    if (!gl) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_source: the likelihood is off (vga_genotype_lik_begin)");
    if (source != VGA_GL_FROM_SUPPORT && source != VGA_GL_FROM_EDIT)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_source: %u is neither VGA_GL_FROM_SUPPORT nor VGA_GL_FROM_EDIT", source);
    if (source == VGA_GL_FROM_EDIT && !pe_active(ctx))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_source: the edit distance is off (vga_path_edit_begin)");
    gl->source = source;
    return VGA_OK;
}

extern "C" int vga_genotype_lik_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    gl_state *gl = gl_active(ctx);
    return ps_child_reset(ctx, gl != nullptr, "vga_genotype_lik_reset: the likelihood is off (vga_genotype_lik_begin)", [&]() { return gl->cost.zero(ctx); });
}

extern "C" int vga_genotype_lik_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_end(ctx, &ps_state::gl);
}

extern "C" int vga_genotype_lik_read(vga_ctx *ctx, uint64_t n_pairs, uint64_t *cost, uint64_t *n_scored)
{
    if (!ctx) return VGA_ERR_ARG;
    gl_state *gl = gl_active(ctx);
    if (!gl) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_read: the likelihood is off (vga_genotype_lik_begin)");
    const int rc = gl->cost.check(ctx, "vga_genotype_lik_read", n_pairs);
    if (rc != VGA_OK) return rc;
    (void)hipSetDevice(ctx->device);
    return gl->cost.read(ctx, &cost, n_scored);
}

// The kernel seam: explicit matrices through k_gl_deficit and k_gl_pairs into a table of its own.
static int gl_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges, uint32_t lambda, uint32_t cap,
                    uint8_t *deficit_out, uint64_t *cost_out, uint64_t *n_scored)
{
    const size_t cells = (size_t)n_reads * n_paths;
    hipStream_t st = ctx->stream;
    pair_table cost;
    vga_dbuf<uint16_t> d_table2;
    vga_dbuf<uint32_t> d_b, d_e;
    vga_dbuf<uint8_t> d_def;
    uint16_t h2[256];
    int rc = cost.alloc(ctx, n_paths, 1, 1);
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, cost.clear(st));
    vga_timers_reset(ctx);
    if (n_reads) {
        VGA_HIP_CHECK_OOM(ctx, d_def.reserve(cells));
        rc = gl_table_upload(ctx, lambda, cap, h2, d_table2);
        if (rc == VGA_OK) rc = pair_upload(ctx, cells, bases, edges, d_b, d_e);
        if (rc != VGA_OK) { (void)hipStreamSynchronize(st); return rc; }  // (h2 is on its way)
        gl_launch(ctx, (uint32_t)n_reads, n_paths, lambda, cap, d_b.p, d_e.p, d_def.p, d_table2.p, cost.d.p);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess && deficit_out) e = hipMemcpyAsync(deficit_out, d_def.p, cells, hipMemcpyDeviceToHost, st);
        if (e != hipSuccess) (void)hipStreamSynchronize(st);
        VGA_HIP_CHECK(ctx, e);
    }
    if ((rc = cost.read(ctx, &cost_out, n_scored)) != VGA_OK) return rc;
    vga_timers_collect(ctx);
    return VGA_OK;
}

extern "C" int vga_genotype_lik_pairs(vga_ctx *ctx, uint64_t n_reads, uint32_t n_paths, const uint32_t *bases, const uint32_t *edges, uint32_t lambda,
                                      uint32_t cap, uint8_t *deficit_out, uint64_t *cost_out, uint64_t *n_scored)
{
    if (!ctx) return VGA_ERR_ARG;
    if (n_paths == 0 || n_paths > GL_MAX_PATHS)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_pairs: %u paths, 1 to %u are paired", n_paths, GL_MAX_PATHS);
    if (!gl_params_ok(lambda, cap))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_pairs: lambda %u, cap %u: lambda is 1 to %u and cap 1 to %u", lambda, cap, GL_MAX_LAMBDA, GL_MAX_CAP);
    if (n_reads && (!bases || !edges)) return vga_set_error(ctx, VGA_ERR_ARG, "vga_genotype_lik_pairs: null matrix");
    if (n_reads > GL_MAX_CALL_READS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_genotype_lik_pairs: too many reads");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    return gl_pairs(ctx, n_reads, n_paths, bases, edges, lambda, cap, deficit_out, cost_out, n_scored);
}
