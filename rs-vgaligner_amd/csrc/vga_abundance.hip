// vga_abundance.hip -- the path abundance: the store of deficit rows (k_ab_keep), the counts of an estimate (k_ab_count), the two
// steps of an iteration (k_ab_estep, k_ab_mstep) and the C entry points vga_path_abundance_begin / _reset / _end / _store,
// vga_path_abundance, vga_path_abundance_rows and vga_path_abundance_table.  See vga_abundance.hpp for the definition.
//
// The quotient.  resp = floor(N / z) with N = term << 16 <= 2^56 and 1 <= z <= 2^40 is taken with one 64-bit reciprocal per row,
// R = floor((2^64 - 1) / z) (the one generic division of a row, per lane), and per path q = mulhi64(N, R) with one correction.
// 2^64 / z - 1 <= R <= 2^64 / z, so N / z - N / 2^64 <= N R / 2^64 <= N / z; N / 2^64 <= 2^-8 < 1, so q is floor(N / z) or one
// below, and "q + 1 if N - q z >= z" is exact.  Integers throughout: no float enters the result.
//
// Overflow.  A lane adds at most 2^16 per row into a 32-bit partial sum and a workgroup takes at most AB_GROUP_ROWS
// AB_MAX_ROW_FACTOR rows (vga_ab_group_rows), which ends at its only flush: the partial sums of its lanes are combined in 64 bits
// through LDS and leave as one 64-bit atomic add per path.
#include "vga_abundance.hpp"
#include "vga_hap_paths.hpp"
#include "vga_path_edit.hpp"
#include "vga_path_support.hpp"

#include <algorithm>

static_assert(65536ull * AB_GROUP_ROWS * AB_MAX_ROW_FACTOR < (1ull << 32), "a workgroup's rows fit the 32-bit partial sums of k_ab_estep");
static_assert(AB_THREADS % 64u == 0 && AB_CHUNK_PATHS == 4u * AB_THREADS, "a thread of k_ab_estep owns four paths of the chunk at the end");
static_assert(AB_MAX_PATHS == PS_MAX_PATHS && AB_MAX_PATHS % AB_CHUNK_PATHS == 0, "the paths of path support, in whole chunks");
static_assert(AB_CAP_MAX == HP_CAP_MAX, "a deficit is a byte");

namespace {

constexpr uint32_t AB_WAVES = AB_THREADS / 64u;
// the rows of a workgroup of k_ab_count
constexpr uint32_t AB_COUNT_ROWS = 128u;

// the record the host reads between blocks of iterations
struct ab_dev_state {
    uint32_t done, converged, iterations, diff;
};

// One wave per winner (hp_keep_row, vga_hap_paths.hpp); the caller passes the store from the rows kept before on.
__global__ __launch_bounds__(64) void k_ab_keep(uint32_t n, uint32_t n_paths, uint32_t pitch, uint32_t cap, const uint32_t *__restrict__ rows,
                                                 const uint32_t *__restrict__ bases, const uint32_t *__restrict__ edges, uint8_t *__restrict__ deficits,
                                                 uint8_t *__restrict__ scored)
{
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    hp_keep_row(i, lane, n_paths, pitch, cap, rows, bases, edges, deficits, scored);
}

// Once per estimate.  Thread t of workgroup (x, y) owns path 256 y + t over the AB_COUNT_ROWS rows from AB_COUNT_ROWS x on: best[p]
// counts the scored rows with d = 0 on p; the workgroups of y = 0 count the scored rows as well.
__global__ __launch_bounds__(AB_THREADS) void k_ab_count(uint32_t n_rows, uint32_t n_paths, uint32_t pitch, const uint8_t *__restrict__ deficits,
                                                          const uint8_t *__restrict__ scored, unsigned long long *__restrict__ best,
                                                          unsigned long long *__restrict__ n_scored)
{
    const uint32_t tid = threadIdx.x, p = blockIdx.y * AB_THREADS + tid;
    const uint32_t r0 = blockIdx.x * AB_COUNT_ROWS, r1 = min(n_rows, r0 + AB_COUNT_ROWS);
    uint32_t c = 0;
    if (p < n_paths)
        for (uint32_t r = r0; r < r1; r++) c += scored[r] != 0 && deficits[(size_t)r * pitch + p] == 0 ? 1u : 0u;
    if (c) atomicAdd(best + p, (unsigned long long)c);
    if (blockIdx.y == 0) {
        uint32_t s = 0;
        for (uint32_t r = r0 + tid; r < r1; r += AB_THREADS) s += scored[r] != 0 ? 1u : 0u;
        if (s) atomicAdd(n_scored, (unsigned long long)s);
    }
}

// floor(N / z) from R = floor((2^64 - 1) / z): see the head of the file
__device__ __forceinline__ uint32_t ab_quot(unsigned long long N, unsigned long long z, unsigned long long R)
{
    unsigned long long q = __umul64hi(N, R);
    if (N - q * z >= z) q++;
    return (uint32_t)q;
}

// One E-step.  Workgroup (x, y) takes the rows [x group_rows, (x + 1) group_rows) and the paths of chunk y.
//   n_paths <= 64 (one chunk): a row is served by G lanes (vga_ab_row_lanes), lane l of them owns path l; a wave takes 64 / G rows
//     at a time and the waves deal them round.  z is reduced with 64-bit __shfl_xor inside the G lanes.
//   n_paths > 64: a wave takes a row; its lanes stride over the 32-bit words of the row (four paths each) for z, all paths, then
//     take the words 64 k + lane, k = 0 .. 3, of the chunk for resp: sixteen 32-bit partial sums per lane.  theta sits in LDS,
//     zero behind the last path, so the padding of a row adds nothing.
// An unscored row is skipped (a row is wave-uniform there; under the lane groups its lanes add nothing).  At the end the partial
// sums are combined through LDS and thread t adds the sums of the paths it owns to S with 64-bit atomics.
__global__ __launch_bounds__(AB_THREADS) void k_ab_estep(uint32_t n_rows, uint32_t group_rows, uint32_t n_paths, uint32_t pitch, uint32_t G,
                                                          const uint8_t *__restrict__ deficits, const uint8_t *__restrict__ scored,
                                                          const uint32_t *__restrict__ theta, const uint32_t *__restrict__ W, unsigned long long *__restrict__ S,
                                                          const ab_dev_state *__restrict__ state)
{
    __shared__ uint32_t s_w[256];
    __shared__ __attribute__((aligned(16))) uint32_t s_theta[AB_MAX_PATHS];
    __shared__ __attribute__((aligned(16))) uint32_t part[AB_WAVES][AB_CHUNK_PATHS];
    if (state->done) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t r_begin = blockIdx.x * group_rows, r_end = min(n_rows, r_begin + group_rows);
    s_w[tid] = W[tid];
    if (n_paths <= 64u) {
        const uint32_t per = 64u / G, g = lane / G, l = lane & (G - 1u);
        const bool mine = l < n_paths;
        const uint32_t th = mine ? theta[l] : 0u;
        __syncthreads();
        uint32_t acc = 0;
        for (uint32_t base = r_begin + wave * per; base < r_end; base += AB_WAVES * per) {
            const uint32_t r = base + g;
            const bool live = r < r_end;
            const uint32_t rr = live ? r : r_end - 1u;  // (a lane group behind the last row takes that row and adds nothing)
            const bool use = live && scored[rr] != 0;
            const uint32_t d = mine ? deficits[(size_t)rr * pitch + l] : 0u;
            const unsigned long long term = (unsigned long long)th * s_w[d];
            unsigned long long z = term;
            for (uint32_t off = G >> 1; off; off >>= 1) z += __shfl_xor(z, (int)off);
            if (use && z) acc += ab_quot(term << AB_RESP_BITS, z, ~0ull / z);
        }
        part[wave][lane] = acc;
        __syncthreads();
        if (tid < G && tid < n_paths) {
            unsigned long long sum = 0;
            for (uint32_t w = 0; w < AB_WAVES; w++)
                for (uint32_t k = 0; k < per; k++) sum += part[w][k * G + tid];
            if (sum) atomicAdd(S + tid, sum);
        }
        return;
    }
    for (uint32_t p = tid; p < pitch; p += AB_THREADS) s_theta[p] = p < n_paths ? theta[p] : 0u;
    __syncthreads();
    const uint32_t n_words = pitch >> 2, w0 = blockIdx.y * (AB_CHUNK_PATHS / 4u);
    uint32_t acc[4][4];
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
        for (uint32_t j = 0; j < 4u; j++) acc[k][j] = 0;
    for (uint32_t r = r_begin + wave; r < r_end; r += AB_WAVES) {
        if (!scored[r]) continue;
        const uint32_t *row = reinterpret_cast<const uint32_t *>(deficits + (size_t)r * pitch);
        unsigned long long z = 0;
        for (uint32_t w = lane; w < n_words; w += 64u) {
            const uint32_t word = row[w];
            const uint4 t = *reinterpret_cast<const uint4 *>(&s_theta[4u * w]);
            z += (unsigned long long)t.x * s_w[word & 0xFFu] + (unsigned long long)t.y * s_w[(word >> 8) & 0xFFu] +
                 (unsigned long long)t.z * s_w[(word >> 16) & 0xFFu] + (unsigned long long)t.w * s_w[word >> 24];
        }
#pragma unroll
        for (int off = 32; off; off >>= 1) z += __shfl_xor(z, off);
        if (!z) continue;
        const unsigned long long R = ~0ull / z;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            const uint32_t w = w0 + k * 64u + lane;
            if (w >= n_words) continue;
            const uint32_t word = row[w];
            const uint4 t = *reinterpret_cast<const uint4 *>(&s_theta[4u * w]);
            acc[k][0] += ab_quot(((unsigned long long)t.x * s_w[word & 0xFFu]) << AB_RESP_BITS, z, R);
            acc[k][1] += ab_quot(((unsigned long long)t.y * s_w[(word >> 8) & 0xFFu]) << AB_RESP_BITS, z, R);
            acc[k][2] += ab_quot(((unsigned long long)t.z * s_w[(word >> 16) & 0xFFu]) << AB_RESP_BITS, z, R);
            acc[k][3] += ab_quot(((unsigned long long)t.w * s_w[word >> 24]) << AB_RESP_BITS, z, R);
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) *reinterpret_cast<uint4 *>(&part[wave][4u * (k * 64u + lane)]) = make_uint4(acc[k][0], acc[k][1], acc[k][2], acc[k][3]);
    __syncthreads();
    unsigned long long sum[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t w = 0; w < AB_WAVES; w++) {
        const uint4 v = *reinterpret_cast<const uint4 *>(&part[w][4u * tid]);
        sum[0] += v.x; sum[1] += v.y; sum[2] += v.z; sum[3] += v.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < 4u; j++) {
        const uint32_t p = blockIdx.y * AB_CHUNK_PATHS + 4u * tid + j;
        if (p < n_paths && sum[j]) atomicAdd(S + p, sum[j]);
    }
}

// One M-step, one workgroup: total, theta', diff; S goes to reads_q16 and is zeroed; the iteration is counted and done / converged
// set.  Every thread reads `done` before thread 0 writes it (the barriers lie between).
__global__ __launch_bounds__(AB_THREADS) void k_ab_mstep(uint32_t n_paths, uint32_t iters, uint32_t tol, uint32_t *__restrict__ theta,
                                                          unsigned long long *__restrict__ S, unsigned long long *__restrict__ reads_q16,
                                                          ab_dev_state *__restrict__ state)
{
    __shared__ unsigned long long s_sum[AB_WAVES];
    __shared__ uint32_t s_max[AB_WAVES];
    if (state->done) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long mine = 0;
    for (uint32_t p = tid; p < n_paths; p += AB_THREADS) mine += S[p];
#pragma unroll
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if (lane == 0) s_sum[wave] = mine;
    __syncthreads();
    unsigned long long total = 0;
#pragma unroll
    for (uint32_t w = 0; w < AB_WAVES; w++) total += s_sum[w];
    uint32_t dmax = 0;
    for (uint32_t p = tid; p < n_paths; p += AB_THREADS) {
        const unsigned long long s = S[p];
        const uint32_t old = theta[p];
        const uint32_t t = total ? (uint32_t)((s << AB_THETA_BITS) / total) : old;
        dmax = max(dmax, t > old ? t - old : old - t);
        theta[p] = t;
        reads_q16[p] = s;
        S[p] = 0;
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) dmax = max(dmax, (uint32_t)__shfl_xor((int)dmax, off));
    if (lane == 0) s_max[wave] = dmax;
    __syncthreads();
    if (tid == 0) {
        uint32_t diff = 0;
#pragma unroll
        for (uint32_t w = 0; w < AB_WAVES; w++) diff = max(diff, s_max[w]);
        const uint32_t it = state->iterations + 1u;
        state->iterations = it;
        state->diff = diff;
        if (diff <= tol) {
            state->converged = 1u;
            state->done = 1u;
        } else if (it >= iters)
            state->done = 1u;
    }
}

struct ab_result {
    uint32_t *theta;
    uint64_t *reads_q16, *best, *n_scored;
    uint32_t *iterations, *converged;
};

void ab_result_zero(const ab_result &out, uint32_t n_paths)
{
    if (out.theta) memset(out.theta, 0, (size_t)n_paths * 4);
    if (out.reads_q16) memset(out.reads_q16, 0, (size_t)n_paths * 8);
    if (out.best) memset(out.best, 0, (size_t)n_paths * 8);
    if (out.n_scored) *out.n_scored = 0;
    if (out.iterations) *out.iterations = 0;
    if (out.converged) *out.converged = 0;
}

// The estimate over n_rows rows of the device store (pitch: whole words, zero behind the last path).  The iterations are enqueued
// AB_BLOCK_ITERS at a time and the state record read between the blocks: a kernel that finds `done` set returns at once, so the
// result does not depend on the block size.  The launches of the first block are timed (vga_last_kernel_times), the rest are not:
// two events per launch would be 400 000 events at the most iterations.
int ab_estimate(vga_ctx *ctx, const char *who, uint64_t n_rows, uint32_t n_paths, uint32_t pitch, const uint8_t *d_deficits, const uint8_t *d_scored,
                uint32_t lambda, uint32_t iters, uint32_t tol, const ab_result &out)
{
    ab_result_zero(out, n_paths);
    vga_timers_reset(ctx);
    if (n_rows == 0) return VGA_OK;
    if (n_rows >= (1ull << 32)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu rows", who, (unsigned long long)n_rows);
    hipStream_t st = ctx->stream;
    const size_t np = n_paths;
    // theta | W, and S | reads_q16 | best | n_scored, and the state
    vga_dbuf<uint32_t> d_u32;
    vga_dbuf<unsigned long long> d_u64;
    vga_dbuf<ab_dev_state> d_state;
    VGA_HIP_CHECK_OOM(ctx, d_u32.reserve(np + 256));
    VGA_HIP_CHECK_OOM(ctx, d_u64.reserve(3 * np + 1));
    VGA_HIP_CHECK_OOM(ctx, d_state.reserve(1));
    uint32_t *d_theta = d_u32.p, *d_W = d_u32.p + np;
    unsigned long long *d_S = d_u64.p, *d_reads = d_u64.p + np, *d_best = d_u64.p + 2 * np, *d_n = d_u64.p + 3 * np;
    std::vector<uint32_t> h(np + 256, (1u << AB_THETA_BITS) / n_paths);
    vga_ab_table(lambda, AB_CAP_MAX, h.data() + np);
    hipError_t e = hipMemcpyAsync(d_u32.p, h.data(), h.size() * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_u64.p, 0, (3 * np + 1) * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_state.p, 0, sizeof(ab_dev_state), st);
    if (e != hipSuccess) (void)hipStreamSynchronize(st);  // (h is on its way)
    VGA_HIP_CHECK(ctx, e);
    int rc = vga_launch(ctx, "k_ab_count", n_rows * ((uint64_t)pitch + 1u), k_ab_count, dim3((unsigned)((n_rows + AB_COUNT_ROWS - 1u) / AB_COUNT_ROWS), (n_paths + AB_THREADS - 1u) / AB_THREADS),
                        dim3(AB_THREADS), n_rows, n_paths, pitch, d_deficits, d_scored, d_best, d_n);
    unsigned long long n = 0;
    if (rc == VGA_OK && hipMemcpyAsync(&n, d_n, sizeof n, hipMemcpyDeviceToHost, st) != hipSuccess) rc = vga_set_error(ctx, VGA_ERR_HIP, "%s: reading the count", who);
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (rc != VGA_OK) return rc;
    if (n >= AB_MAX_ROWS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu scored rows, fewer than %llu are estimated from", who, n, (unsigned long long)AB_MAX_ROWS);
    if (n == 0) {  // no call
        vga_timers_collect(ctx);
        return VGA_OK;
    }
    const uint32_t group_rows = vga_ab_group_rows(n_rows), G = vga_ab_row_lanes(n_paths);
    const dim3 grid((unsigned)((n_rows + group_rows - 1u) / group_rows), (n_paths + AB_CHUNK_PATHS - 1u) / AB_CHUNK_PATHS);
    const uint64_t e_bytes = n_rows * ((uint64_t)pitch * (grid.y + 1u) + 1u);
    ab_dev_state state = {0, 0, 0, 0};
    for (uint32_t sent = 0; sent < iters && !state.done;) {
        const uint32_t block = std::min(AB_BLOCK_ITERS, iters - sent);
        for (uint32_t i = 0; i < block; i++) {
            if (sent == 0) {
                rc = vga_launch(ctx, "k_ab_estep", e_bytes, k_ab_estep, grid, dim3(AB_THREADS), n_rows, group_rows, n_paths, pitch, G, d_deficits, d_scored, d_theta, d_W,
                                d_S, d_state.p);
                if (rc == VGA_OK) rc = vga_launch(ctx, "k_ab_mstep", np * 28u, k_ab_mstep, dim3(1), dim3(AB_THREADS), n_paths, iters, tol, d_theta, d_S, d_reads, d_state.p);
                if (rc != VGA_OK) { (void)hipStreamSynchronize(st); return rc; }
            } else {
                hipLaunchKernelGGL(k_ab_estep, grid, dim3(AB_THREADS), 0, st, (uint32_t)n_rows, group_rows, n_paths, pitch, G, d_deficits, d_scored, d_theta, d_W, d_S,
                                   d_state.p);
                hipLaunchKernelGGL(k_ab_mstep, dim3(1), dim3(AB_THREADS), 0, st, n_paths, iters, tol, d_theta, d_S, d_reads, d_state.p);
            }
        }
        sent += block;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&state, d_state.p, sizeof state, hipMemcpyDeviceToHost, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        VGA_HIP_CHECK(ctx, e);
        VGA_HIP_CHECK(ctx, e2);
    }
    e = hipSuccess;
    if (out.theta) e = hipMemcpyAsync(out.theta, d_theta, np * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out.reads_q16) e = hipMemcpyAsync(out.reads_q16, d_reads, np * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && out.best) e = hipMemcpyAsync(out.best, d_best, np * 8, hipMemcpyDeviceToHost, st);
    const hipError_t e2 = hipStreamSynchronize(st);
    VGA_HIP_CHECK(ctx, e);
    VGA_HIP_CHECK(ctx, e2);
    if (out.n_scored) *out.n_scored = n;
    if (out.iterations) *out.iterations = state.iterations;
    if (out.converged) *out.converged = state.converged;
    vga_timers_collect(ctx);
    return VGA_OK;
}

}  // namespace

// The store of a context while it is on: a child of path support (ps_state::ab), released with it and with the index.
struct ab_state {
    uint32_t n_paths = 0, pitch = 0, cap = AB_CAP_DEFAULT, source = AB_FROM_SUPPORT;
    uint8_t *d_deficits = nullptr, *d_scored = nullptr;
    uint64_t cap_rows = 0, n_rows = 0, first_rows = AB_STORE_ROWS0;
    ~ab_state()
    {
        if (d_deficits) (void)hipFree(d_deficits);
        if (d_scored) (void)hipFree(d_scored);
    }
};

ab_state *ab_active(vga_ctx *ctx)
{
    ps_state *ps = ps_active(ctx);
    return ps ? ps->ab.get() : nullptr;
}

bool ab_from_edit(const ab_state *ab) { return ab->source == AB_FROM_EDIT; }

int ab_keep_winners(vga_ctx *ctx, ab_state *ab, ps_state *ps, const uint32_t *d_rows, size_t nw)
{
    if (nw == 0) return VGA_OK;
    if (ab_from_edit(ab) && !ps->pe)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_align_batch: the path abundance reads the edit distance (vga_path_abundance_begin), which is off (vga_path_edit_begin)");
    const uint64_t at = ab->n_rows + nw;
    int rc = hp_store_grow(ctx, "path abundance", ab->d_deficits, ab->d_scored, ab->cap_rows, ab->n_rows, ab->first_rows, ab->pitch, at);
    if (rc != VGA_OK) return rc;
    const bool edit = ab_from_edit(ab);
    const uint32_t *d_bases = edit ? pe_gl_bases(ps->pe.get()) : ps->d_bases.p, *d_edges = edit ? pe_gl_edges(ps->pe.get()) : ps->d_edges.p;
    rc = vga_launch(ctx, "k_ab_keep", nw * ((uint64_t)ab->n_paths * 8u + ab->pitch), k_ab_keep, dim3((unsigned)nw), dim3(64), nw, ab->n_paths, ab->pitch, ab->cap, d_rows,
                    d_bases, d_edges, ab->d_deficits + ab->n_rows * ab->pitch, ab->d_scored + ab->n_rows);
    if (rc != VGA_OK) return rc;
    ab->n_rows = at;
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_path_abundance_table(uint32_t lambda, uint32_t cap, uint32_t *out)
{
    if (lambda < 1u || lambda > AB_LAMBDA_MAX || cap < 1u || cap > AB_CAP_MAX || !out) return VGA_ERR_ARG;
    vga_ab_table(lambda, cap, out);
    return VGA_OK;
}

extern "C" int vga_path_abundance_begin(vga_ctx *ctx, uint32_t cap, uint32_t source)
{
    if (!ctx) return VGA_ERR_ARG;
    if (cap < 1u || cap > AB_CAP_MAX) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_begin: cap %u (1 .. %u)", cap, AB_CAP_MAX);
    if (source != AB_FROM_SUPPORT && source != AB_FROM_EDIT) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_begin: source %u (0 support, 1 edit)", source);
    if (source == AB_FROM_EDIT && !pe_active(ctx))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_begin: the edit distance is off (vga_path_edit_begin), which source edit reads");
    return ps_child_begin(ctx, "vga_path_abundance_begin", &ps_state::ab, [&](ps_state *ps, ab_state *ab) {
        ab->n_paths = ps->n_paths;
        ab->pitch = hp_pitch(ps->n_paths);
        ab->cap = cap;
        ab->source = source;
        if (const char *e = getenv("VGA_PATH_ABUNDANCE_STORE_ROWS")) ab->first_rows = (uint64_t)std::max(1ll, atoll(e));
        return VGA_OK;
    });
}

extern "C" int vga_path_abundance_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ab_state *ab = ab_active(ctx);
    return ps_child_reset(ctx, ab != nullptr, "vga_path_abundance_reset: the store is off (vga_path_abundance_begin)", [&]() {
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ab->n_rows = 0;
        return VGA_OK;
    });
}

extern "C" int vga_path_abundance_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_end(ctx, &ps_state::ab);
}

extern "C" int vga_path_abundance_store(vga_ctx *ctx, uint64_t cap_rows, uint8_t *deficits, uint8_t *scored, uint64_t *n_rows)
{
    if (!ctx) return VGA_ERR_ARG;
    ab_state *ab = ab_active(ctx);
    if (!ab) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_store: the store is off (vga_path_abundance_begin)");
    if (n_rows) *n_rows = ab->n_rows;
    if (cap_rows < ab->n_rows || ab->n_rows == 0) return VGA_OK;
    (void)hipSetDevice(ctx->device);
    if (deficits) VGA_HIP_CHECK(ctx, hipMemcpy2DAsync(deficits, ab->n_paths, ab->d_deficits, ab->pitch, ab->n_paths, ab->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (scored) VGA_HIP_CHECK(ctx, hipMemcpyAsync(scored, ab->d_scored, ab->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

extern "C" int vga_path_abundance(vga_ctx *ctx, uint32_t lambda, uint32_t iters, uint32_t tol, uint32_t *theta, uint64_t *reads_q16, uint64_t *best,
                                  uint64_t *n_scored, uint32_t *iterations, uint32_t *converged)
{
    if (!ctx) return VGA_ERR_ARG;
    vga_timers_reset(ctx);  // (a refusal reports no kernel)
    ab_state *ab = ab_active(ctx);
    if (!ab) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance: the store is off (vga_path_abundance_begin)");
    if (!vga_ab_params_ok(lambda, iters, tol))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance: lambda %u, iters %u, tol %u: lambda is 1 to %u, iters 1 to %u and tol 0 to %u", lambda, iters, tol,
                             AB_LAMBDA_MAX, AB_ITERS_MAX, AB_TOL_MAX);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    const ab_result out = {theta, reads_q16, best, n_scored, iterations, converged};
    try {
        return ab_estimate(ctx, "vga_path_abundance", ab->n_rows, ab->n_paths, ab->pitch, ab->d_deficits, ab->d_scored, lambda, iters, tol, out);
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_abundance: out of host memory");
    }
}

static int ab_rows(vga_ctx *ctx, uint64_t n_rows, uint32_t n_paths, const uint8_t *deficits, const uint8_t *scored, uint32_t lambda, uint32_t iters, uint32_t tol,
                   const ab_result &out)
{
    const uint32_t pitch = hp_pitch(n_paths);
    vga_dbuf<uint8_t> d_def, d_sc;
    std::vector<uint8_t> pitched;  // the rows at the store's pitch, zero behind the last path: one copy, whatever the width of a row
    if (n_rows) {
        hipStream_t st = ctx->stream;
        VGA_HIP_CHECK_OOM(ctx, d_def.reserve((size_t)n_rows * pitch));
        VGA_HIP_CHECK_OOM(ctx, d_sc.reserve(n_rows));
        if (pitch != n_paths) {
            pitched.assign((size_t)n_rows * pitch, 0);
            for (uint64_t r = 0; r < n_rows; r++) memcpy(pitched.data() + r * pitch, deficits + r * n_paths, n_paths);
        }
        hipError_t e = hipMemcpyAsync(d_def.p, pitch != n_paths ? pitched.data() : deficits, (size_t)n_rows * pitch, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_sc.p, scored, n_rows, hipMemcpyHostToDevice, st);
        const hipError_t e2 = hipStreamSynchronize(st);
        VGA_HIP_CHECK(ctx, e);
        VGA_HIP_CHECK(ctx, e2);
    }
    return ab_estimate(ctx, "vga_path_abundance_rows", n_rows, n_paths, pitch, d_def.p, d_sc.p, lambda, iters, tol, out);
}

extern "C" int vga_path_abundance_rows(vga_ctx *ctx, uint64_t n_rows, uint32_t n_paths, const uint8_t *deficits, const uint8_t *scored, uint32_t lambda,
                                       uint32_t iters, uint32_t tol, uint32_t *theta, uint64_t *reads_q16, uint64_t *best, uint64_t *n_scored, uint32_t *iterations,
                                       uint32_t *converged)
{
    if (!ctx) return VGA_ERR_ARG;
    vga_timers_reset(ctx);  // (a refusal reports no kernel)
    if (n_paths == 0 || n_paths > AB_MAX_PATHS) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_rows: %u paths, 1 to %u are estimated", n_paths, AB_MAX_PATHS);
    if (!vga_ab_params_ok(lambda, iters, tol))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_rows: lambda %u, iters %u, tol %u: lambda is 1 to %u, iters 1 to %u and tol 0 to %u", lambda, iters, tol,
                             AB_LAMBDA_MAX, AB_ITERS_MAX, AB_TOL_MAX);
    if (n_rows && (!deficits || !scored)) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_rows: null array");
    if (n_rows >= (1ull << 32)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_abundance_rows: %llu rows", (unsigned long long)n_rows);
    for (uint64_t r = 0; r < n_rows; r++)
        if (scored[r] > 1u) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_abundance_rows: scored[%llu] is %u, a byte of 0 or 1", (unsigned long long)r, scored[r]);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    const ab_result out = {theta, reads_q16, best, n_scored, iterations, converged};
    try {
        return ab_rows(ctx, n_rows, n_paths, deficits, scored, lambda, iters, tol, out);
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_abundance_rows: out of host memory");
    }
}
