// vga_path_support.hip -- reads x paths support: k_ps_build, k_ps_score and the six C entry points vga_path_support_begin /
// _read / _last / _reset / _end / _lists.  See vga_path_support.hpp for the shape and the lane mapping.
//
// Meaning (include/vga_hip.h): bases[r][p] is the number of graph bases under M operations of alignment r that lie in a node
// path p visits forward, edges[r][p] the number of consecutive node pairs of r's path that p steps over forward to forward.  All
// values are integers; sums and ORs do not depend on order, so the tables are exact and repeatable.
#include "vga_path_support.hpp"
#include "vga_genotype.hpp"
#include "vga_genotype_lik.hpp"
#include "vga_path_edit.hpp"
#include "vga_hap_paths.hpp"
#include "vga_abundance.hpp"
#include "vga_phase.hpp"

#include <algorithm>

namespace {

// One thread per path step.  Bit p of node_paths[id - 1] for a forward step; for a forward step followed by a forward step, bit
// p of the slot of the second node in the outgoing part of the first's edge slice (coverage's slot rule).  A pair without such a
// slot (no L line) sets nothing and is counted.
__global__ __launch_bounds__(256) void k_ps_build(uint32_t n_paths, const unsigned long long *__restrict__ step_off, const uint32_t *__restrict__ steps,
                                                   const uint32_t *__restrict__ edge_idx, const uint32_t *__restrict__ edges_to,
                                                   const uint32_t *__restrict__ edges, uint32_t PW, uint32_t *__restrict__ node_paths,
                                                   uint32_t *__restrict__ edge_paths, unsigned long long *__restrict__ n_missing)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t < step_off[0] || t >= step_off[n_paths]) return;
    uint32_t lo = 0, hi = n_paths;  // the last path whose first step is at or before t
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (step_off[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t p = lo, word = p >> 5, bit = 1u << (p & 31u);
    const uint32_t h = steps[t];
    if (h & 1u) return;
    const uint32_t a = h >> 1;
    atomicOr(node_paths + (size_t)(a - 1) * PW + word, bit);
    if (t + 1 >= step_off[p + 1]) return;
    const uint32_t want = steps[t + 1];
    if (want & 1u) return;
    const uint32_t e1 = edge_idx[a];
    for (uint32_t s = edge_idx[a - 1] + edges_to[a - 1]; s < e1; s++)
        if (edges[s] == want) { atomicOr(edge_paths + (size_t)s * PW + word, bit); return; }
    atomicAdd(n_missing, 1ull);
}

// The wave hands its (up to 64) items round: lane j's item is row `item` of a bitset table (0xFFFFFFFF: none) with value `val`;
// lane l of path block q adds val to acc[64 q + l] when bit 64 q + l of the row is set.  acc is the wave's LDS: a lane touches
// only its own words.
__device__ __forceinline__ void ps_hand_round(uint32_t item, uint32_t val, const uint32_t *__restrict__ tab, uint32_t PW, uint32_t n_blocks,
                                              uint32_t *acc, int lane)
{
    const bool have = item != 0xFFFFFFFFu && val != 0u;
    const uint64_t mask = __builtin_amdgcn_ballot_w64(have);
    if (!mask) return;
    const uint32_t *row = tab + (size_t)(have ? item : 0u) * PW;
    for (uint32_t q = 0; q < n_blocks; q++) {
        uint32_t w0 = 0, w1 = 0;
        if (have) {
            w0 = row[2 * q];
            if (2 * q + 1 < PW) w1 = row[2 * q + 1];
        }
        uint32_t a = acc[q * 64 + lane];
        uint64_t m = mask;
        while (m) {
            const int j = __builtin_ctzll(m);
            m &= m - 1;
            const uint32_t x0 = (uint32_t)__builtin_amdgcn_readlane((int)w0, j), x1 = (uint32_t)__builtin_amdgcn_readlane((int)w1, j);
            const uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)val, j);
            const uint32_t x = lane < 32 ? x0 : x1;
            a += ((x >> (lane & 31)) & 1u) ? v : 0u;
        }
        acc[q * 64 + lane] = a;
    }
}

// One wave per reported alignment (or per list of the seam), paths across the lanes (vga_path_support.hpp).
//   bases: the runs of the list, two events each (start << 1, end << 1 | 1), are cut at the node starts; a lane takes a run,
//          finds the node of its first base (binary search over node_start) and gives one piece per round;
//   edges: a lane takes a consecutive pair of the node list and scans the outgoing slice of the first for the second.
// Then the maximum key (bases, edges) over the paths, the row of the two matrices, and -- with accumulators -- the four
// per-path sums and the two scalars (acc: sum_bases, sum_edges, top, top_alone of n_paths words each, n_alignments, n_unplaced).
__global__ __launch_bounds__(64) void k_ps_score(uint32_t n, const cov_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                  const uint32_t *__restrict__ host_lists, const uint32_t *__restrict__ row_of,
                                                  const uint32_t *__restrict__ node_start, const uint32_t *__restrict__ edge_idx,
                                                  const uint32_t *__restrict__ edges_to, const uint32_t *__restrict__ edges, uint32_t n_graph_nodes,
                                                  uint32_t seq_length, uint32_t n_paths, uint32_t PW, const uint32_t *__restrict__ node_paths,
                                                  const uint32_t *__restrict__ edge_paths, uint32_t *__restrict__ bases_out,
                                                  uint32_t *__restrict__ edges_out, unsigned long long *__restrict__ acc)
{
    __shared__ uint32_t s_b[PS_MAX_PATHS], s_e[PS_MAX_PATHS];
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const int lane = threadIdx.x;
    const uint32_t n_blocks = (n_paths + 63u) >> 6;
    for (uint32_t q = 0; q < n_blocks; q++) { s_b[q * 64 + lane] = 0u; s_e[q * 64 + lane] = 0u; }
    const cov_rec rc = recs[wi];
    const uint32_t *nodes = (rc.flags == 3u ? host_lists : lists) + rc.off;
    const uint32_t *ev = nodes + rc.n_a;
    // ---- bases
    const uint32_t n_runs = rc.n_b >> 1;
    for (uint32_t base = 0; base < n_runs; base += 64) {
        const uint32_t r = base + (uint32_t)lane;
        uint32_t cur = 0, end = 0, node = 0;  // the part of the run still to be handed out, and the (0-based) node `cur` lies in
        if (r < n_runs) {
            const uint32_t s = ev[2 * r] >> 1, e = ev[2 * r + 1] >> 1;
            if (s < e && e <= seq_length) {
                cur = s; end = e;
                uint32_t lo = 0, hi = n_graph_nodes;
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (node_start[mid] <= s) lo = mid; else hi = mid;
                }
                node = lo;
            }
        }
        while (__builtin_amdgcn_ballot_w64(cur < end)) {
            uint32_t item = 0xFFFFFFFFu, len = 0;
            if (cur < end) {
                if (node < n_graph_nodes) {
                    const uint32_t stop = min(end, node_start[node + 1]);
                    item = node; len = stop > cur ? stop - cur : 0u;
                    cur = stop > cur ? stop : cur;
                    node++;
                } else
                    cur = end;
            }
            ps_hand_round(item, len, node_paths, PW, n_blocks, s_b, lane);
        }
    }
    // ---- edges
    for (uint32_t base = 0; base + 1 < rc.n_a; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t slot = 0xFFFFFFFFu;
        if (i + 1 < rc.n_a) {
            const uint32_t a = nodes[i], b = nodes[i + 1];
            if (a >= 1u && a <= n_graph_nodes && b >= 1u && b <= n_graph_nodes) {
                const uint32_t want = b << 1, e1 = edge_idx[a];
                for (uint32_t t = edge_idx[a - 1] + edges_to[a - 1]; t < e1; t++)
                    if (edges[t] == want) { slot = t; break; }
            }
        }
        ps_hand_round(slot, 1u, edge_paths, PW, n_blocks, s_e, lane);
    }
    // ---- the maximum key, the row, the accumulators
    unsigned long long best = 0;
    for (uint32_t q = 0; q < n_blocks; q++) {
        const unsigned long long key = ((unsigned long long)s_b[q * 64 + lane] << 32) | s_e[q * 64 + lane];  // (paths past n_paths: no bit, 0)
        best = key > best ? key : best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor((long long)best, d);
        best = o > best ? o : best;
    }
    uint32_t n_top = 0;
    if (best)
        for (uint32_t q = 0; q < n_blocks; q++) {
            const unsigned long long key = ((unsigned long long)s_b[q * 64 + lane] << 32) | s_e[q * 64 + lane];
            n_top += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(key == best));
        }
    const uint32_t row = row_of ? row_of[wi] : wi;
    for (uint32_t q = 0; q < n_blocks; q++) {
        const uint32_t p = q * 64 + (uint32_t)lane;
        if (p >= n_paths) continue;
        const uint32_t b = s_b[p], e = s_e[p];
        bases_out[(size_t)row * n_paths + p] = b;
        edges_out[(size_t)row * n_paths + p] = e;
        if (!acc) continue;
        if (b) atomicAdd(acc + p, (unsigned long long)b);
        if (e) atomicAdd(acc + n_paths + p, (unsigned long long)e);
        if (best && (((unsigned long long)b << 32) | e) == best) {
            atomicAdd(acc + 2ull * n_paths + p, 1ull);
            if (n_top == 1u) atomicAdd(acc + 3ull * n_paths + p, 1ull);
        }
    }
    if (acc && lane == 0) {
        atomicAdd(acc + 4ull * n_paths, 1ull);
        if (!best) atomicAdd(acc + 4ull * n_paths + 1, 1ull);
    }
}

}  // namespace

ps_state *ps_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? ctx->index.ps.get() : nullptr; }

int ps_acc_block::zero(vga_ctx *ctx)
{
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d.p, 0, words() * sizeof(unsigned long long), ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

int ps_acc_block::read(vga_ctx *ctx, uint64_t *const col[4], uint64_t *s0, uint64_t *s1)
{
    const size_t np = n_paths;
    std::vector<unsigned long long> h(words());
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(h.data(), d.p, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++)
        if (col[k])
            for (size_t p = 0; p < np; p++) col[k][p] = h[k * np + p];
    if (s0) *s0 = h[4 * np];
    if (s1) *s1 = h[4 * np + 1];
    return VGA_OK;
}

int ps_read_last(vga_ctx *ctx, const char *who, bool have_last, uint64_t last_reads, uint64_t n_reads, uint32_t n_paths, uint32_t *const dst[2],
                 const uint32_t *const src[2])
{
    if (!have_last) return vga_set_error(ctx, VGA_ERR_ARG, "%s: no vga_align_batch has been scored on this context yet", who);
    if (n_reads != last_reads)
        return vga_set_error(ctx, VGA_ERR_ARG, "%s: the last vga_align_batch had %llu reads, not %llu", who, (unsigned long long)last_reads,
                             (unsigned long long)n_reads);
    (void)hipSetDevice(ctx->device);
    const size_t bytes = (size_t)n_reads * n_paths * 4;
    for (int k = 0; k < 2; k++)
        if (dst[k] && bytes) VGA_HIP_CHECK(ctx, hipMemcpyAsync(dst[k], src[k], bytes, hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

static void ps_launch_score(vga_ctx *ctx, const ps_state *ps, uint32_t n, const cov_win_view &v, const uint32_t *d_rows, uint32_t *d_bases,
                            uint32_t *d_edges, unsigned long long *d_acc)
{
    const vga_dev_index &ix = ctx->index;
    const int t = vga_timer_begin(ctx, "k_ps_score", 0, ctx->stream);
    hipLaunchKernelGGL(k_ps_score, dim3(n), dim3(64), 0, ctx->stream, n, v.recs, v.lists, v.host_lists, d_rows, ix.d_node_start, ix.d_edge_idx,
                       ix.d_edges_to, ix.d_edges, (uint32_t)ix.n_nodes, (uint32_t)ix.seq_length, ps->n_paths, ps->PW, ps->d_node_paths.p,
                       ps->d_edge_paths.p, d_bases, d_edges, d_acc);
    vga_timer_end(ctx, t);
}

int ps_score_winners(vga_ctx *ctx, ps_state *ps, const cov_win_view &v, const std::vector<uint32_t> &reads, uint64_t n_reads, const pe_queries *q)
{
    const size_t nw = reads.size(), cells = (size_t)n_reads * ps->n_paths;
    hipStream_t st = ctx->stream;
    ps->have_last = false;
    VGA_HIP_CHECK_OOM(ctx, ps->d_bases.reserve(cells + 1));
    VGA_HIP_CHECK_OOM(ctx, ps->d_edges.reserve(cells + 1));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ps->d_bases.p, 0, cells * 4, st));  // (a read without a reported alignment keeps a zero row)
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ps->d_edges.p, 0, cells * 4, st));
    if (nw) {
        VGA_HIP_CHECK(ctx, ps->h_rows.reserve(nw));
        VGA_HIP_CHECK_OOM(ctx, ps->d_rows.reserve(nw));
        memcpy(ps->h_rows.p, reads.data(), nw * 4);
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(ps->d_rows.p, ps->h_rows.p, nw * 4, hipMemcpyHostToDevice, st));
        ps_launch_score(ctx, ps, (uint32_t)nw, v, ps->d_rows.p, ps->d_bases.p, ps->d_edges.p, ps->acc.d.p);
        VGA_HIP_CHECK(ctx, hipGetLastError());
        const bool gl_from_edit = ps->gl && gl_source(ps->gl.get()) == VGA_GL_FROM_EDIT;
        if (gl_from_edit && !ps->pe)
            return vga_set_error(ctx, VGA_ERR_ARG, "vga_align_batch: the likelihood reads the edit distance (vga_genotype_lik_source), which is off (vga_path_edit_begin)");
        hp_state *hp = hp_active(ctx);  // the deficit store beside the phase store is on: it keeps a row per winner, from the matrices of its source
        ab_state *ab = ps->ab.get();    // ... and so does the store of the path abundance
        if (ps->pe) {  // the edit distance is on: its three kernels over the same winners, on the same stream
            if (!q) return vga_set_error(ctx, VGA_ERR_ARG, "path edit: no queries");
            const int rc = pe_add_call(ctx, ps, v, ps->d_rows.p, nw, n_reads, *q, gl_from_edit || (hp && hp_from_edit(hp)) || (ab && ab_from_edit(ab)));
            if (rc != VGA_OK) return rc;
        }
        if (ps->gt) {  // genotyping is on: the pairs of paths over the two matrices, behind k_ps_score on the same stream
            const int rc = gt_add_call(ctx, ps->gt.get(), n_reads, ps->d_bases.p, ps->d_edges.p);
            if (rc != VGA_OK) return rc;
        }
        if (ps->gl) {  // the read likelihood is on: the byte deficits of the two matrices and the cost of every pair, on the same stream
            const int rc = gl_from_edit ? gl_add_call(ctx, ps->gl.get(), n_reads, pe_gl_bases(ps->pe.get()), pe_gl_edges(ps->pe.get()))
                                        : gl_add_call(ctx, ps->gl.get(), n_reads, ps->d_bases.p, ps->d_edges.p);
            if (rc != VGA_OK) return rc;
        }
        if (hp) {  // behind k_ps_score and the edit kernels on the same stream
            const int rc = hp_keep_winners(ctx, hp, ps, ps->d_rows.p, nw);
            if (rc != VGA_OK) return rc;
        }
        if (ab) {  // likewise
            const int rc = ab_keep_winners(ctx, ab, ps, ps->d_rows.p, nw);
            if (rc != VGA_OK) return rc;
        }
    } else if (ps->pe) {  // (no winner: the call's matrix is all NONE)
        const pe_queries none = {nullptr, nullptr, nullptr};
        const int rc = pe_add_call(ctx, ps, v, nullptr, 0, n_reads, none, false);
        if (rc != VGA_OK) return rc;
    }
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    ps->last_reads = n_reads;
    ps->have_last = true;
    if (nw) vga_timers_collect(ctx);  // (poa_run collected before this launch: once more, with it)
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
static void ps_release(vga_ctx *ctx)
{
    if (ph_state *ph = ph_active(ctx)) ph_hap_paths(ph).reset();  // (the deficit store holds rows of these paths)
    ctx->index.ps.reset();
    cov_lists_release(ctx, COV_USER_PATHS);
}

static int ps_begin(vga_ctx *ctx, uint32_t n_paths, const uint64_t *step_off, const uint64_t *steps, uint64_t *n_pairs_without_edge)
{
    const vga_dev_index &ix = ctx->index;
    const uint64_t total = step_off[n_paths] - step_off[0];
    std::vector<uint32_t> h32(total + 1);
    for (uint64_t t = 0; t < total; t++) h32[t] = (uint32_t)steps[step_off[0] + t];
    std::vector<unsigned long long> off(n_paths + 1);
    for (uint32_t p = 0; p <= n_paths; p++) off[p] = step_off[p] - step_off[0];
    int rc = cov_lists_acquire(ctx, COV_USER_PATHS, "vga_path_support_begin");
    if (rc != VGA_OK) return rc;
    if (!(ctx->index.ps = vga_make_owned<ps_state>())) return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_support_begin: out of host memory");
    ps_state *ps = ctx->index.ps.get();
    ps->n_paths = n_paths;
    ps->PW = (n_paths + 31u) / 32u;
    ps->h_off = off;
    ps->h_steps.assign(h32.begin(), h32.begin() + (long)total);
    const size_t node_words = (size_t)ix.n_nodes * ps->PW, edge_words = (size_t)ix.n_edges * ps->PW;
    hipStream_t st = ctx->stream;
    vga_dbuf<uint32_t> d_steps;
    vga_dbuf<unsigned long long> d_off, d_missing;
    VGA_HIP_CHECK_OOM(ctx, ps->d_node_paths.reserve(node_words + 1));
    VGA_HIP_CHECK_OOM(ctx, ps->d_edge_paths.reserve(edge_words + 1));
    VGA_HIP_CHECK_OOM(ctx, ps->acc.reserve(n_paths));
    VGA_HIP_CHECK_OOM(ctx, d_steps.reserve(total + 1));
    VGA_HIP_CHECK_OOM(ctx, d_off.reserve(n_paths + 1));
    VGA_HIP_CHECK_OOM(ctx, d_missing.reserve(1));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ps->d_node_paths.p, 0, node_words * 4, st));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ps->d_edge_paths.p, 0, edge_words * 4, st));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_missing.p, 0, sizeof(unsigned long long), st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_steps.p, h32.data(), (total + 1) * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_off.p, off.data(), (n_paths + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    unsigned long long missing = 0;
    vga_timers_reset(ctx);
    if (total) {
        const int t = vga_timer_begin(ctx, "k_ps_build", 0, st);
        hipLaunchKernelGGL(k_ps_build, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, n_paths, d_off.p, d_steps.p, ix.d_edge_idx, ix.d_edges_to,
                           ix.d_edges, ps->PW, ps->d_node_paths.p, ps->d_edge_paths.p, d_missing.p);
        vga_timer_end(ctx, t);
        VGA_HIP_CHECK(ctx, hipGetLastError());
    }
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(&missing, d_missing.p, sizeof missing, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    vga_timers_collect(ctx);
    if (n_pairs_without_edge) *n_pairs_without_edge = missing;
    return ps->acc.zero(ctx);
}

extern "C" int vga_path_support_begin(vga_ctx *ctx, uint32_t n_paths, const uint64_t *step_off, const uint64_t *steps, uint64_t *n_pairs_without_edge)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_path_support_begin: no index uploaded");
    if (n_paths == 0 || !step_off) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_begin: no paths");
    if (n_paths > PS_MAX_PATHS)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_support_begin: %u paths, at most %u are scored", n_paths, PS_MAX_PATHS);
    const vga_dev_index &ix = ctx->index;
    if (ix.seq_length >= (1ull << 31) || ix.n_nodes >= (1ull << 31) || ix.n_edges >= (1ull << 32))
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_support_begin: graph too large for 32-bit positions");
    for (uint32_t p = 0; p < n_paths; p++)
        if (step_off[p + 1] < step_off[p]) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_begin: step_off decreases at path %u", p);
    if (step_off[n_paths] > step_off[0] && !steps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_begin: no steps");
    for (uint64_t t = step_off[0]; t < step_off[n_paths]; t++)
        if ((steps[t] >> 1) < 1 || (steps[t] >> 1) > ix.n_nodes)
            return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_begin: step %llu names node %llu, the index has nodes 1..%llu", (unsigned long long)t,
                                 (unsigned long long)(steps[t] >> 1), (unsigned long long)ix.n_nodes);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ps_release(ctx);  // (a second begin starts over with the new paths)
    int rc;
    try {
        rc = ps_begin(ctx, n_paths, step_off, steps, n_pairs_without_edge);
    } catch (const std::bad_alloc &) {
        rc = vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_support_begin: out of host memory");
    }
    if (rc != VGA_OK) ps_release(ctx);
    return rc;
}

extern "C" int vga_path_support_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_reset: path support is off (vga_path_support_begin)");
    (void)hipSetDevice(ctx->device);
    return ps->acc.zero(ctx);
}

extern "C" int vga_path_support_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ps_release(ctx);
    return VGA_OK;
}

extern "C" int vga_path_support_read(vga_ctx *ctx, uint64_t *sum_bases, uint64_t *sum_edges, uint64_t *top, uint64_t *top_alone, uint64_t *n_alignments,
                                     uint64_t *n_unplaced)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_read: path support is off (vga_path_support_begin)");
    (void)hipSetDevice(ctx->device);
    uint64_t *const dst[4] = {sum_bases, sum_edges, top, top_alone};
    return ps->acc.read(ctx, dst, n_alignments, n_unplaced);
}

extern "C" int vga_path_support_last(vga_ctx *ctx, uint64_t n_reads, uint32_t *bases, uint32_t *edges)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_last: path support is off (vga_path_support_begin)");
    uint32_t *const dst[2] = {bases, edges};
    const uint32_t *const src[2] = {ps->d_bases.p, ps->d_edges.p};
    return ps_read_last(ctx, "vga_path_support_last", ps->have_last, ps->last_reads, n_reads, ps->n_paths, dst, src);
}

// The kernel seam: explicit lists through k_ps_score.  Each list becomes what k_cov_runs would have written -- its node ids, then
// one run per node with covered bases (the first node_bases[i] bases of the node) -- and is scored without accumulators.
static int ps_lists(vga_ctx *ctx, ps_state *ps, uint64_t n, const uint64_t *node_off, const uint32_t *node_ids, const uint32_t *node_bases,
                    uint32_t *bases_out, uint32_t *edges_out)
{
    const vga_dev_index &ix = ctx->index;
    std::vector<cov_rec> recs(n);
    std::vector<uint32_t> words;
    for (uint64_t i = 0; i < n; i++) {
        if (node_off[i + 1] < node_off[i]) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_lists: node_off decreases at list %llu", (unsigned long long)i);
        if (node_off[i + 1] - node_off[i] >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_support_lists: list too long");
        cov_rec rc = {(uint32_t)words.size(), (uint32_t)(node_off[i + 1] - node_off[i]), 0u, 3u};
        for (uint64_t t = node_off[i]; t < node_off[i + 1]; t++) {
            const uint32_t id = node_ids[t];
            if (id < 1 || id > ix.n_nodes)
                return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_lists: entry %llu names node %u, the index has nodes 1..%llu", (unsigned long long)t, id,
                                     (unsigned long long)ix.n_nodes);
            if (node_bases[t] > ix.node_start[id] - ix.node_start[id - 1])
                return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_lists: entry %llu covers %u bases of node %u, which has %u", (unsigned long long)t,
                                     node_bases[t], id, ix.node_start[id] - ix.node_start[id - 1]);
            words.push_back(id);
        }
        for (uint64_t t = node_off[i]; t < node_off[i + 1]; t++)
            if (node_bases[t]) {
                const uint32_t s = ix.node_start[node_ids[t] - 1];
                words.push_back(s << 1);
                words.push_back(((s + node_bases[t]) << 1) | 1u);
                rc.n_b += 2;
            }
        if (words.size() >= 0xFFFFFF00ull) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_support_lists: lists too long");
        recs[i] = rc;
    }
    if (n == 0) return VGA_OK;
    const size_t cells = (size_t)n * ps->n_paths;
    hipStream_t st = ctx->stream;
    vga_dbuf<cov_rec> d_recs;
    vga_dbuf<uint32_t> d_words, d_b, d_e;
    VGA_HIP_CHECK_OOM(ctx, d_recs.reserve(n));
    VGA_HIP_CHECK_OOM(ctx, d_words.reserve(words.size() + 1));
    VGA_HIP_CHECK_OOM(ctx, d_b.reserve(cells));
    VGA_HIP_CHECK_OOM(ctx, d_e.reserve(cells));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_recs.p, recs.data(), n * sizeof(cov_rec), hipMemcpyHostToDevice, st));
    if (!words.empty()) VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_words.p, words.data(), words.size() * 4, hipMemcpyHostToDevice, st));
    vga_timers_reset(ctx);
    ps_launch_score(ctx, ps, (uint32_t)n, cov_win_view{d_recs.p, d_words.p, d_words.p}, nullptr, d_b.p, d_e.p, nullptr);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    if (bases_out) VGA_HIP_CHECK(ctx, hipMemcpyAsync(bases_out, d_b.p, cells * 4, hipMemcpyDeviceToHost, st));
    if (edges_out) VGA_HIP_CHECK(ctx, hipMemcpyAsync(edges_out, d_e.p, cells * 4, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    vga_timers_collect(ctx);
    return VGA_OK;
}

extern "C" int vga_path_support_lists(vga_ctx *ctx, uint64_t n, const uint64_t *node_off, const uint32_t *node_ids, const uint32_t *node_bases,
                                      uint32_t *bases_out, uint32_t *edges_out)
{
    if (!ctx) return VGA_ERR_ARG;
    ps_state *ps = ps_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_lists: path support is off (vga_path_support_begin)");
    if (n >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_support_lists: too many lists");
    if (n && (!node_off || (node_off[n] > node_off[0] && (!node_ids || !node_bases))))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_support_lists: null array");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    try {
        return ps_lists(ctx, ps, n, node_off, node_ids, node_bases, bases_out, edges_out);
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_support_lists: out of host memory");
    }
}
