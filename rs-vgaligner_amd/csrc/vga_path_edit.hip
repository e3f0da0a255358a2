// vga_path_edit.hip -- reads x paths edit distance: k_pe_paths, k_pe_encode, k_pe_jobs, k_pe_dist<R>, k_pe_rows and the six C
// entry points vga_path_edit_begin / _read / _last / _reset / _end / _pairs.  See vga_path_edit.hpp for the measure, the shape of
// the kernels and the lane mapping.
//
// All values are integers; the accumulators are sums and counts, so the tables are exact and independent of order.
#include "vga_path_edit.hpp"
#include "vga_path_support.hpp"

#include <algorithm>

// (query, lo, hi, path): the job of one reported alignment and one path.  lo > hi: no window, the pair is not scored.
struct pe_job { uint32_t query, lo, hi, path; };

struct pe_state {
    uint32_t n_paths = 0;
    vga_dbuf<uint32_t> d_step_pos;               // per step of every path, the offset of its first base in d_seq (one more: the end)
    vga_dbuf<unsigned long long> d_step_off;      // n_paths + 1: the steps of path p
    vga_dbuf<unsigned long long> d_seq_off;       // n_paths + 1: seq_p is d_seq[d_seq_off[p] .. d_seq_off[p + 1])
    vga_dbuf<unsigned long long> d_fwd_off, d_fwd;  // per path its forward steps as (node << 32 | step within the path), sorted
    vga_dbuf<uint8_t> d_seq;                      // one letter code per path base
    ps_acc_block acc;                             // n_scored, sum_edit, best, best_alone (n_paths each), n_alignments, n_too_long
    // ---- the last call
    vga_dbuf<uint32_t> d_edit, d_gl_bases, d_gl_edges, d_qlen;
    vga_dbuf<unsigned long long> d_qoff;
    vga_dbuf<pe_job> d_jobs;
    vga_hbuf<unsigned long long> h_qoff;
    vga_hbuf<uint32_t> h_qlen;
    uint64_t last_reads = 0;
    bool have_last = false;
};

namespace {

__global__ __launch_bounds__(256) void k_pe_encode(unsigned long long n, const char *__restrict__ in, uint8_t *__restrict__ out)
{
    const unsigned long long t = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (t < n) out[t] = (uint8_t)pe_code((unsigned char)in[t]);
}

// One thread per path base: the step it lies in (the last step that begins at or before it), then the letter of that step's node
// -- read backwards and complemented for an "id-" step.
__global__ __launch_bounds__(256) void k_pe_paths(uint32_t n_bases, uint32_t n_steps, const uint32_t *__restrict__ step_pos,
                                                   const uint32_t *__restrict__ steps, const uint32_t *__restrict__ node_start,
                                                   const char *__restrict__ seq_fwd, uint8_t *__restrict__ out)
{
    const unsigned long long g = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    if (g >= n_bases) return;
    const uint32_t t = (uint32_t)g;
    uint32_t lo = 0, hi = n_steps;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (step_pos[mid] <= t) lo = mid; else hi = mid;
    }
    const uint32_t h = steps[lo], id = h >> 1, off = t - step_pos[lo];
    const uint32_t s0 = node_start[id - 1], len = node_start[id] - s0;
    if (off >= len) { out[t] = (uint8_t)PE_CODE_OTHER; return; }
    const uint32_t c = pe_code((unsigned char)seq_fwd[(h & 1u) ? s0 + len - 1u - off : s0 + off]);
    out[t] = (uint8_t)((h & 1u) ? pe_code_complement(c) : c);
}

// the first entry of f[0 .. n) that is >= key
__device__ __forceinline__ uint32_t pe_lower_bound(const unsigned long long *__restrict__ f, uint32_t n, unsigned long long key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (f[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One wave per reported alignment, the paths across the lanes (vga_path_edit.hpp).
__global__ __launch_bounds__(64) void k_pe_jobs(uint32_t n, const cov_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                 const uint32_t *__restrict__ host_lists, const uint32_t *__restrict__ node_start, uint32_t n_graph_nodes,
                                                 uint32_t n_paths, uint32_t PW, const uint32_t *__restrict__ node_paths,
                                                 const unsigned long long *__restrict__ fwd_off, const unsigned long long *__restrict__ fwd,
                                                 const unsigned long long *__restrict__ step_off, const uint32_t *__restrict__ step_pos,
                                                 const uint32_t *__restrict__ q_len, pe_job *__restrict__ jobs)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const cov_rec rc = recs[wi];
    const uint32_t *nodes = (rc.flags == 3u ? host_lists : lists) + rc.off;
    const uint32_t m = q_len[wi];
    for (uint32_t p = threadIdx.x; p < n_paths; p += 64u) {
        pe_job job = {wi, 1u, 0u, p};
        const uint32_t word = p >> 5, bit = 1u << (p & 31u);
        uint32_t a = 0, b = 0;
        if (m >= 1u && m <= PE_MAX_QUERY) {
            for (uint32_t t = 0; t < rc.n_a; t++) {
                const uint32_t id = nodes[t];
                if (id >= 1u && id <= n_graph_nodes && (node_paths[(size_t)(id - 1u) * PW + word] & bit)) { a = id; break; }
            }
            for (uint32_t t = rc.n_a; a && t-- > 0;) {
                const uint32_t id = nodes[t];
                if (id >= 1u && id <= n_graph_nodes && (node_paths[(size_t)(id - 1u) * PW + word] & bit)) { b = id; break; }
            }
        }
        if (a && b) {
            const unsigned long long *f = fwd + fwd_off[p];
            const uint32_t nf = (uint32_t)(fwd_off[p + 1] - fwd_off[p]);
            const uint32_t ia = pe_lower_bound(f, nf, (unsigned long long)a << 32);
            const uint32_t jb = pe_lower_bound(f, nf, ((unsigned long long)b + 1ull) << 32);
            if (ia < nf && jb >= 1u && (uint32_t)(f[ia] >> 32) == a && (uint32_t)(f[jb - 1u] >> 32) == b) {
                const uint32_t i = (uint32_t)f[ia], j = (uint32_t)f[jb - 1u];
                if (j >= i) {
                    const unsigned long long s0 = step_off[p];
                    const uint32_t pos0 = step_pos[s0];
                    const pe_window w = pe_window_of(step_pos[s0 + i] - pos0, step_pos[s0 + j] - pos0, node_start[b] - node_start[b - 1u], m,
                                                     step_pos[step_off[p + 1]] - pos0);
                    job.lo = w.lo;
                    job.hi = w.hi;
                }
            }
        }
        jobs[(size_t)wi * n_paths + p] = job;
    }
}

// lane l takes the value of lane l - 1 (DPP wave_shr:1); lane 0 keeps `first`
__device__ __forceinline__ uint32_t pe_from_lane_below(uint32_t first, uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138, 0xF, 0xF, false);
}

// One wave per job (vga_path_edit.hpp): Myers' block recurrence with the horizontal delta carried from block to block -- inside a
// lane through registers, from lane to lane through the wave shift.  A job whose query is served with another R, that has no
// window, or whose query is too long returns at once: `out` is filled with PE_NONE before the launches.
//   out index: row_of[query] * n_paths + path with rows (vga_align_batch), the job's own index without (the seam).
template <int R>
__global__ __launch_bounds__(64) void k_pe_dist(uint32_t n_jobs, const pe_job *__restrict__ jobs, const char *__restrict__ q,
                                                 const unsigned long long *__restrict__ q_off, const uint32_t *__restrict__ q_len,
                                                 const uint8_t *__restrict__ text, const unsigned long long *__restrict__ t_off,
                                                 const uint32_t *__restrict__ row_of, uint32_t n_paths, uint32_t *__restrict__ out)
{
    if (blockIdx.x >= n_jobs) return;
    const pe_job job = jobs[blockIdx.x];
    const uint32_t m = q_len[job.query];
    if (pe_blocks_per_lane(m) != (uint32_t)R || job.lo > job.hi) return;
    const uint32_t lane = threadIdx.x;
    const size_t at = row_of ? (size_t)row_of[job.query] * n_paths + job.path : (size_t)blockIdx.x;
    if (m == 0u) {
        if (lane == 0u) out[at] = 0u;
        return;
    }
    const uint32_t nb = pe_blocks(m), L = pe_lanes(m, (uint32_t)R);
    const char *Q = q + q_off[job.query];
    // ---- the match masks: the wave reads 64 letters of the query at a time, one ballot per letter, the owner of the block keeps them
    uint64_t eq[R][4];
#pragma unroll
    for (int b = 0; b < R; b++)
#pragma unroll
        for (int c = 0; c < 4; c++) eq[b][c] = 0ull;
    for (uint32_t ol = 0; ol < L; ol++) {
#pragma unroll
        for (int b = 0; b < R; b++) {
            const uint32_t idx = (ol * (uint32_t)R + (uint32_t)b) * 64u + lane;
            const uint32_t code = idx < m ? pe_code((unsigned char)Q[idx]) : PE_CODE_OTHER;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint64_t bal = __builtin_amdgcn_ballot_w64(code == (uint32_t)c);
                eq[b][c] = lane == ol ? bal : eq[b][c];
            }
        }
    }
    uint64_t pv[R], mv[R];
#pragma unroll
    for (int b = 0; b < R; b++) { pv[b] = ~0ull; mv[b] = 0ull; }
    const uint32_t kb = (nb - 1u) % (uint32_t)R, sh = (m - 1u) & 63u;  // the block (within its lane) and the bit of row m
    const uint32_t n = job.hi - job.lo;
    const uint8_t *T = text + t_off[job.path] + job.lo;
    int32_t score = (int32_t)m, best = (int32_t)m;
    uint32_t pass = PE_CODE_OTHER, chunk = PE_CODE_OTHER;  // pass: letter | (delta > 0) << 3 | (delta < 0) << 4 from the lane below
    const uint32_t steps = n ? n + L - 1u : 0u;
    for (uint32_t t = 0; t < steps; t++) {
        if ((t & 63u) == 0u) chunk = t + lane < n ? (uint32_t)T[t + lane] : PE_CODE_OTHER;  // 64 columns, coalesced
        const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)chunk, (int)(t & 63u));
        const uint32_t in = lane == 0u ? first : pass;  // block 0 takes delta 0 for every column
        const uint32_t code = in & 7u;
        uint64_t hp = (in >> 3) & 1u, hm = (in >> 4) & 1u;
#pragma unroll
        for (int b = 0; b < R; b++) {
            uint64_t Eq = code == 0u ? eq[b][0] : code == 1u ? eq[b][1] : code == 2u ? eq[b][2] : code == 3u ? eq[b][3] : 0ull;
            const uint64_t Pv = pv[b], Mv = mv[b];
            const uint64_t Xv = Eq | Mv;
            Eq |= hm;
            const uint64_t Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
            uint64_t Ph = Mv | ~(Xh | Pv);
            uint64_t Mh = Pv & Xh;
            if ((uint32_t)b == kb) score += (int32_t)((Ph >> sh) & 1ull) - (int32_t)((Mh >> sh) & 1ull);
            const uint64_t ohp = Ph >> 63, ohm = Mh >> 63;
            Ph = (Ph << 1) | hp;
            Mh = (Mh << 1) | hm;
            pv[b] = Mh | ~(Xv | Ph);
            mv[b] = Ph & Xv;
            hp = ohp;
            hm = ohm;
        }
        best = score < best ? score : best;
        pass = pe_from_lane_below(PE_CODE_OTHER, code | ((uint32_t)hp << 3) | ((uint32_t)hm << 4));
    }
    const uint32_t e = (uint32_t)__builtin_amdgcn_readlane(best, (int)(L - 1u));
    if (lane == 0u) out[at] = e;
}

// One wave per reported alignment: the minimum of its row over the scored paths, the per-path accumulators (acc: n_scored,
// sum_edit, best, best_alone of n_paths words each, n_alignments, n_too_long) and, for the likelihood, the row m - e.
__global__ __launch_bounds__(64) void k_pe_rows(uint32_t n, const uint32_t *__restrict__ row_of, const uint32_t *__restrict__ q_len, uint32_t n_paths,
                                                 const uint32_t *__restrict__ edit, uint32_t *__restrict__ gl_bases, unsigned long long *__restrict__ acc)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const uint32_t lane = threadIdx.x, m = q_len[wi], n_blocks = (n_paths + 63u) >> 6;
    const size_t row = (size_t)row_of[wi] * n_paths;
    uint32_t mn = PE_NONE;
    for (uint32_t p = lane; p < n_paths; p += 64u) mn = min(mn, edit[row + p]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, d));
    uint32_t n_best = 0;
    if (mn != PE_NONE)
        for (uint32_t qb = 0; qb < n_blocks; qb++) {
            const uint32_t p = qb * 64u + lane;
            const bool is = p < n_paths && edit[row + p] == mn;
            n_best += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(is));
        }
    for (uint32_t p = lane; p < n_paths; p += 64u) {
        const uint32_t e = edit[row + p];
        if (gl_bases) gl_bases[row + p] = e == PE_NONE ? 0u : m - e;
        if (e == PE_NONE) continue;
        atomicAdd(acc + p, 1ull);
        if (e) atomicAdd(acc + n_paths + p, (unsigned long long)e);
        if (e == mn) {
            atomicAdd(acc + 2ull * n_paths + p, 1ull);
            if (n_best == 1u) atomicAdd(acc + 3ull * n_paths + p, 1ull);
        }
    }
    if (lane == 0u) {
        atomicAdd(acc + 4ull * n_paths, 1ull);
        if (m > PE_MAX_QUERY) atomicAdd(acc + 4ull * n_paths + 1ull, 1ull);
    }
}

// k_pe_dist for every R that some query of the call is served with (has[R]: the host knows the lengths)
void pe_launch_dist(vga_ctx *ctx, const bool *has, uint32_t n_jobs, const pe_job *jobs, const char *q, const unsigned long long *q_off,
                    const uint32_t *q_len, const uint8_t *text, const unsigned long long *t_off, const uint32_t *row_of, uint32_t n_paths, uint32_t *out)
{
    hipStream_t st = ctx->stream;
    if (has[1]) {
        const int t = vga_timer_begin(ctx, "k_pe_dist", 0, st);
        hipLaunchKernelGGL(k_pe_dist<1>, dim3(n_jobs), dim3(64), 0, st, n_jobs, jobs, q, q_off, q_len, text, t_off, row_of, n_paths, out);
        vga_timer_end(ctx, t);
    }
    if (has[2]) {
        const int t = vga_timer_begin(ctx, "k_pe_dist", 0, st);
        hipLaunchKernelGGL(k_pe_dist<2>, dim3(n_jobs), dim3(64), 0, st, n_jobs, jobs, q, q_off, q_len, text, t_off, row_of, n_paths, out);
        vga_timer_end(ctx, t);
    }
    if (has[4]) {
        const int t = vga_timer_begin(ctx, "k_pe_dist", 0, st);
        hipLaunchKernelGGL(k_pe_dist<4>, dim3(n_jobs), dim3(64), 0, st, n_jobs, jobs, q, q_off, q_len, text, t_off, row_of, n_paths, out);
        vga_timer_end(ctx, t);
    }
}

}  // namespace

pe_state *pe_active(vga_ctx *ctx)
{
    ps_state *ps = ps_active(ctx);
    return ps ? ps->pe.get() : nullptr;
}

const uint32_t *pe_gl_bases(const pe_state *pe) { return pe->d_gl_bases.p; }
const uint32_t *pe_gl_edges(const pe_state *pe) { return pe->d_gl_edges.p; }

int pe_add_call(vga_ctx *ctx, ps_state *ps, const cov_win_view &v, const uint32_t *d_rows, uint64_t nw, uint64_t n_reads, const pe_queries &q, bool with_gl)
{
    pe_state *pe = ps->pe.get();
    const vga_dev_index &ix = ctx->index;
    const size_t cells = (size_t)n_reads * pe->n_paths, n_jobs = (size_t)nw * pe->n_paths;
    hipStream_t st = ctx->stream;
    pe->have_last = false;
    if (n_jobs >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "path edit: %llu alignments x %u paths in one call", (unsigned long long)nw, pe->n_paths);
    VGA_HIP_CHECK_OOM(ctx, pe->d_edit.reserve(cells + 1));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(pe->d_edit.p, 0xFF, cells * 4, st));  // (a read without a reported alignment keeps a NONE row)
    if (with_gl) {
        VGA_HIP_CHECK_OOM(ctx, pe->d_gl_bases.reserve(cells + 1));
        VGA_HIP_CHECK_OOM(ctx, pe->d_gl_edges.reserve(cells + 1));
        VGA_HIP_CHECK(ctx, hipMemsetAsync(pe->d_gl_bases.p, 0, cells * 4, st));
        VGA_HIP_CHECK(ctx, hipMemsetAsync(pe->d_gl_edges.p, 0, cells * 4, st));
    }
    if (nw) {
        VGA_HIP_CHECK(ctx, pe->h_qoff.reserve(nw));
        VGA_HIP_CHECK(ctx, pe->h_qlen.reserve(nw));
        VGA_HIP_CHECK_OOM(ctx, pe->d_qoff.reserve(nw));
        VGA_HIP_CHECK_OOM(ctx, pe->d_qlen.reserve(nw));
        VGA_HIP_CHECK_OOM(ctx, pe->d_jobs.reserve(n_jobs));
        bool has[PE_MAX_R + 1] = {};
        for (uint64_t i = 0; i < nw; i++) {
            pe->h_qoff.p[i] = q.off[i];
            pe->h_qlen.p[i] = q.len[i];
            has[pe_blocks_per_lane(q.len[i])] = true;  // (0: too long, no launch)
        }
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_qoff.p, pe->h_qoff.p, nw * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_qlen.p, pe->h_qlen.p, nw * 4, hipMemcpyHostToDevice, st));
        int t = vga_timer_begin(ctx, "k_pe_jobs", 0, st);
        hipLaunchKernelGGL(k_pe_jobs, dim3((unsigned)nw), dim3(64), 0, st, (uint32_t)nw, v.recs, v.lists, v.host_lists, ix.d_node_start, (uint32_t)ix.n_nodes,
                           pe->n_paths, ps->PW, ps->d_node_paths.p, pe->d_fwd_off.p, pe->d_fwd.p, pe->d_step_off.p, pe->d_step_pos.p, pe->d_qlen.p, pe->d_jobs.p);
        vga_timer_end(ctx, t);
        pe_launch_dist(ctx, has, (uint32_t)n_jobs, pe->d_jobs.p, q.d_reads, pe->d_qoff.p, pe->d_qlen.p, pe->d_seq.p, pe->d_seq_off.p, d_rows, pe->n_paths, pe->d_edit.p);
        t = vga_timer_begin(ctx, "k_pe_rows", 0, st);
        hipLaunchKernelGGL(k_pe_rows, dim3((unsigned)nw), dim3(64), 0, st, (uint32_t)nw, d_rows, pe->d_qlen.p, pe->n_paths, pe->d_edit.p,
                           with_gl ? pe->d_gl_bases.p : nullptr, pe->acc.d.p);
        vga_timer_end(ctx, t);
        VGA_HIP_CHECK(ctx, hipGetLastError());
    }
    pe->last_reads = n_reads;
    pe->have_last = true;  // (the caller waits for the stream before it returns)
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
static int pe_begin(vga_ctx *ctx, ps_state *ps, pe_state *pe)
{
    const vga_dev_index &ix = ctx->index;
    const uint32_t np = ps->n_paths;
    const size_t n_steps = ps->h_steps.size();
    std::vector<uint32_t> pos(n_steps + 1);
    std::vector<unsigned long long> seq_off(np + 1), fwd_off(np + 1), fwd;
    unsigned long long total = 0;
    for (uint32_t p = 0; p < np; p++) {
        seq_off[p] = total;
        fwd_off[p] = fwd.size();
        for (unsigned long long s = ps->h_off[p]; s < ps->h_off[p + 1]; s++) {
            const uint32_t h = ps->h_steps[s], id = h >> 1;
            pos[s] = (uint32_t)total;
            total += ix.node_start[id] - ix.node_start[id - 1];
            if (total >= (1ull << 32))
                return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_edit_begin: the paths hold 2^32 bases or more");
            if (!(h & 1u)) fwd.push_back(((unsigned long long)id << 32) | (s - ps->h_off[p]));
        }
        std::sort(fwd.begin() + (long)fwd_off[p], fwd.end());
    }
    pos[n_steps] = (uint32_t)total;
    seq_off[np] = total;
    fwd_off[np] = fwd.size();
    pe->n_paths = np;
    hipStream_t st = ctx->stream;
    vga_dbuf<uint32_t> d_steps;
    VGA_HIP_CHECK_OOM(ctx, pe->d_step_pos.reserve(n_steps + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->d_step_off.reserve(np + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->d_seq_off.reserve(np + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->d_fwd_off.reserve(np + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->d_fwd.reserve(fwd.size() + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->d_seq.reserve((size_t)total + 1));
    VGA_HIP_CHECK_OOM(ctx, pe->acc.reserve(np));
    VGA_HIP_CHECK_OOM(ctx, d_steps.reserve(n_steps + 1));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_step_pos.p, pos.data(), (n_steps + 1) * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_step_off.p, ps->h_off.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_seq_off.p, seq_off.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_fwd_off.p, fwd_off.data(), (np + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    if (!fwd.empty()) VGA_HIP_CHECK(ctx, hipMemcpyAsync(pe->d_fwd.p, fwd.data(), fwd.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
    if (n_steps) VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_steps.p, ps->h_steps.data(), n_steps * 4, hipMemcpyHostToDevice, st));
    vga_timers_reset(ctx);
    if (total) {
        const int t = vga_timer_begin(ctx, "k_pe_paths", 0, st);
        hipLaunchKernelGGL(k_pe_paths, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (uint32_t)total, (uint32_t)n_steps, pe->d_step_pos.p, d_steps.p,
                           ix.d_node_start, ix.d_seq_fwd, pe->d_seq.p);
        vga_timer_end(ctx, t);
        VGA_HIP_CHECK(ctx, hipGetLastError());
    }
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));  // (the host arrays above are on their way until here)
    vga_timers_collect(ctx);
    return pe->acc.zero(ctx);
}

extern "C" int vga_path_edit_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_begin(ctx, "vga_path_edit_begin", &ps_state::pe, [&](ps_state *ps, pe_state *pe) { return pe_begin(ctx, ps, pe); });
}

extern "C" int vga_path_edit_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    pe_state *pe = pe_active(ctx);
    return ps_child_reset(ctx, pe != nullptr, "vga_path_edit_reset: the edit distance is off (vga_path_edit_begin)", [&]() { return pe->acc.zero(ctx); });
}

extern "C" int vga_path_edit_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    return ps_child_end(ctx, &ps_state::pe);
}

extern "C" int vga_path_edit_read(vga_ctx *ctx, uint64_t *n_scored, uint64_t *sum_edit, uint64_t *best, uint64_t *best_alone, uint64_t *n_alignments,
                                  uint64_t *n_too_long)
{
    if (!ctx) return VGA_ERR_ARG;
    pe_state *pe = pe_active(ctx);
    if (!pe) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_edit_read: the edit distance is off (vga_path_edit_begin)");
    (void)hipSetDevice(ctx->device);
    uint64_t *const dst[4] = {n_scored, sum_edit, best, best_alone};
    return pe->acc.read(ctx, dst, n_alignments, n_too_long);
}

extern "C" int vga_path_edit_last(vga_ctx *ctx, uint64_t n_reads, uint32_t *edit)
{
    if (!ctx) return VGA_ERR_ARG;
    pe_state *pe = pe_active(ctx);
    if (!pe) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_edit_last: the edit distance is off (vga_path_edit_begin)");
    uint32_t *const dst[2] = {edit, nullptr};
    const uint32_t *const src[2] = {pe->d_edit.p, nullptr};
    return ps_read_last(ctx, "vga_path_edit_last", pe->have_last, pe->last_reads, n_reads, pe->n_paths, dst, src);
}

// The kernel seam: explicit strings through k_pe_encode and k_pe_dist, job i = (query i, 0, |text i|, text i).
static int pe_pairs(vga_ctx *ctx, uint64_t n, const uint64_t *q_off, const char *q, const uint64_t *t_off, const char *t, uint32_t *out)
{
    std::vector<pe_job> jobs(n);
    std::vector<uint32_t> qlen(n);
    std::vector<unsigned long long> qo(n + 1), to(n + 1);
    bool has[PE_MAX_R + 1] = {};
    for (uint64_t i = 0; i <= n; i++) { qo[i] = q_off[i] - q_off[0]; to[i] = t_off[i] - t_off[0]; }
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t m = q_off[i + 1] - q_off[i], tl = t_off[i + 1] - t_off[i];
        qlen[i] = (uint32_t)std::min<uint64_t>(m, 0xFFFFFFFFull);  // (anything past PE_MAX_QUERY is skipped alike)
        jobs[i] = {(uint32_t)i, 0u, (uint32_t)tl, (uint32_t)i};
        has[pe_blocks_per_lane(qlen[i])] = true;
    }
    const size_t qb = (size_t)qo[n], tb = (size_t)to[n];
    hipStream_t st = ctx->stream;
    vga_dbuf<char> d_q, d_t;
    vga_dbuf<uint8_t> d_codes;
    vga_dbuf<unsigned long long> d_qo, d_to;
    vga_dbuf<uint32_t> d_qlen, d_out;
    vga_dbuf<pe_job> d_jobs;
    VGA_HIP_CHECK_OOM(ctx, d_q.reserve(qb + 1));
    VGA_HIP_CHECK_OOM(ctx, d_t.reserve(tb + 1));
    VGA_HIP_CHECK_OOM(ctx, d_codes.reserve(tb + 1));
    VGA_HIP_CHECK_OOM(ctx, d_qo.reserve(n + 1));
    VGA_HIP_CHECK_OOM(ctx, d_to.reserve(n + 1));
    VGA_HIP_CHECK_OOM(ctx, d_qlen.reserve(n));
    VGA_HIP_CHECK_OOM(ctx, d_out.reserve(n));
    VGA_HIP_CHECK_OOM(ctx, d_jobs.reserve(n));
    hipError_t e = hipSuccess;
    if (qb) e = hipMemcpyAsync(d_q.p, q + q_off[0], qb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && tb) e = hipMemcpyAsync(d_t.p, t + t_off[0], tb, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qo.p, qo.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_to.p, to.data(), (n + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_qlen.p, qlen.data(), n * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_jobs.p, jobs.data(), n * sizeof(pe_job), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d_out.p, 0xFF, n * 4, st);
    vga_timers_reset(ctx);
    if (e == hipSuccess) {
        if (tb) {
            const int tm = vga_timer_begin(ctx, "k_pe_encode", 0, st);
            hipLaunchKernelGGL(k_pe_encode, dim3((unsigned)((tb + 255) / 256)), dim3(256), 0, st, (unsigned long long)tb, d_t.p, d_codes.p);
            vga_timer_end(ctx, tm);
        }
        pe_launch_dist(ctx, has, (uint32_t)n, d_jobs.p, d_q.p, d_qo.p, d_qlen.p, d_codes.p, d_to.p, nullptr, 1u, d_out.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out.p, n * 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);  // (the host arrays above are on their way until here)
    VGA_HIP_CHECK(ctx, e);
    VGA_HIP_CHECK(ctx, es);
    vga_timers_collect(ctx);
    return VGA_OK;
}

extern "C" int vga_path_edit_pairs(vga_ctx *ctx, uint64_t n, const uint64_t *q_off, const char *q, const uint64_t *t_off, const char *t, uint32_t *out)
{
    if (!ctx) return VGA_ERR_ARG;
    if (n == 0) return VGA_OK;
    if (n >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_edit_pairs: too many pairs");
    if (!q_off || !t_off || !out) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_edit_pairs: null array");
    for (uint64_t i = 0; i < n; i++) {
        if (q_off[i + 1] < q_off[i] || t_off[i + 1] < t_off[i])
            return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_edit_pairs: offsets decrease at pair %llu", (unsigned long long)i);
        if (t_off[i + 1] - t_off[i] >= (1ull << 32))
            return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_path_edit_pairs: text %llu holds 2^32 letters or more", (unsigned long long)i);
    }
    if ((q_off[n] > q_off[0] && !q) || (t_off[n] > t_off[0] && !t)) return vga_set_error(ctx, VGA_ERR_ARG, "vga_path_edit_pairs: null string");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    try {
        return pe_pairs(ctx, n, q_off, q, t_off, t, out);
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_path_edit_pairs: out of host memory");
    }
}
