// vga_coverage.hip -- read coverage of graph bases, nodes and edges: k_cov_runs, k_cov_add, k_cov_depth and the four C entry
// points vga_coverage_begin / _read / _reset / _end.  See vga_coverage.hpp for the shape and why it has two kernels.
//
// Meaning (include/vga_hip.h): an M operation (match or mismatch) adds one to the depth of the base of its row; D and I add
// nothing; every node the path enters (a node crossed only by a deletion included) adds one to node_reads, every consecutive
// pair of path nodes one to the slot of the second in the outgoing part of the first's edge slice.  All counters are 32-bit
// integers added with vector atomics: sums of integers do not depend on order, so the tables are exact and repeatable.
#include "vga_coverage.hpp"

#include <algorithm>

namespace {

// ---- wave helpers (64 lanes)
__device__ __forceinline__ int cov_scan_add(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}
__device__ __forceinline__ int cov_scan_max(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v = t > v ? t : v;
    }
    return v;
}
// the value of the lane below; lane 0 takes `carry` (the last lane of the previous block)
__device__ __forceinline__ uint32_t cov_shr1(uint32_t v, uint32_t carry, int lane)
{
    const uint32_t t = (uint32_t)__shfl_up((int)v, 1);
    return lane == 0 ? carry : t;
}

// One wave per problem of a finished launch.  Reads the traceback's operations once per pass, forward, 64 at a time (they are
// stored sink -> source), and writes the problem's list: the id of every node the path enters, then one event word per end of a
// run of M operations on consecutive positions of the linearised graph (seq_fwd): position << 1 where a run starts, (position
// behind its last base) << 1 | 1 where it ends.  A row opens a node exactly when its row record has predecessors of its own
// (k_poa_text's rule); only those rows look their node up (binary search over the node table, handle from the subgraph store,
// start from the index), every other row takes the offset  position - row  of the latest opening row before it.  Two passes:
// lengths first, one atomic add claims the words, then the words.  ids[2 i] is problem i's index in the subgraph store.
__global__ __launch_bounds__(64) void k_cov_runs(uint32_t n, const poa_prob *__restrict__ probs, const poa_out *__restrict__ outs,
                                                  const uint8_t *__restrict__ ops, const uint32_t *__restrict__ orow, const poa_row *__restrict__ rows,
                                                  const uint4 *__restrict__ node_tab, const uint32_t *__restrict__ ids, const sg_off *__restrict__ offs,
                                                  uint32_t split, const uint32_t *__restrict__ handles0, const uint32_t *__restrict__ handles1,
                                                  const uint32_t *__restrict__ node_start, uint32_t n_graph_nodes, uint32_t *__restrict__ lists,
                                                  uint32_t list_words, unsigned long long *__restrict__ cursor, cov_rec *__restrict__ recs)
{
    const uint32_t pi = blockIdx.x;
    if (pi >= n) return;
    const int lane = threadIdx.x;
    const poa_prob pb = probs[pi];
    const poa_out po = outs[pi];
    cov_rec T = {0u, 0u, 0u, 0u};
    if (po.status != POA_ST_OK) {
        if (lane == 0) recs[pi] = T;
        return;
    }
    const uint32_t p = ids[2 * pi];
    const uint32_t *hd = (p >= split ? handles1 : handles0) + offs[p].node0;
    const uint32_t nops = po.nops;
    const uint8_t *op_p = ops + pb.ops0;
    const uint32_t *or_p = orow + pb.ops0;
    const poa_row *R = rows + pb.row0;
    const uint4 *ntab = node_tab + pb.node0;
    const uint32_t nv = pb.n_nodes;  // entries incl. the virtual source (entry 0)
    auto node_of = [&](uint32_t row) -> uint32_t {  // 0-based index of the real node that holds `row`
        uint32_t lo = 1, hi = nv;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ntab[mid].x <= row) lo = mid; else hi = mid;
        }
        return lo - 1;
    };
    uint32_t *nodes_w = nullptr, *ev_w = nullptr;
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        uint32_t c_m = 0, c_g = 0, c_delta = 0;  // carried from block to block: was the last operation an M, its position, the open node's offset
        uint32_t n_nodes = 0, n_ev = 0;
        for (uint32_t base = 0; base <= nops; base += 64) {
            const uint32_t f = base + (uint32_t)lane;
            const bool valid = f < nops;
            uint32_t op = 3, row = 0;
            if (valid) { op = op_p[nops - 1 - f]; row = or_p[nops - 1 - f]; }
            const bool cg = valid && (op == 0 || op == 2) && row >= 1u && row <= pb.N;
            const bool opens = cg && R[row].npred != 0u;
            uint32_t my_delta = 0, my_id = 0;
            if (opens) {
                my_id = hd[node_of(row)] >> 1;
                if (my_id < 1u || my_id > n_graph_nodes) my_id = 1u;  // (cannot happen with a store built from this index)
                my_delta = node_start[my_id - 1] - row;
            }
            const int idx = cov_scan_max(opens ? lane : -1, lane);
            const uint32_t got = (uint32_t)__shfl((int)my_delta, idx >= 0 ? idx : 0);
            const uint32_t g = row + (idx >= 0 ? got : c_delta);
            const uint32_t is_m = cg && op == 0 ? 1u : 0u;
            const uint32_t p_m = cov_shr1(is_m, c_m, lane), p_g = cov_shr1(g, c_g, lane);
            const bool cont = is_m && p_m && p_g + 1u == g;
            const bool start = is_m && !cont, end = p_m && !cont;
            const int len = (start ? 1 : 0) + (end ? 1 : 0);
            const int inc = cov_scan_add(len, lane);
            if (wr && len) {
                uint32_t *w = ev_w + n_ev + (uint32_t)(inc - len);
                if (end) *w++ = ((p_g + 1u) << 1) | 1u;
                if (start) *w = g << 1;
            }
            n_ev += (uint32_t)__builtin_amdgcn_readlane(inc, 63);
            const uint64_t omask = __builtin_amdgcn_ballot_w64(opens);
            if (wr && opens) nodes_w[n_nodes + (uint32_t)__builtin_popcountll(omask & ((1ull << lane) - 1ull))] = my_id;
            n_nodes += (uint32_t)__builtin_popcountll(omask);
            c_m = (uint32_t)__builtin_amdgcn_readlane((int)is_m, 63);
            c_g = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
            if (omask) c_delta = (uint32_t)__shfl((int)my_delta, 63 - __builtin_clzll(omask));
        }
        if (!wr) {
            const uint32_t words = n_nodes + n_ev;
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(cursor, (unsigned long long)words);
            at = (unsigned long long)__shfl((long long)at, 0);
            T.n_nodes = n_nodes; T.n_events = n_ev;
            if (at + words > (unsigned long long)list_words) {
                T.flags = 2u;
                if (lane == 0) recs[pi] = T;
                return;
            }
            T.off = (uint32_t)at;
            nodes_w = lists + at;
            ev_w = nodes_w + n_nodes;
        }
    }
    T.flags = 1u;
    if (lane == 0) recs[pi] = T;
}

// One wave per reported alignment: its list goes into the counters.  Per node one add into node_reads and, for the pair it
// forms with the next node of the path, a scan of its (short) outgoing slice for the slot of that node; per event +1 or -1 into
// the difference array over the bases (seq_length + 1 words), which vga_coverage_read turns into depths with a prefix sum.
// Hundreds of atomics per read instead of one per base: 10 000 reads on 22 595 graph bases would otherwise all land on the same
// few lines.
__global__ __launch_bounds__(64) void k_cov_add(uint32_t n, const cov_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                 const uint32_t *__restrict__ host_lists, const uint32_t *__restrict__ edge_idx,
                                                 const uint32_t *__restrict__ edges_to, const uint32_t *__restrict__ edges, uint32_t n_graph_nodes,
                                                 uint32_t seq_length, uint32_t *__restrict__ diff, uint32_t *__restrict__ node_reads,
                                                 uint32_t *__restrict__ edge_reads)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const int lane = threadIdx.x;
    const cov_rec rc = recs[wi];
    const uint32_t *nodes = (rc.flags == 3u ? host_lists : lists) + rc.off;
    const uint32_t *ev = nodes + rc.n_nodes;
    for (uint32_t i = (uint32_t)lane; i < rc.n_nodes; i += 64) {
        const uint32_t a = nodes[i];
        if (a < 1u || a > n_graph_nodes) continue;
        atomicAdd(node_reads + (a - 1), 1u);
        if (i + 1 < rc.n_nodes) {
            const uint32_t want = nodes[i + 1] << 1;  // forward handle of the next path node
            const uint32_t e1 = edge_idx[a];
            for (uint32_t t = edge_idx[a - 1] + edges_to[a - 1]; t < e1; t++)
                if (edges[t] == want) { atomicAdd(edge_reads + t, 1u); break; }
        }
    }
    for (uint32_t i = (uint32_t)lane; i < rc.n_events; i += 64) {
        const uint32_t w = ev[i];
        if ((w >> 1) <= seq_length) atomicAdd(diff + (w >> 1), (w & 1u) ? 0xFFFFFFFFu : 1u);
    }
}

// depth[i] = diff[0] + ... + diff[i]: one workgroup, a contiguous piece per thread, the pieces' sums scanned in LDS
__global__ __launch_bounds__(1024) void k_cov_depth(const uint32_t *__restrict__ diff, uint32_t *__restrict__ depth, uint32_t n)
{
    __shared__ uint32_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t piece = (n + 1023u) / 1024u;
    const uint64_t a64 = (uint64_t)tid * piece, b64 = a64 + piece;
    const uint32_t a = a64 < n ? (uint32_t)a64 : n, b = b64 < n ? (uint32_t)b64 : n;
    uint32_t s = 0;
    for (uint32_t i = a; i < b; i++) s += diff[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t t = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    uint32_t run = tid ? part[tid - 1] : 0u;
    for (uint32_t i = a; i < b; i++) { run += diff[i]; depth[i] = run; }
}

}  // namespace

// The counters of a context's index while counting is on (vga_dev_index::cov: released with the index), and the lists of the
// vga_align_batch call in progress.
struct cov_state {
    uint32_t users = 0;  // COV_USER_*: who reads the lists (the counters below exist while COV_USER_COVERAGE is among them)
    uint32_t seq_length = 0, n_nodes = 0, n_edges = 0;
    vga_dbuf<uint32_t> d_diff, d_node, d_edge, d_depth;
    uint64_t n_alignments = 0;
    // ---- one call
    vga_dbuf<uint32_t> d_lists;             // the lists k_cov_runs writes, claimed through d_cur
    uint32_t list_words = 0;
    vga_dbuf<unsigned long long> d_cur;
    vga_dbuf<cov_rec> d_recs[POA_SLOTS];    // per staged problem of the slot's launch
    vga_hbuf<cov_rec> h_recs[POA_SLOTS][2];
    std::vector<cov_rec> recs;              // per problem of the call
    std::vector<uint32_t> host_lists;       // lists the host built (flags 3)
    vga_dbuf<uint32_t> d_host_lists;
    vga_dbuf<cov_rec> d_win;
    vga_hbuf<cov_rec> h_win;
};

cov_state *cov_lists_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? (cov_state *)ctx->index.cov : nullptr; }
cov_state *cov_active(vga_ctx *ctx)
{
    cov_state *cv = cov_lists_active(ctx);
    return cv && (cv->users & COV_USER_COVERAGE) ? cv : nullptr;
}

static void cov_release(vga_ctx *ctx)
{
    if (ctx->index.cov && ctx->index.cov_free) ctx->index.cov_free(ctx->index.cov);
    ctx->index.cov = nullptr;
    ctx->index.cov_free = nullptr;
}

int cov_lists_acquire(vga_ctx *ctx, uint32_t user, const char *who)
{
    try {
        if (!ctx->index.cov) {
            ctx->index.cov = new cov_state();
            ctx->index.cov_free = [](void *q) { delete (cov_state *)q; };
        }
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "%s: out of host memory", who);
    }
    ((cov_state *)ctx->index.cov)->users |= user;
    return VGA_OK;
}

void cov_lists_release(vga_ctx *ctx, uint32_t user)
{
    cov_state *cv = (cov_state *)ctx->index.cov;
    if (!cv) return;
    cv->users &= ~user;
    if (!cv->users) { cov_release(ctx); return; }
    if (user == COV_USER_COVERAGE) { cv->d_diff.release(); cv->d_node.release(); cv->d_edge.release(); cv->d_depth.release(); }
}

int cov_call_begin(vga_ctx *ctx, cov_state *cv, uint64_t n, uint64_t total_q)
{
    // a list holds the path's nodes and two words per run: about a word per read base on a graph of short nodes with reads of
    // 10 % errors.  Not a bound -- a problem that finds no room says so and the host builds its list (VGA_COV_LIST_WORDS caps the
    // buffer: the tests force that route with it)
    uint64_t words = std::min<uint64_t>(total_q + 256ull * n + 4096ull, 0xFFFFFF00ull);
    if (const char *e = getenv("VGA_COV_LIST_WORDS")) words = std::min<uint64_t>(words, (uint64_t)std::max(0ll, atoll(e)));
    VGA_HIP_CHECK(ctx, cv->d_lists.reserve(words + 1));
    VGA_HIP_CHECK(ctx, cv->d_cur.reserve(1));
    cv->list_words = (uint32_t)words;
    VGA_HIP_CHECK(ctx, hipMemsetAsync(cv->d_cur.p, 0, sizeof(unsigned long long), ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the launches' streams do not wait for the context's)
    cv->recs.assign(n, cov_rec{0u, 0u, 0u, 0u});
    cv->host_lists.clear();
    return VGA_OK;
}

hipError_t cov_enqueue_runs(vga_ctx *ctx, cov_state *cv, hipStream_t st, int slot, int oset, uint32_t nb, const poa_launch_bufs &b, const uint32_t *ids,
                            const sg_store &store)
{
    hipError_t e;
    if ((e = cv->d_recs[slot].reserve(nb)) != hipSuccess) return e;
    if ((e = cv->h_recs[slot][oset].reserve(nb)) != hipSuccess) return e;
    const int t = vga_timer_begin(ctx, "k_cov_runs", 0, st);
    hipLaunchKernelGGL(k_cov_runs, dim3(nb), dim3(64), 0, st, nb, b.probs, b.outs, b.ops, b.orow, b.rows, b.ntab, ids, store.d_off, (uint32_t)store.split,
                       store.part[0].d_handles, store.part[1].d_handles, ctx->index.d_node_start, (uint32_t)ctx->index.n_nodes, cv->d_lists.p,
                       cv->list_words, cv->d_cur.p, cv->d_recs[slot].p);
    vga_timer_end(ctx, t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(cv->h_recs[slot][oset].p, cv->d_recs[slot].p, nb * sizeof(cov_rec), hipMemcpyDeviceToHost, st);
}

const cov_rec *cov_launch_recs(const cov_state *cv, int slot, int oset) { return cv->h_recs[slot][oset].p; }

void cov_keep(cov_state *cv, uint32_t p, const cov_rec &r) { cv->recs[p] = r; }

void cov_keep_from_ops(cov_state *cv, uint32_t p, const uint8_t *ops, const uint32_t *orow, uint32_t nops, const uint32_t *first_row, uint32_t n_nodes,
                       const uint32_t *handles, const std::vector<uint32_t> &node_start)
{
    std::vector<uint32_t> nodes, ev;
    bool prev_m = false;
    uint32_t pg = 0, v = 0;
    for (uint32_t x = nops; x > 0; x--) {
        const uint32_t op = ops[x - 1], r = orow[x - 1];
        if (op != 0 && op != 2) {
            if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
            prev_m = false;
            continue;
        }
        while (v + 1 < n_nodes && first_row[v + 1] <= r) v++;  // rows ascend along the path
        const uint32_t id = handles[v] >> 1;
        if (r == first_row[v]) nodes.push_back(id);
        const uint32_t g = node_start[id - 1] + (r - first_row[v]);
        if (op == 0) {
            if (!(prev_m && pg + 1 == g)) {
                if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
                ev.push_back(g << 1);
            }
            prev_m = true;
            pg = g;
        } else {
            if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
            prev_m = false;
        }
    }
    if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
    cov_rec rc = {(uint32_t)cv->host_lists.size(), (uint32_t)nodes.size(), (uint32_t)ev.size(), 3u};
    cv->host_lists.insert(cv->host_lists.end(), nodes.begin(), nodes.end());
    cv->host_lists.insert(cv->host_lists.end(), ev.begin(), ev.end());
    cv->recs[p] = rc;
}

int cov_stage_winners(vga_ctx *ctx, cov_state *cv, const std::vector<uint32_t> &winners, cov_win_view &v)
{
    const size_t nw = winners.size();
    v = cov_win_view{nullptr, nullptr, nullptr};
    if (nw == 0) return VGA_OK;
    VGA_HIP_CHECK(ctx, cv->h_win.reserve(nw));
    VGA_HIP_CHECK(ctx, cv->d_win.reserve(nw));
    for (size_t i = 0; i < nw; i++) {
        const cov_rec &r = cv->recs[winners[i]];
        if (r.flags != 1u && r.flags != 3u)
            return vga_set_error(ctx, VGA_ERR_HIP, "coverage: reported alignment %zu has no run list (flags %u)", i, r.flags);
        cv->h_win.p[i] = r;
    }
    hipStream_t st = ctx->stream;
    VGA_HIP_CHECK(ctx, cv->d_host_lists.reserve(cv->host_lists.size() + 1));
    if (!cv->host_lists.empty())
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(cv->d_host_lists.p, cv->host_lists.data(), cv->host_lists.size() * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(cv->d_win.p, cv->h_win.p, nw * sizeof(cov_rec), hipMemcpyHostToDevice, st));
    v = cov_win_view{cv->d_win.p, cv->d_lists.p, cv->d_host_lists.p};
    return VGA_OK;
}

int cov_add_winners(vga_ctx *ctx, cov_state *cv, size_t nw)
{
    if (nw == 0) return VGA_OK;
    hipStream_t st = ctx->stream;
    const vga_dev_index &ix = ctx->index;
    const int t = vga_timer_begin(ctx, "k_cov_add", 0, st);
    hipLaunchKernelGGL(k_cov_add, dim3((unsigned)nw), dim3(64), 0, st, (uint32_t)nw, cv->d_win.p, cv->d_lists.p, cv->d_host_lists.p, ix.d_edge_idx,
                       ix.d_edges_to, ix.d_edges, cv->n_nodes, cv->seq_length, cv->d_diff.p, cv->d_node.p, cv->d_edge.p);
    vga_timer_end(ctx, t);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    cv->n_alignments += nw;
    vga_timers_collect(ctx);  // (poa_run collected before this launch: once more, with it)
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
static int cov_zero(vga_ctx *ctx, cov_state *cv)
{
    VGA_HIP_CHECK(ctx, hipMemsetAsync(cv->d_diff.p, 0, ((size_t)cv->seq_length + 1) * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(cv->d_node.p, 0, ((size_t)cv->n_nodes + 1) * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(cv->d_edge.p, 0, ((size_t)cv->n_edges + 1) * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    cv->n_alignments = 0;
    return VGA_OK;
}

extern "C" int vga_coverage_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_coverage_begin: no index uploaded");
    const vga_dev_index &ix = ctx->index;
    if (ix.seq_length >= (1ull << 31) || ix.n_nodes >= (1ull << 31) || ix.n_edges >= (1ull << 32))
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_coverage_begin: graph too large for 32-bit positions");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    int rc = cov_lists_acquire(ctx, COV_USER_COVERAGE, "vga_coverage_begin");
    if (rc != VGA_OK) return rc;
    cov_state *cv = (cov_state *)ctx->index.cov;
    cv->seq_length = (uint32_t)ix.seq_length; cv->n_nodes = (uint32_t)ix.n_nodes; cv->n_edges = (uint32_t)ix.n_edges;
    hipError_t e = cv->d_diff.reserve((size_t)cv->seq_length + 1);
    if (e == hipSuccess) e = cv->d_node.reserve((size_t)cv->n_nodes + 1);
    if (e == hipSuccess) e = cv->d_edge.reserve((size_t)cv->n_edges + 1);
    if (e == hipSuccess) e = cv->d_depth.reserve((size_t)cv->seq_length + 1);
    rc = e == hipSuccess ? cov_zero(ctx, cv) : vga_set_error(ctx, VGA_ERR_NOMEM, "vga_coverage_begin: %s", hipGetErrorString(e));
    if (rc != VGA_OK) cov_lists_release(ctx, COV_USER_COVERAGE);
    return rc;
}

extern "C" int vga_coverage_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    cov_state *cv = cov_active(ctx);
    if (!cv) return vga_set_error(ctx, VGA_ERR_ARG, "vga_coverage_reset: counting is off (vga_coverage_begin)");
    (void)hipSetDevice(ctx->device);
    return cov_zero(ctx, cv);
}

extern "C" int vga_coverage_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    cov_lists_release(ctx, COV_USER_COVERAGE);
    return VGA_OK;
}

extern "C" int vga_coverage_read(vga_ctx *ctx, uint32_t *base_depth, uint32_t *node_reads, uint32_t *edge_reads, uint64_t *n_alignments)
{
    if (!ctx) return VGA_ERR_ARG;
    cov_state *cv = cov_active(ctx);
    if (!cv) return vga_set_error(ctx, VGA_ERR_ARG, "vga_coverage_read: counting is off (vga_coverage_begin)");
    if (cv->n_alignments >= 0xFFFFFFFFull)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_coverage_read: %llu alignments counted: a 32-bit counter may have wrapped",
                             (unsigned long long)cv->n_alignments);
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (base_depth && cv->seq_length) {
        hipLaunchKernelGGL(k_cov_depth, dim3(1), dim3(1024), 0, st, cv->d_diff.p, cv->d_depth.p, cv->seq_length);
        VGA_HIP_CHECK(ctx, hipGetLastError());
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(base_depth, cv->d_depth.p, (size_t)cv->seq_length * 4, hipMemcpyDeviceToHost, st));
    }
    if (node_reads && cv->n_nodes) VGA_HIP_CHECK(ctx, hipMemcpyAsync(node_reads, cv->d_node.p, (size_t)cv->n_nodes * 4, hipMemcpyDeviceToHost, st));
    if (edge_reads && cv->n_edges) VGA_HIP_CHECK(ctx, hipMemcpyAsync(edge_reads, cv->d_edge.p, (size_t)cv->n_edges * 4, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    if (n_alignments) *n_alignments = cv->n_alignments;
    return VGA_OK;
}
