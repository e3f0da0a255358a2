// vga_coverage.hip -- read coverage of graph bases, nodes and edges: k_cov_runs, k_cov_add, k_cov_depth and the four C entry
// points vga_coverage_begin / _read / _reset / _end.  See vga_coverage.hpp for the shape and why it has two kernels.
//
// Meaning (include/vga_hip.h): an M operation (match or mismatch) adds one to the depth of the base of its row; D and I add
// nothing; every node the path enters (a node crossed only by a deletion included) adds one to node_reads, every consecutive
// pair of path nodes one to the slot of the second in the outgoing part of the first's edge slice.  All counters are 32-bit
// integers added with vector atomics: sums of integers do not depend on order, so the tables are exact and repeatable.
#include "vga_coverage.hpp"

namespace {

// One wave per problem of a finished launch.  Walks the traceback's operations twice (vga_oplist.hpp: opl_block) and writes the
// problem's list: the id of every node the path enters, then one event word per end of a run of M operations on consecutive
// positions of the linearised graph (seq_fwd).  Two passes: lengths first, one atomic add claims the words, then the words.
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
    opl_prob P;
    if (!opl_open<false>(P, pi, lane, probs, outs, ops, orow, rows, node_tab, nullptr, nullptr, ids, offs, split, handles0, handles1, node_start,
                         n_graph_nodes, recs))
        return;
    cov_rec T = {0u, 0u, 0u, 0u};
    uint32_t *nodes_w = nullptr, *ev_w = nullptr;
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        opl_carry c;
        opl_runs runs;
        uint32_t n_nodes = 0;
        for (uint32_t base = 0; base <= P.nops; base += 64) {
            const opl_lane o = opl_block<false>(P, base, lane, c);
            const opl_runs::cut k = runs.step(o.cg && o.op == 0 ? 1u : 0u, o.g, lane);
            if (wr) k.put(ev_w, o.g);
            if (wr && o.opens) nodes_w[n_nodes + (uint32_t)__builtin_popcountll(o.omask & opl_below(lane))] = o.id;
            n_nodes += (uint32_t)__builtin_popcountll(o.omask);
        }
        if (!wr) {
            T.n_a = n_nodes; T.n_b = runs.n;
            if (!opl_claim(T, pi, lane, 0u, list_words, cursor, recs)) return;
            nodes_w = lists + T.off;
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
    const uint32_t *ev = nodes + rc.n_a;
    for (uint32_t i = (uint32_t)lane; i < rc.n_a; i += 64) {
        const uint32_t a = nodes[i];
        if (a < 1u || a > n_graph_nodes) continue;
        atomicAdd(node_reads + (a - 1), 1u);
        if (i + 1 < rc.n_a) {
            const uint32_t want = nodes[i + 1] << 1;  // forward handle of the next path node
            const uint32_t e1 = edge_idx[a];
            for (uint32_t t = edge_idx[a - 1] + edges_to[a - 1]; t < e1; t++)
                if (edges[t] == want) { atomicAdd(edge_reads + t, 1u); break; }
        }
    }
    for (uint32_t i = (uint32_t)lane; i < rc.n_b; i += 64) {
        const uint32_t w = ev[i];
        if ((w >> 1) <= seq_length) atomicAdd(diff + (w >> 1), (w & 1u) ? 0xFFFFFFFFu : 1u);
    }
}

// depth[i] = diff[0] + ... + diff[i]: one workgroup, a contiguous piece per thread (opl_block_scan)
__global__ __launch_bounds__(1024) void k_cov_depth(const uint32_t *__restrict__ diff, uint32_t *__restrict__ depth, uint32_t n)
{
    uint32_t a, b;
    uint32_t run = opl_block_scan(diff, n, a, b);
    for (uint32_t i = a; i < b; i++) { run += diff[i]; depth[i] = run; }
}

}  // namespace

// The counters of a context's index while counting is on (vga_dev_index::cov: released with the index), and the lists
struct cov_state : oplist_state {
    uint32_t users = 0;  // COV_USER_*: who reads the lists (the counters below exist while COV_USER_COVERAGE is among them)
    uint32_t n_nodes = 0, n_edges = 0;
    vga_dbuf<uint32_t> d_diff, d_node, d_edge, d_depth;
};

cov_state *cov_lists_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? ctx->index.cov.get() : nullptr; }
cov_state *cov_active(vga_ctx *ctx)
{
    cov_state *cv = cov_lists_active(ctx);
    return cv && (cv->users & COV_USER_COVERAGE) ? cv : nullptr;
}

int cov_lists_acquire(vga_ctx *ctx, uint32_t user, const char *who)
{
    const int rc = oplist_make(ctx, ctx->index.cov, who);
    if (rc == VGA_OK) ctx->index.cov->users |= user;
    return rc;
}

void cov_lists_release(vga_ctx *ctx, uint32_t user)
{
    cov_state *cv = ctx->index.cov.get();
    if (!cv) return;
    cv->users &= ~user;
    if (!cv->users) { ctx->index.cov.reset(); return; }
    if (user == COV_USER_COVERAGE) { cv->d_diff.release(); cv->d_node.release(); cv->d_edge.release(); cv->d_depth.release(); }
}

cov_win_view cov_staged_winners(const cov_state *cv, size_t nw)
{
    return nw ? cov_win_view{cv->lists.d_win.p, cv->lists.d_lists.p, cv->lists.d_host_lists.p} : cov_win_view{nullptr, nullptr, nullptr};
}

static void cov_keep_from_ops(oplist_call &lists, uint32_t p, const oplist_ops &o)
{
    std::vector<uint32_t> nodes;
    oplist_runs_host runs;
    oplist_walk_host<false>(o, [&](const oplist_op &k) {
        if (k.enters) nodes.push_back(k.id);
        runs.step(k.cg && k.op == 0, k.g);
    });
    runs.close();
    lists.keep_host(p, nodes, runs.ev, 0u);
}

static int cov_add(vga_ctx *ctx, oplist_state *s, size_t nw)
{
    cov_state *cv = static_cast<cov_state *>(s);
    const vga_dev_index &ix = ctx->index;
    return oplist_add_staged(ctx, cv, nw, "k_cov_add", k_cov_add, [] { return VGA_OK; }, ix.d_edge_idx, ix.d_edges_to, ix.d_edges, cv->n_nodes, cv->seq_length, cv->d_diff.p,
                             cv->d_node.p, cv->d_edge.p);
}

static std::vector<oplist_counter> cov_counters(const vga_dev_index &ix, oplist_state *s)
{
    cov_state *cv = static_cast<cov_state *>(s);
    cv->n_nodes = (uint32_t)ix.n_nodes; cv->n_edges = (uint32_t)ix.n_edges;
    return {{&cv->d_diff, (size_t)cv->seq_length + 1, true}, {&cv->d_node, (size_t)cv->n_nodes + 1, true}, {&cv->d_edge, (size_t)cv->n_edges + 1, true},
            {&cv->d_depth, (size_t)cv->seq_length + 1, false}};
}

// The lists are made while any reader is on (path support holds them too: the users mask), the counters while coverage is
const oplist_maker &cov_maker()
{
    static const oplist_maker m = {
        OPLIST_TEXT_COV,
        [](vga_ctx *ctx) -> oplist_state * { return cov_lists_active(ctx); },
        [](vga_ctx *ctx) -> oplist_state * { return cov_active(ctx); },
        &poa_switches::has_cov_words, &poa_switches::cov_words,
        [](vga_ctx *ctx, oplist_call &lists, const oplist_launch &L) { return oplist_enqueue<false>(ctx, lists, L, "k_cov_runs", k_cov_runs); },
        cov_keep_from_ops,
        cov_add,
        [](const vga_dev_index &ix) { return ix.seq_length < (1ull << 31) && ix.n_nodes < (1ull << 31) && ix.n_edges < (1ull << 32); },
        [](vga_ctx *ctx, const char *fn) { return cov_lists_acquire(ctx, COV_USER_COVERAGE, fn); },
        [](vga_ctx *ctx) { cov_lists_release(ctx, COV_USER_COVERAGE); },
        cov_counters,
        nullptr,
    };
    return m;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_coverage_begin(vga_ctx *ctx) { return oplist_begin(ctx, cov_maker(), __func__); }
extern "C" int vga_coverage_reset(vga_ctx *ctx) { return oplist_reset(ctx, cov_maker(), __func__); }
extern "C" int vga_coverage_end(vga_ctx *ctx) { return oplist_end(ctx, cov_maker()); }

extern "C" int vga_coverage_read(vga_ctx *ctx, uint32_t *base_depth, uint32_t *node_reads, uint32_t *edge_reads, uint64_t *n_alignments)
{
    cov_state *cv = static_cast<cov_state *>(oplist_on(ctx, cov_maker(), __func__));
    if (!cv) return VGA_ERR_ARG;
    const int rc = oplist_wrapped(ctx, cv, __func__);
    if (rc != VGA_OK) return rc;
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
