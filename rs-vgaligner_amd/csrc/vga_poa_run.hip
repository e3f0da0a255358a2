// vga_poa_run.hip -- host orchestration of the POA engine: poa_run (validate and order, size and obtain the pool, then the
// pipeline of sub-batches: choose, stage, launch, fetch text, requeue, post-process, account) and the C entry points built on it
// (vga_align_prepare, vga_poa_batch).  No kernel is visible here: launches go through vga_poa_launch.hpp, the launch shape comes
// from vga_poa_shape.hpp, the traceback pool is vga_poa_pool.hip.  The engine itself is described at the top of vga_poa.hip.
#include "vga_common.hpp"
#include "vga_oplist.hpp"
#include "vga_poa_internal.hpp"
#include "vga_poa_pool.hpp"

#include <algorithm>
#include <chrono>
#include <memory>
#include <thread>

namespace {

struct poa_prep {
    bool ok = false;
    uint32_t N = 0, qlen = 0;
    int32_t longest = 0;                // graph bases on the longest source-sink path
    uint32_t life = 1;                  // largest dst - src over the edges: how many node-end rows a value row must outlive
    std::vector<uint4> ntab;            // node table incl. the source entry
    std::vector<uint32_t> preds, sinks; // row ids
    std::vector<uint32_t> first_row;    // per input node
    uint32_t n_ntab = 0, n_preds = 0, n_sinks = 0;  // entries of the three lists (with a device store the vectors stay empty)
    const uint32_t *first_row_p = nullptr;          // first rows, n_ntab - 1 entries (host graphs: first_row.data())
};

// Node-level graph description: first rows, predecessor rows in edge-list order, remain of the last base of each
// node (over the nodes, last first: the longest path, or with first_edge the path through the first out-edge in
// edge-list order -- vga_poa_params.remain_rule), sink predecessors.  Mirrors the row construction of oracle/og_poa.c.
void poa_prepare(const poa_view &v, poa_prep &g, bool first_edge)
{
    g.ok = false;
    const uint64_t nv = v.n_nodes;
    if (nv == 0 || v.qlen >= (1u << 24)) return;
    g.first_row.resize(nv);
    std::vector<uint32_t> last_row(nv);
    uint64_t N = 0;
    for (uint64_t i = 0; i < nv; i++) {
        const uint64_t len = v.node_off[i + 1] - v.node_off[i];
        if (len == 0 || len >= (1u << 24)) return;
        g.first_row[i] = (uint32_t)(N + 1);
        N += len;
        last_row[i] = (uint32_t)N;
    }
    if (N >= (1ull << 31)) return;
    g.N = (uint32_t)N;
    g.qlen = v.qlen;
    std::vector<uint32_t> in_off(nv + 1, 0), out_off(nv + 1, 0);
    g.life = 1;
    std::vector<uint32_t> reach(nv, 0);  // per node: how far (in nodes) its farthest successor is
    for (uint64_t e = 0; e < v.n_edges; e++) {
        if (v.esrc[e] >= v.edst[e] || v.edst[e] >= nv) return;
        in_off[v.edst[e] + 1]++;
        out_off[v.esrc[e] + 1]++;
        reach[v.esrc[e]] = std::max(reach[v.esrc[e]], v.edst[e] - v.esrc[e]);
    }
    // nodes whose value row is read far ahead keep it for good; the rest share a ring of POA_RING_SPAN + 1 rows
    for (uint64_t i = 0; i < nv; i++)
        if (reach[i] <= POA_RING_SPAN) g.life = std::max(g.life, reach[i]);
    for (uint64_t i = 0; i < nv; i++) { in_off[i + 1] += in_off[i]; out_off[i + 1] += out_off[i]; }
    std::vector<uint32_t> in_adj(v.n_edges ? v.n_edges : 1), out_adj(v.n_edges ? v.n_edges : 1), fi(nv, 0), fo(nv, 0);
    for (uint64_t e = 0; e < v.n_edges; e++) {
        in_adj[in_off[v.edst[e]] + fi[v.edst[e]]++] = v.esrc[e];
        out_adj[out_off[v.esrc[e]] + fo[v.esrc[e]]++] = v.edst[e];
    }
    // remain of the LAST base of each node; interior bases add their distance to it on the device
    std::vector<int32_t> remain_last(nv, 0), remain_first(nv, 0);
    for (uint64_t i = nv; i-- > 0;) {
        int32_t rl = 0;
        for (uint32_t t = out_off[i]; t < out_off[i + 1]; t++) {
            rl = std::max(rl, 1 + remain_first[out_adj[t]]);
            if (first_edge) break;
        }
        remain_last[i] = rl;
        remain_first[i] = rl + (int32_t)(last_row[i] - g.first_row[i]);
    }
    int32_t longest = 0;
    bool have_src = false;
    g.ntab.clear();
    g.preds.clear();
    g.sinks.clear();
    g.ntab.resize(nv + 1);
    for (uint64_t i = 0; i < nv; i++) {
        const uint32_t deg = in_off[i + 1] - in_off[i];
        if (deg > 255) return;
        const uint32_t pstart = (uint32_t)g.preds.size();
        if (deg == 0) {
            g.preds.push_back(0);
            if (!(first_edge && have_src)) longest = std::max(longest, 1 + remain_first[i]);
            have_src = true;
        } else {
            for (uint32_t t = in_off[i]; t < in_off[i + 1]; t++) g.preds.push_back(last_row[in_adj[t]]);
        }
        const uint32_t len = last_row[i] - g.first_row[i] + 1;
        const bool is_sink = out_off[i + 1] == out_off[i];
        // .z: remain of the node's last base; bit 31 marks a node without successors (its last row feeds the sink),
        // bit 30 a node whose value row is read more than POA_RING_SPAN nodes ahead
        g.ntab[i + 1] = make_uint4(g.first_row[i], len | ((deg ? deg : 1u) << 24),
                                   (uint32_t)remain_last[i] | (is_sink ? 0x80000000u : 0u) | (reach[i] > POA_RING_SPAN ? 0x40000000u : 0u),
                                   deg <= 1 ? g.preds[pstart] : pstart);
        if (is_sink) g.sinks.push_back(last_row[i]);
    }
    g.longest = longest;
    g.ntab[0] = make_uint4(0u, 1u, (uint32_t)longest, 0u);  // the virtual source: row 0, remain over the source nodes
    g.n_ntab = (uint32_t)g.ntab.size(); g.n_preds = (uint32_t)g.preds.size(); g.n_sinks = (uint32_t)g.sinks.size();
    g.first_row_p = g.first_row.data();
    g.ok = true;
}

template <typename T>
T *pmalloc(size_t n)
{
    return (T *)malloc((n ? n : 1) * sizeof(T));
}

inline char lower(char c) { return (c >= 'A' && c <= 'Z') ? (char)(c + 32) : c; }

template <typename F>
void parallel_for(uint64_t n, F f) { vga_parallel_for(n, f); }

// host: CIGAR / cs / node path of one problem from the raw op stream (reverse order on the device), or copied from the text
// k_poa_text wrote.  `at`: the problem's place in its launch; dev: the graph came from the device store
void poa_post_one(const poa_slot::out_set &S, uint64_t at, poa_item &it, const poa_prep &g, const poa_prob &pb, const poa_view &view, bool dev, bool keep_text)
{
    const poa_out &ho = S.h_outs.p[at];
    if (ho.status == POA_ST_POOL || ho.status == POA_ST_RETRY) return;  // re-run later
    it.ok = ho.status == POA_ST_OK ? 1 : 0;
    it.score = ho.score;
    it.n_cells = ho.cells;
    it.n_vcells = ho.vcells;
    if (!it.ok) return;
    if (S.text && S.h_touts.p[at].flags == 1u) {
        // K4c wrote the fields (vga_poa_text.hpp): they are copied, not derived
        const poa_text_out &t = S.h_touts.p[at];
        const uint32_t *runs = (const uint32_t *)(S.text_p + t.runs_off);
        if (keep_text) {
            it.cs_p = S.text_p + t.cs_off; it.cs_n = t.cs_len;
            it.cigar_p = S.text_p + t.cg_off; it.cigar_n = t.cg_len;
            it.gnodes_p = runs; it.gnodes_n = t.n_runs;
            it.cs.clear(); it.cigar.clear(); it.gnodes.clear();
        } else {
            it.cs.assign(S.text_p + t.cs_off, t.cs_len);
            it.cigar.assign(S.text_p + t.cg_off, t.cg_len);
            it.gnodes.assign(runs, runs + t.n_runs);
        }
        it.rows.clear();
        it.deduped = true;
        it.n_path = t.n_path; it.start_off = t.start_off; it.end_off = t.end_off; it.aligned = t.aligned;
        return;
    }
    const uint8_t *po = S.h_ops.p + pb.ops0;
    const uint32_t *pr = S.h_orow.p + pb.ops0;
    const char *q = view.query;
    // base of graph row r: bases[r - 1] -- the node strings of a host graph, or (device store) the sub-batch's gathered
    // node sequences, which came back with the operations
    const char *bases = dev ? S.h_seq.p + pb.seq0 : view.nodes + view.node_off[0];
    const uint32_t *frow = g.first_row_p;
    const size_t nv = (size_t)g.n_ntab - 1;
    const uint32_t nops = ho.nops;
    // one pass over the operations (stored sink -> source), writing through raw pointers into buffers of the largest
    // possible size: 3 characters per operation for cs ("*ac"), a run of one per operation for the CIGAR ("1M").  Those
    // are scratch of the worker thread; the problem keeps copies of the exact size (the largest possible size is four
    // times what a 10 kbp read uses: 2.4 GB of touched, unused capacity per 10 000 reads, which the process then carries
    // to its exit)
    struct scratch_t { std::vector<char> cs, cg; std::vector<uint32_t> rows; };
    static thread_local scratch_t sc;
    if (sc.cs.size() < 5 + 3 * (size_t)nops + 24) sc.cs.resize(5 + 3 * (size_t)nops + 24 + 4096);
    if (sc.cg.size() < 2 * (size_t)nops + 24) sc.cg.resize(2 * (size_t)nops + 24 + 4096);
    if (sc.rows.size() < nops) sc.rows.resize((size_t)nops + 1024);
    char *const cs0 = sc.cs.data(), *const cg0 = sc.cg.data();
    char *c = cs0, *d = cg0;
    uint32_t *rowp = sc.rows.data();
    memcpy(c, "cs:Z:", 5);
    c += 5;
    auto put_u = [](char *&w, uint64_t v) {
        char t[24];
        int k = 0;
        do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (k) *w++ = t[--k];
    };
    uint64_t eq_run = 0, aligned = 0;
    uint32_t qi = 0, n_rows = 0;
    uint32_t t2 = nops;
    while (t2 > 0) {
        const uint8_t op = po[t2 - 1];
        uint32_t u = t2 - 1;
        while (u > 0 && po[u - 1] == op) u--;
        put_u(d, t2 - u);
        *d++ = op == 0 ? 'M' : (op == 1 ? 'I' : 'D');
        if (op != 0 && eq_run) { *c++ = ':'; put_u(c, eq_run); eq_run = 0; }
        if (op == 0) {
            for (uint32_t x = t2; x > u; x--) {
                const uint32_t r = pr[x - 1];
                const char gb = bases[r - 1], qb = q[qi++];
                rowp[n_rows++] = r;
                if (gb == qb) eq_run++;
                else {
                    if (eq_run) { *c++ = ':'; put_u(c, eq_run); eq_run = 0; }
                    *c++ = '*'; *c++ = lower(gb); *c++ = lower(qb);
                }
            }
            aligned += t2 - u;
        } else if (op == 1) {
            *c++ = '+';
            for (uint32_t x = t2; x > u; x--) *c++ = lower(q[qi++]);
        } else {
            *c++ = '-';
            for (uint32_t x = t2; x > u; x--) {
                const uint32_t r = pr[x - 1];
                rowp[n_rows++] = r;
                *c++ = lower(bases[r - 1]);
            }
        }
        t2 = u;
    }
    if (eq_run) { *c++ = ':'; put_u(c, eq_run); }
    it.cs.assign(cs0, (size_t)(c - cs0));
    it.cigar.assign(cg0, (size_t)(d - cg0));
    it.rows.assign(rowp, rowp + n_rows);
    it.n_path = n_rows;
    it.deduped = false;
    it.aligned = (uint32_t)aligned;
    // rows ascend along the path: merge-walk the node table to label them
    it.gnodes.resize(it.rows.size());
    size_t v = 0;
    for (size_t t = 0; t < it.rows.size(); t++) {
        while (v + 1 < nv && frow[v + 1] <= it.rows[t]) v++;
        it.gnodes[t] = (uint32_t)v;
    }
    if (!it.rows.empty()) {
        it.start_off = it.rows.front() - frow[it.gnodes.front()];
        it.end_off = it.rows.back() - frow[it.gnodes.back()] + 1;
    }
}

// ============================================================================================ one call
// a sub-batch in flight: launch positions [i0, i1) on a slot, its results in the slot's result set `oset`
struct sub_t { uint64_t i0, i1; double raw_est; int slot; int oset; bool general = false; bool arena = false; };
// launch positions still to be enqueued
struct range_t { uint64_t first, second; bool general; bool arena; };
// a sub-batch while it is being put together (poa_call::launch and its stages)
struct launch_t {
    uint64_t i0 = 0, i1 = 0;
    int slot = 0, oset = 0;
    bool general = false, arena = false;
    uint32_t nb = 0;  // problems
    double raw_est = 0;
    uint64_t tot_nodes = 0, tot_preds = 0, tot_sink = 0, tot_q = 0, tot_ops = 0, tot_rows = 0, tot_seq = 0;  // what they take of the slot's buffers
    bool text_on_device = false;
    bool fused = false;       // the DP kernel does the traceback as well
    uint8_t *pool_base = nullptr;  // classic mode: the slot's part of the pool
    std::chrono::steady_clock::time_point t0;
};

// The state of one poa_run call.  poa_run below is the sequence of its stages; the section comments name them.
struct poa_call {
    vga_ctx *const ctx;
    poa_feed &feed;
    const vga_poa_params *const params;
    std::vector<poa_item> &out;
    poa_timing &tm;
    const uint64_t n;
    std::vector<poa_view> &views;
    const poa_switches sw;
    const poa_family family;
    const std::chrono::steady_clock::time_point t_host0 = std::chrono::steady_clock::now();
    vga_trace tr{"poa"};
    poa_ws &W;
    poa_pool pool;
    // The list makers (oplist_makers()) that are on while the graphs are in the device store, with the lists of this call: the list
    // kernel of each runs behind k_poa_text
    struct list_maker {
        const oplist_maker *maker;
        oplist_call *lists;
    };
    std::vector<list_maker> makers;
    uint32_t max_q = 0;
    // ---- plan: node tables, estimates, launch order
    std::vector<poa_prep> G;
    std::vector<poa_prob> probs;
    std::vector<double> est, estw;  // footprint in the pool (bytes) and widest-row estimate (columns) per problem
    std::vector<uint8_t> ready;
    std::vector<uint32_t> order;    // launch positions -> problems; re-runs are appended
    std::vector<uint32_t> ids;
    bool malformed = false, dev_failed = false;
    int dev_rc = VGA_OK;
    poa_probe probe;
    // ---- launches
    int n_slots = 2;
    hipStream_t sarr[POA_SLOTS] = {};
    poa_dev_params P = {};
    hipError_t launch_err = hipSuccess;
    // a sub-batch is closed once it holds this many problems and this many estimated DP cells (or its pool half is full)
    // measured on configs 3-5 (tests/prof_sub_sweep.sh, tests/prof_ab.sh).  Classic mode: 3072..5120 is flat, uncapped
    // loses 40 % on config 5.  Arena mode: launches share the GPU seamlessly, so shorter ones only cost when two of them
    // cannot fill it (1024: -12 % on config 3); 2048 is best on all three.
    uint64_t sub_problems = 4096;
    double sub_cells = 2e9;
    uint64_t in_flight_other = 0;  // problems of the sub-batches on the other streams (they share the GPU with a new launch)
    bool any_fused = false;        // the DP kernel walked the alignments back itself
    int t_total = -1;
    // ---- collection
    int rc_final = VGA_OK;
    std::vector<range_t> todo;      // used as a stack of [begin, end) ranges of launch positions, front = back()
    std::vector<uint32_t> retry;    // problems a specialised DP kernel handed back (POA_ST_RETRY): re-run with the general one
    std::vector<uint32_t> too_big;  // problems chunk mode gave up on twice: classic mode once the chunk-mode launches are done
    std::vector<uint32_t> again;    // ... once: they run again in chunk mode when the others are through (the pool has grown, fewer compete)
    std::vector<uint8_t> gave_up;
    std::vector<sub_t> inflight;
    bool slot_busy[POA_SLOTS] = {};
    uint64_t all_cells = 0, all_vcells = 0, all_rows = 0, all_q = 0, all_ops = 0;
    uint64_t text_bytes = 0;  // what came back over PCIe for the strings and paths: K4c's text, or the raw operations

    poa_call(vga_ctx *c, poa_feed &f, const vga_poa_params *p, std::vector<poa_item> &o, poa_timing &t)
        : ctx(c), feed(f), params(p), out(o), tm(t), n(f.views.size()), views(f.views), sw(poa_read_switches()),
          family(poa_choose_family(*p, sw)), W(poa_ws_of(c)), pool(c, W, sw, tr, n)
    {
        if (!f.dev) return;
        for (const oplist_maker *m : oplist_makers())
            if (oplist_state *s = m->making(c)) makers.push_back({m, &s->lists});
    }

    double ms_since_start() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host0).count(); }
    void chk(hipError_t e) { if (e != hipSuccess && launch_err == hipSuccess) launch_err = e; }
    // chunk-pool mode (k_poa_dp_t5 with its fused traceback; VGA_POA_ARENAS=0 switches it off): every row of a problem must
    // fit a chunk (a multi-predecessor row has four planes), and a state region holds the ring, the scratch rows and a few
    // kept value rows
    bool chunk_pool_wanted() const { return family == POA_FAM_T5 && sw.tb_fused && !sw.arenas_off && 4ull * ((uint64_t)max_q + 8) <= POA_CHUNK; }
    int malformed_error()
    {
        return vga_set_error(ctx, VGA_ERR_ARG, "a POA problem is malformed (no node, empty node, edge with src >= dst, in-degree > 255, or sequence too long)");
    }
    // validate and order
    int validate();
    double est_width(uint64_t p) const;
    void ensure(uint64_t a, uint64_t b);
    int order_problems();
    // size and obtain the pool
    int size_pool();
    int obtain_pool();
    // choose a sub-batch, stage it, launch it
    sub_t launch(uint64_t i0, uint64_t cap, int slot, bool general, bool arena);
    void choose(launch_t &L, uint64_t cap);
    void lay_out(launch_t &L);
    void stage(const launch_t &L);
    void launch_dp(launch_t &L);
    void enqueue_results(const launch_t &L);
    void collect_lists(const list_maker &m, const sub_t &cur, const poa_slot::out_set &S);
    void fill();
    // fetch its text, requeue, post-process, account
    void collect();
    sub_t take_finished();
    bool fetch_text(const sub_t &cur, poa_slot::out_set &S);
    void requeue_handed_back(const sub_t &cur, const poa_slot::out_set &S);
    void post_process(const sub_t &cur, const poa_slot::out_set &S);
    int finish();
    // VGA_TRACE, VGA_POA_DUMP_ROWS
    void trace_setup(const launch_t &L, const char *what) const;
    void trace_shape(const launch_t &L, const poa_shape &sh, double mean_w, double max_w) const;
    void trace_sub_batch(const sub_t &cur, const poa_slot::out_set &S) const;
    void trace_order() const;
    void dump_rows(const sub_t &cur) const;
};

// ---------------------------------------------------------------------------------------- validate and order
int poa_call::validate()
{
    out.assign(n, poa_item());
    tm = poa_timing();
    (void)hipSetDevice(ctx->device);
    if (params->gap_open1 < 0 || params->gap_open1 > 255 || params->gap_open2 < 0 || params->gap_open2 > 255 ||
        params->gap_ext1 < 0 || params->gap_ext2 < 0 || params->gap_open1 + params->gap_ext1 > 255 ||
        params->gap_open2 + params->gap_ext2 > 255)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "gap penalties: open + extend must be in 0..255 (one byte per gap state)");
    if (params->remain_rule != VGA_REMAIN_LONGEST_PATH && params->remain_rule != VGA_REMAIN_FIRST_OUT_EDGE)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_poa_params.remain_rule %d: not one of VGA_REMAIN_*", params->remain_rule);
    if (feed.dev && feed.dev->remain_rule != params->remain_rule)
        return vga_set_error(ctx, VGA_ERR_ARG, "the device subgraph store was built for another remain_rule");
    if (!feed.keep_timers) vga_timers_reset(ctx);
    if (n == 0) return VGA_OK;
    for (uint64_t p = 0; p < n; p++) {
        if (views[p].qlen >= (1u << 24)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "query %llu too long", (unsigned long long)p);
        max_q = std::max(max_q, views[p].qlen);
    }
    // the longest query must fit the LDS of the kernel family that will run
    if (poa_min_lds_bytes(family, poa_lds_cols(max_q)) > POA_LDS_LIMIT)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "query of %u bases does not fit the LDS-resident POA kernel (limit ~280 kbp, ~22 kbp with large gap penalties)", max_q);
    // k_poa_dp_lds hands pool space out in 1 MiB chunks and assumes that a request fits one (k_poa_dp_t4 takes
    // whole chunks for a larger one): their two wide-row scratch rows (8 B per column) and an unbanded direction row with its
    // three predecessor planes (4 B per column) must stay below that
    if (family == POA_FAM_LDS && 8ull * (uint64_t)poa_lds_cols(max_q) > POA_CHUNK)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "query of %u bases: only k_poa_dp_t4 (default penalties range) handles queries beyond ~131 kbp", max_q);
    return VGA_OK;
}

// Mean band width of a problem.  The band of a row spans from the row maxima to the diagonal qlen - remain, so it
// grows with the excess of the longest source-sink path over the query; on 10 kbp reads against DRB1-3123 the mean is
// 2w + 1 + 430 + 0.27 * excess (rms error ~25 %).  Only the pool budget and the launch order depend on it, and the
// budget scale adapts to the measured footprint after every sub-batch.
double poa_call::est_width(uint64_t p) const
{
    const poa_prep &g = G[p];
    const double w = params->wb < 0 ? (double)g.qlen : (double)params->wb + (double)(uint64_t)(params->wf * (double)g.qlen);
    double excess = (double)g.longest - (double)g.qlen;
    if (excess < 0) excess = -excess;
    return std::min((double)g.qlen + 1.0, 2.0 * w + 1.0 + 430.0 + 0.3 * excess);
}

// prepares launch positions [a, b): the caller's part (subgraphs), then node tables and estimates
void poa_call::ensure(uint64_t a, uint64_t b)
{
    ids.clear();
    for (uint64_t i = a; i < b && i < order.size(); i++)
        if (!ready[order[i]]) ids.push_back(order[i]);
    if (ids.empty()) return;
    if (feed.prepare) feed.prepare(ids.data(), ids.size());
    if (feed.dev && !feed.dev->part[1].ready) {
        // the second part of the device store is built when a problem of it is first needed -- by then the first DP
        // launch is on the GPU and the subgraph kernels run beside it
        bool need = false;
        for (uint32_t p : ids) need |= p >= feed.dev->split;
        if (need) {
            if ((dev_rc = feed.dev_rest()) != VGA_OK) { dev_failed = true; return; }
            // the caller may have re-ordered the second part (none of it has been staged): take its order over, and
            // prepare what now stands at the positions asked for
            if (feed.order) {
                for (uint64_t i = feed.dev->split; i < n; i++) order[i] = feed.order[i];
                ids.clear();
                for (uint64_t i = a; i < b && i < order.size(); i++)
                    if (!ready[order[i]]) ids.push_back(order[i]);
            }
        }
    }
    parallel_for(ids.size(), [&](uint64_t t) {
        const uint32_t p = ids[t];
        if (feed.dev) {
            // the device store holds the graph: only its sizes come to the host
            const sg_sum &sm = feed.dev->sum[p];
            poa_prep &g = G[p];
            g.ok = !(sm.flags & 1u) && sm.n_nodes > 0 && views[p].qlen < (1u << 24);
            g.N = sm.N; g.qlen = views[p].qlen; g.longest = (int32_t)sm.longest; g.life = sm.life;
            g.n_ntab = sm.n_nodes + 1; g.n_preds = sm.n_preds; g.n_sinks = sm.n_sinks;
            g.first_row_p = feed.dev->of(p).h_first_row + feed.dev->off[p].node0;
        } else
            poa_prepare(views[p], G[p], params->remain_rule == VGA_REMAIN_FIRST_OUT_EDGE);
        // footprint in the pool: a direction byte per cell plus the value-row ring
        if (G[p].ok) {
            estw[p] = est_width(p);
            est[p] = (double)G[p].N * estw[p] * 1.15 + (double)(G[p].life + 1) * 6.0 * ((double)G[p].qlen + 8.0) + 2.0 * (double)POA_CHUNK;
        }
        ready[p] = 1;
    });
    for (uint32_t p : ids)
        if (!G[p].ok) malformed = true;
}

// ---- launch order and lazy preparation.  The caller may hand the problems over lazily (feed.prepare fills the graph
// part of a view on request): then the order is fixed up front from a cheap size proxy and a sub-batch's subgraphs
// and node tables are built by the host threads while earlier sub-batches are on the GPU.  Without a proxy every
// problem is prepared first and the order is by the footprint estimate (longest first).
int poa_call::order_problems()
{
    G.resize(n);
    probs.resize(n);
    est.assign(n, 0.0);
    estw.assign(n, 0.0);
    ready.assign(n, 0);
    order.resize(n);
    for (uint64_t p = 0; p < n; p++) order[p] = (uint32_t)p;
    if (feed.order) {
        for (uint64_t p = 0; p < n; p++) order[p] = feed.order[p];
    } else if (feed.proxy) {
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return feed.proxy[x] > feed.proxy[y]; });
    } else {
        ensure(0, n);
        if (!malformed) std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return est[x] > est[y]; });
    }
    if (malformed) return malformed_error();
    tr.mark("order (+ node tables when not lazy)");
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- size and obtain the pool
// the footprint probe, this context's share of the GPU, and how many launches will be in flight
int poa_call::size_pool()
{
    // (poa_feed::keep_text: what the previous call's items pointed into has been read by now)
    for (auto &hb : W.text_live) W.text_free.push_back(std::move(hb));
    W.text_live.clear();
    W.join_preparer();
    VGA_HIP_CHECK(ctx, W.h_next.reserve(POA_SLOTS));
    VGA_HIP_CHECK(ctx, W.d_next.reserve(POA_SLOTS));
    // ---- footprint probe: the first prepared problems (the largest, in launch order)
    probe.n = std::min<uint64_t>(n, 512);
    ensure(0, probe.n);
    if (malformed) return malformed_error();
    // the very long problems of the call (a launch of their own: poa_feed::klass) stand at the head of the order, inside the
    // probe: what the probed ones take is scaled up to all of them, and the mean of the rest is taken apart
    double bulk_sum = 0;
    uint64_t long_cnt = 0, bulk_cnt = 0;
    for (uint64_t i = 0; i < probe.n; i++) {
        const double e = est[order[i]];
        probe.sum += e;
        probe.big = std::max(probe.big, e);
        if (feed.klass && feed.klass[order[i]]) { probe.long_sum += e; long_cnt++; }
        else { bulk_sum += e; bulk_cnt++; }
    }
    probe.mean = probe.sum / (double)probe.n;
    if (feed.klass)
        for (uint64_t p = 0; p < n; p++) probe.long_all += feed.klass[p] != 0;
    if (long_cnt && probe.long_all > long_cnt) probe.long_sum *= (double)probe.long_all / (double)long_cnt;
    probe.bulk_mean = bulk_cnt ? bulk_sum / (double)bulk_cnt : probe.mean;
    const int rc = pool.measure();
    if (rc != VGA_OK) return rc;
    pool.state_size = poa_state_size(max_q);
    pool.probe_mean = probe.mean;
    pool.classic_need = probe.mean * (double)n;
    // Two sub-batches are in flight at any time, one per stream, each carving from its own half of the pool: while one
    // drains (its last workgroups, then the latency-bound traceback and the copies back) the other one's
    // workgroups fill the CUs.
    // classic mode: two sub-batches in flight (three are no faster, four overflow their pool quarters).  Arena mode: the
    // pool is not split and a third slot only costs staging buffers (round 1 ran three throughout: +1.4 % on config 3 with
    // first-in-first-out completion; with launches handled in the order they finish, round 2, that reversed).
    // Two launches in flight keep the GPU full when the problems of a call are of one kind (config 3: 8 410-8 460 reads/s
    // with two, 8 100-8 370 with three, same-box); when the call holds very long problems (poa_feed::klass: config 4's
    // 100 000-row chains) their launch occupies a slot for a second, and a third slot keeps two for everything else
    // (config 4: 7 900 reads/s with three, 5 900 with two)
    const bool arena_wanted = chunk_pool_wanted();
    n_slots = arena_wanted ? (probe.long_all || !feed.klass ? 3 : 2) : 2;
    // ... and when the call's problems are narrow-band (k_poa_dp_t6's launches: 2 048 single-wave workgroups each, two of them are
    // exactly the GPU's 4 096 wave slots): while the first of two launches drains, its freed slots stay empty until it has ended
    // and the next one is staged -- with a third launch in flight they are taken at once (config 5: 58 200 -> 66 400 reads/s,
    // same box; four: 62 700; config 3, wide bands: 9 410 with two, 9 330 with three)
    double wsum = 0;
    for (uint64_t i = 0; i < probe.n; i++) wsum += estw[order[i]];
    if (arena_wanted && wsum / (double)probe.n <= 800.0) n_slots = 3;
    if (sw.has_slots) n_slots = std::max(1, std::min(POA_SLOTS, sw.slots));
    pool.n_slots = n_slots;
    sarr[0] = ctx->stream;
    for (int i = 1; i < n_slots; i++) {
        if (!W.extra[i]) VGA_HIP_CHECK(ctx, hipStreamCreateWithFlags(&W.extra[i], hipStreamNonBlocking));
        sarr[i] = W.extra[i];
    }
    return VGA_OK;
}

// chunk-pool mode or, for the whole call, classic mode
int poa_call::obtain_pool()
{
    int rc = VGA_OK;
    if (chunk_pool_wanted() && (rc = pool.obtain_chunks(probe, ctx->stream)) != VGA_OK) return rc;
    pool.start_keeper();
    if (!pool.n_arenas && (rc = pool.ensure_classic()) != VGA_OK) return rc;
    tr.mark("pool");
    pool.trace_mode();
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- choose, stage, launch
// the problems of a sub-batch that starts at launch position L.i0 and ends at cap at the latest
void poa_call::choose(launch_t &L, uint64_t cap)
{
    const double budget = (double)pool.half_pool * 0.92;
    double used_est = 0, cells_est = 0;
    const uint64_t i0 = L.i0;
    uint64_t i1 = i0;
    // (device store: a launch gathers from one part of it)
    if (feed.dev && feed.dev->split > i0 && feed.dev->split < cap) cap = feed.dev->split;
    while (i1 < cap) {
        // (device store: a problem's preparation is a copy of its sizes -- a whole launch's worth in one fan-out; 256 at a time
        // cost eight thread fan-outs per launch, 6-7 ms before each of a call's first two launches with the GPU idle)
        if (!ready[order[i1]]) ensure(i1, std::min<uint64_t>(cap, i1 + (feed.dev ? 4096 : 256)));
        if (malformed || dev_failed) break;
        const double e = est[order[i1]] * W.pool_scale + 3.0 * (double)POA_CHUNK;
        if (!L.arena && i1 > i0 && used_est + e > budget) break;
        // the pool is not the only reason to cut: the host work either side of a sub-batch (subgraphs and node
        // tables before, CIGAR / cs strings after) only overlaps with the GPU when there are several sub-batches
        if (i1 - i0 >= sub_problems && cells_est >= sub_cells) break;
        // very long problems (a chain that spans 100 kbp of the linearisation: 100 000 sequential rows) are a launch of
        // their own: they decide how long the whole call takes, so they get the largest workgroup and window (poa_choose_shape)
        if (feed.klass && i1 > i0 && feed.klass[order[i1]] != feed.klass[order[i0]]) break;
        used_est += e;
        // (arena mode: problems that are sent on to the classic pass take no arena and do not count)
        L.raw_est += est[order[i1]];
        cells_est += (double)G[order[i1]].N * estw[order[i1]];
        i1++;
    }
    L.i1 = i1;
}

// offsets of the sub-batch's problems inside the slot's buffers, and the buffers themselves
void poa_call::lay_out(launch_t &L)
{
    poa_slot &S = W.slot[L.slot];
    L.oset = (int)(S.uses++ & 1u);
    poa_slot::out_set &O = S.outs[L.oset];
    const uint32_t nb = L.nb = (uint32_t)(L.i1 - L.i0);
    for (uint64_t i = L.i0; i < L.i1; i++) {
        const uint32_t p = order[i];
        poa_prob &pb = probs[p];
        const poa_prep &g = G[p];
        pb.node0 = L.tot_nodes; pb.pred0 = L.tot_preds; pb.sink0 = L.tot_sink; pb.q0 = L.tot_q; pb.ops0 = L.tot_ops; pb.row0 = L.tot_rows;
        pb.seq0 = L.tot_seq;
        pb.n_sink = g.n_sinks; pb.qlen = g.qlen; pb.N = g.N; pb.n_nodes = g.n_ntab; pb.ring_rows = g.life + 1;
        pb.flags = 0u;  // (bit 0: not for the chunk pool -- every problem of a chunk-mode call fits it by construction)
        pb.pad = 0;
        pb.w = params->wb < 0 ? g.qlen : (uint32_t)((int64_t)params->wb + (int64_t)(params->wf * (double)g.qlen));
        L.tot_nodes += g.n_ntab;
        L.tot_preds += g.n_preds;
        L.tot_sink += g.n_sinks;
        L.tot_q += g.qlen;
        L.tot_ops += (uint64_t)g.N + g.qlen + 2;
        L.tot_rows += (uint64_t)g.N + 1;
        L.tot_seq += ((uint64_t)g.N + 3) & ~3ull;
        out[p].n_rows = g.N;
    }
    const bool dev = feed.dev != nullptr;
    // cs / CIGAR / node path on the device (K4c) when the caller does not need the per-base rows; VGA_POA_TEXT=host keeps the host's
    L.text_on_device = dev && !feed.want_rows && !sw.text_host;
    chk(S.h_probs.reserve(nb));
    if (dev) chk(S.h_ids.reserve(2 * (size_t)nb));
    else {
        chk(S.h_ntab.reserve(L.tot_nodes)); chk(S.h_seq32.reserve(L.tot_seq / 4 + 1));
        chk(S.h_preds.reserve(L.tot_preds + 1)); chk(S.h_sink.reserve(L.tot_sink + 1)); chk(S.h_q.reserve(L.tot_q + 1));
    }
    chk(O.h_outs.reserve(nb));
    if (!L.text_on_device) {  // (K4c: the operations stay on the device; the fallback reserves these when it needs them)
        chk(O.h_ops.reserve(L.tot_ops)); chk(O.h_orow.reserve(L.tot_ops));
        if (dev) chk(O.h_seq.reserve(L.tot_seq + 4));
    }
    chk(S.d_probs.reserve(nb)); chk(S.d_ntab.reserve(L.tot_nodes)); chk(S.d_seq32.reserve(L.tot_seq / 4 + 1));
    chk(S.d_preds.reserve(L.tot_preds + 1)); chk(S.d_sink.reserve(L.tot_sink + 1)); chk(S.d_q.reserve(L.tot_q + 1));
    chk(S.d_rows.reserve(L.tot_rows)); chk(S.d_outs.reserve(nb)); chk(S.d_ops.reserve(L.tot_ops)); chk(S.d_orow.reserve(L.tot_ops));
    if (dev) chk(S.d_ids.reserve(2 * (size_t)nb));
}

// the graphs of the sub-batch into the slot's device buffers
void poa_call::stage(const launch_t &L)
{
    hipStream_t st = sarr[L.slot];
    poa_slot &S = W.slot[L.slot];
    const uint32_t nb = L.nb;
    const uint64_t i0 = L.i0;
    if (feed.dev) {
        // the graphs are in the device store: one workgroup per problem copies its pieces into this slot's buffers
        for (uint32_t t = 0; t < nb; t++) {
            const uint32_t p = order[i0 + t];
            S.h_probs.p[t] = probs[p]; S.h_ids.p[2 * t] = p; S.h_ids.p[2 * t + 1] = G[p].n_preds;
        }
        chk(hipMemcpyAsync(S.d_probs.p, S.h_probs.p, nb * sizeof(poa_prob), hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_ids.p, S.h_ids.p, 2 * (size_t)nb * sizeof(uint32_t), hipMemcpyHostToDevice, st));
        const sg_store &D = *feed.dev;
        const sg_gather_src g0 = {D.part[0].d_ntab, D.part[0].d_preds, D.part[0].d_sinks, D.part[0].d_seq, (uint32_t)D.part[0].p0};
        const sg_gather_src g1 = {D.part[1].d_ntab, D.part[1].d_preds, D.part[1].d_sinks, D.part[1].d_seq, (uint32_t)D.part[1].p0};
        chk(poa_launch_gather(st, nb, S.d_ids.p, S.d_probs.p, D.d_off, (uint32_t)D.split, g0, g1, D.d_reads, S.d_ntab.p, S.d_preds.p, S.d_sink.p,
                              (char *)S.d_seq32.p, S.d_q.p));
    } else {
        parallel_for(nb, [&](uint64_t t) {
            const uint32_t p = order[i0 + t];
            const poa_prob &pb = probs[p];
            const poa_prep &g = G[p];
            S.h_probs.p[t] = pb;
            memcpy(S.h_ntab.p + pb.node0, g.ntab.data(), g.ntab.size() * sizeof(uint4));
            if (!g.preds.empty()) memcpy(S.h_preds.p + pb.pred0, g.preds.data(), g.preds.size() * 4);
            if (!g.sinks.empty()) memcpy(S.h_sink.p + pb.sink0, g.sinks.data(), g.sinks.size() * 4);
            // node strings of one problem are contiguous in the view
            memcpy((char *)S.h_seq32.p + pb.seq0, views[p].nodes + views[p].node_off[0], g.N);
            if (g.qlen) memcpy(S.h_q.p + pb.q0, views[p].query, g.qlen);
        });
        chk(hipMemcpyAsync(S.d_probs.p, S.h_probs.p, nb * sizeof(poa_prob), hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_ntab.p, S.h_ntab.p, L.tot_nodes * sizeof(uint4), hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_seq32.p, S.h_seq32.p, L.tot_seq, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_preds.p, S.h_preds.p, L.tot_preds * 4, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_sink.p, S.h_sink.p, L.tot_sink * 4, hipMemcpyHostToDevice, st));
        chk(hipMemcpyAsync(S.d_q.p, S.h_q.p, L.tot_q, hipMemcpyHostToDevice, st));
    }
    chk(hipMemsetAsync(W.d_next.p + L.slot, 0, sizeof(unsigned long long), st));
}

static poa_launch_bufs bufs_of(const poa_slot &S)
{
    return {S.d_probs.p, S.d_q.p, S.d_ntab.p, S.d_seq32.p, S.d_preds.p, S.d_sink.p, S.d_rows.p, S.d_outs.p, S.d_ops.p, S.d_orow.p};
}

// the DP kernel of the sub-batch in the shape poa_choose_shape gives it, then the traceback when the DP kernel does not walk
void poa_call::launch_dp(launch_t &L)
{
    hipStream_t st = sarr[L.slot];
    poa_slot &S = W.slot[L.slot];
    const int t_dp = vga_timer_begin(ctx, "poa_band_dp", 0, st);
    poa_shape_in in;
    double sum_w = 0;
    for (uint64_t i = L.i0; i < L.i1; i++) {
        in.max_q = std::max(in.max_q, G[order[i]].qlen);
        in.max_w = std::max(in.max_w, estw[order[i]]);
        sum_w += estw[order[i]];
    }
    in.mean_w = sum_w / (double)L.nb;
    in.left = order.size() - L.i0;
    in.in_flight = in_flight_other;
    in.n_cu = (uint32_t)ctx->n_cu;
    in.giant = feed.klass && feed.klass[order[L.i0]];
    in.general = L.general;
    in.arena = L.arena;
    in.fused = L.fused = family != POA_FAM_LDS && sw.tb_fused;
    in.default_penalties = P.o1 == 4 && P.e1 == 2 && P.o2 == 24 && P.e2 == 1;
    in.family = family;
    any_fused = any_fused || L.fused;
    const poa_shape sh = poa_choose_shape(in, sw);
    trace_shape(L, sh, in.mean_w, in.max_w);
    L.pool_base = L.arena ? nullptr : W.classic + (uint64_t)L.slot * pool.half_pool;
    poa_chunk_pool cp_arg = pool.CP;
    if (!L.arena) cp_arg.n_slots = 0;
    const poa_t5_args a = {S.d_probs.p, S.d_q.p, S.d_ntab.p, S.d_seq32.p, S.d_preds.p, S.d_rows.p, L.pool_base, W.d_next.p + L.slot, pool.half_pool,
                           S.d_outs.p, (L.fused ? S.d_ops.p : nullptr), (L.fused ? S.d_orow.p : nullptr), cp_arg, sh.lds_cols, sh.hg_cols, sh.win_mask, P,
                           (in.giant && sw.giant_prio) ? 1u : 0u};
    chk(poa_launch_dp(ctx->device, st, sh, L.nb, a, S.d_sink.p));
    vga_timer_end(ctx, t_dp);
    const int t_tb = vga_timer_begin(ctx, "poa_traceback", 0, st);
    // (fused: the DP kernel's first wave already walked each problem back)
    if (!L.fused) poa_launch_traceback(st, sh.kernel, L.nb, bufs_of(S), L.pool_base);
    vga_timer_end(ctx, t_tb);
}

// the copies back, and k_poa_text before them when the strings are written on the device
void poa_call::enqueue_results(const launch_t &L)
{
    hipStream_t st = sarr[L.slot];
    poa_slot &S = W.slot[L.slot];
    poa_slot::out_set &O = S.outs[L.oset];
    const uint32_t nb = L.nb;
    chk(hipMemcpyAsync(O.h_outs.p, S.d_outs.p, nb * sizeof(poa_out), hipMemcpyDeviceToHost, st));
    chk(hipMemcpyAsync(W.h_next.p + L.slot, W.d_next.p + L.slot, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    O.text = L.text_on_device;
    O.tot_ops = L.tot_ops; O.tot_seq = L.tot_seq;
    if (L.text_on_device) {
        // K4c: the strings and the node path are written where the operations are (vga_poa_text.hpp); what crosses PCIe now is a
        // record per problem and the counter of the arena -- the text itself follows when the host knows how much there is
        uint64_t arena = std::min<uint64_t>(2ull * L.tot_ops + 64ull * nb + 4096ull, 0xF0000000ull);
        if (sw.has_text_arena) arena = std::min<uint64_t>(arena, sw.text_arena);  // (testing: the overflow path)
        chk(S.d_text.reserve(arena + 16)); chk(S.d_touts.reserve(nb)); chk(S.d_tcur.reserve(1));
        chk(O.h_touts.reserve(nb)); chk(O.h_tcur.reserve(1));
        if (launch_err == hipSuccess) {
            const int t_tx = vga_timer_begin(ctx, "poa_text", 0, st);
            chk(hipMemsetAsync(S.d_tcur.p, 0, sizeof(unsigned long long), st));
            chk(poa_launch_text(st, nb, bufs_of(S), S.d_text.p, (uint32_t)arena, S.d_tcur.p, S.d_touts.p));
            vga_timer_end(ctx, t_tx);
            chk(hipMemcpyAsync(O.h_touts.p, S.d_touts.p, nb * sizeof(poa_text_out), hipMemcpyDeviceToHost, st));
            chk(hipMemcpyAsync(O.h_tcur.p, S.d_tcur.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        }
    } else {
        chk(hipMemcpyAsync(O.h_ops.p, S.d_ops.p, L.tot_ops, hipMemcpyDeviceToHost, st));
        chk(hipMemcpyAsync(O.h_orow.p, S.d_orow.p, L.tot_ops * 4, hipMemcpyDeviceToHost, st));
        // (device store: the cs strings need the graph bases of the aligned rows -- the gathered node sequences come back too,
        // 17 KB per problem, instead of a handle lookup per aligned base)
        if (feed.dev) chk(hipMemcpyAsync(O.h_seq.p, S.d_seq32.p, L.tot_seq, hipMemcpyDeviceToHost, st));
    }
    // coverage's run list and the pileup's list of every problem, while its operations are in the slot (the refill recycles them)
    for (const list_maker &m : makers)
        if (launch_err == hipSuccess) chk(m.maker->enqueue(ctx, *m.lists, {st, L.slot, L.oset, nb, bufs_of(S), S.d_ids.p, *feed.dev}));
}

// stage, upload and enqueue DP + traceback + result copies of a sub-batch that starts at launch position i0 and ends
// at cap at the latest; an empty sub-batch (i1 == i0) says that nothing was launched
sub_t poa_call::launch(uint64_t i0, uint64_t cap, int slot, bool general, bool arena)
{
    const sub_t none = {i0, i0, 0.0, slot, 0};
    if (!arena) {
        const int rcc = pool.ensure_classic();
        if (rcc != VGA_OK) { dev_failed = true; dev_rc = rcc; return none; }
    }
    launch_t L;
    L.i0 = i0; L.slot = slot; L.general = general; L.arena = arena;
    L.t0 = std::chrono::steady_clock::now();
    if (arena && launch_err == hipSuccess) launch_err = pool.list_new_segments();
    trace_setup(L, "free lists looked after");
    choose(L, cap);
    trace_setup(L, "problems chosen (and prepared)");
    if (malformed || dev_failed || L.i1 == L.i0) return none;
    lay_out(L);
    if (launch_err != hipSuccess) return none;
    trace_setup(L, "buffers reserved");
    stage(L);
    trace_setup(L, "graphs staged");
    launch_dp(L);
    enqueue_results(L);
    return {i0, L.i1, L.raw_est, slot, L.oset, false, arena};
}

void poa_call::fill()
{
    while ((int)inflight.size() < n_slots && !todo.empty() && !malformed && !dev_failed && launch_err == hipSuccess) {
        int slot = 0;
        while (slot_busy[slot]) slot++;
        auto &seg = todo.back();
        // arena launches use the whole pool, classic ones its per-slot segments: never both at a time
        if (!inflight.empty() && inflight.front().arena != seg.arena) break;
        in_flight_other = 0;
        for (const sub_t &o : inflight) in_flight_other += o.i1 - o.i0;
        sub_t sb = launch(seg.first, seg.second, slot, seg.general, seg.arena);
        sb.general = seg.general;
        if (sb.i1 == sb.i0) break;
        if (sb.i1 >= seg.second) todo.pop_back();
        else seg.first = sb.i1;
        slot_busy[slot] = true;
        inflight.push_back(sb);
    }
}

// ---------------------------------------------------------------------------------------- collect
// the launch that finishes first is handled first: a launch of long problems (they come first in the order) must
// not keep the slots of the shorter ones behind it from being refilled
sub_t poa_call::take_finished()
{
    size_t pick = 0;
    if (inflight.size() > 1) {
        for (bool found = false; !found;) {
            for (size_t q = 0; q < inflight.size() && !found; q++) {
                const hipError_t qe = hipStreamQuery(sarr[inflight[q].slot]);
                if (qe != hipErrorNotReady) { pick = q; found = true; }  // finished (or failed: the synchronize that follows reports it)
            }
            if (!found) std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
    }
    const sub_t cur = inflight[pick];
    inflight.erase(inflight.begin() + (long)pick);
    return cur;
}

// K4c, second half: the text the kernel wrote (its length is known now); problems that found the arena full fall back
// to the operations, which are still on the device.  False: a HIP call failed (launch_err says which)
bool poa_call::fetch_text(const sub_t &cur, poa_slot::out_set &S)
{
    if (!S.text) {
        text_bytes += 5 * S.tot_ops + (feed.dev ? S.tot_seq : 0);
        return true;
    }
    hipStream_t st = sarr[cur.slot];
    poa_slot &SL = W.slot[cur.slot];
    const uint64_t used = std::min<uint64_t>(S.h_tcur.p[0], SL.d_text.cap);
    uint64_t no_text = 0;  // problems that found the arena full
    for (uint64_t i = cur.i0; i < cur.i1; i++) no_text += S.h_touts.p[i - cur.i0].flags == 2u ? 1u : 0u;
    bool overflow = no_text != 0;
    // (a problem whose run list or pileup list found no room is served from the operations too)
    for (const list_maker &m : makers)
        for (uint64_t i = cur.i0; i < cur.i1; i++) overflow = overflow || (m.lists->launch_recs(cur.slot, cur.oset)[i - cur.i0].flags & 3u) == 2u;
    hipError_t ce = hipSuccess;
    if (feed.keep_text) {
        // a buffer of the context's that holds the text: the smallest free one that fits, else the largest free one grows
        size_t pickb = W.text_free.size(), big = W.text_free.size();
        for (size_t k = 0; k < W.text_free.size(); k++) {
            if (W.text_free[k]->cap >= used + 16 && (pickb == W.text_free.size() || W.text_free[k]->cap < W.text_free[pickb]->cap)) pickb = k;
            if (big == W.text_free.size() || W.text_free[k]->cap > W.text_free[big]->cap) big = k;
        }
        if (pickb == W.text_free.size()) pickb = big;
        std::unique_ptr<vga_hbuf<char>> hb;
        if (pickb < W.text_free.size()) { hb = std::move(W.text_free[pickb]); W.text_free.erase(W.text_free.begin() + (long)pickb); }
        else hb.reset(new vga_hbuf<char>());
        ce = hb->reserve(used + 16);
        S.text_p = hb->p;
        W.text_live.push_back(std::move(hb));
    } else {
        ce = S.h_text.reserve(used + 16);
        S.text_p = S.h_text.p;
    }
    if (ce == hipSuccess && used) {
        void *hd = nullptr;
        if (!sw.text_memcpy && hipHostGetDevicePointer(&hd, S.text_p, 0) == hipSuccess && hd) {
            // (both buffers are 16-byte aligned and hold 16 bytes of slack)
            ce = poa_launch_text_to_host(st, (const uint4 *)SL.d_text.p, (uint4 *)hd, (used + 15) / 16);
        } else {
            (void)hipGetLastError();
            ce = hipMemcpyAsync(S.text_p, SL.d_text.p, used, hipMemcpyDeviceToHost, st);
        }
    }
    if (ce == hipSuccess && overflow) {
        if (tr.on && no_text) fprintf(stderr, "[vga-trace] poa:   the text arena was too small for %llu of %llu problems: their operations come back\n",
                                      (unsigned long long)no_text, (unsigned long long)(cur.i1 - cur.i0));
        if (tr.on && !no_text) fprintf(stderr, "[vga-trace] poa:   some run or pileup lists found no room: the operations come back\n");
        ce = S.h_ops.reserve(S.tot_ops);
        if (ce == hipSuccess) ce = S.h_orow.reserve(S.tot_ops);
        if (ce == hipSuccess) ce = S.h_seq.reserve(S.tot_seq + 4);
        if (ce == hipSuccess) ce = hipMemcpyAsync(S.h_ops.p, SL.d_ops.p, S.tot_ops, hipMemcpyDeviceToHost, st);
        if (ce == hipSuccess) ce = hipMemcpyAsync(S.h_orow.p, SL.d_orow.p, S.tot_ops * 4, hipMemcpyDeviceToHost, st);
        if (ce == hipSuccess) ce = hipMemcpyAsync(S.h_seq.p, SL.d_seq32.p, S.tot_seq, hipMemcpyDeviceToHost, st);
    }
    const auto t_tx0 = std::chrono::steady_clock::now();
    if (ce == hipSuccess) ce = hipStreamSynchronize(st);
    if (ce != hipSuccess) { launch_err = ce; return false; }
    if (tr.on) fprintf(stderr, "[vga-trace] poa:   text of the sub-batch: %.1f MB copied back in %.2f ms\n", (double)used / 1e6,
                       std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tx0).count());
    text_bytes += used + (cur.i1 - cur.i0) * sizeof(poa_text_out);
    if (overflow) text_bytes += 5 * S.tot_ops + S.tot_seq;
    return true;
}

// what a launch did not finish goes back on the stack: POA_ST_RETRY to the general kernel at once, and, once nothing else is
// left, the problems that gave up waiting for chunks -- a second chunk-mode pass, then the classic pass
void poa_call::requeue_handed_back(const sub_t &cur, const poa_slot::out_set &S)
{
    // problems the 16-bit kernel stopped (a score near the int16 range) run again with 32-bit words
    for (uint64_t i = cur.i0; i < cur.i1; i++)
        if (S.h_outs.p[i - cur.i0].status == POA_ST_RETRY) retry.push_back(order[i]);
    if (!retry.empty()) {
        // at once, beside the launches that are still to come: a pass of its own at the end would run for as long as its
        // longest problem has rows with most of the GPU idle (config 5, first build of k_poa_dp_t6: 45 ms of a 170 ms call)
        const uint64_t a = order.size();
        for (uint32_t p : retry) order.push_back(p);
        if (tr.on) fprintf(stderr, "[vga-trace] poa: %zu problems handed back by the specialised DP kernel: re-run with the general one\n", retry.size());
        retry.clear();
        todo.push_back({a, order.size(), true, pool.n_arenas != 0});
    }
    if (todo.empty() && inflight.empty() && !again.empty()) {
        const uint64_t a = order.size();
        for (uint32_t p : again) order.push_back(p);
        if (tr.on) fprintf(stderr, "[vga-trace] poa: %zu problems gave up waiting for chunks: they run again\n", again.size());
        again.clear();
        todo.push_back({a, order.size(), cur.general, true});
    }
    if (todo.empty() && inflight.empty() && !too_big.empty()) {
        pool.classic_need = 0;
        for (uint32_t p : too_big) pool.classic_need += est[p];
        const uint64_t a = order.size();
        for (uint32_t p : too_big) order.push_back(p);
        if (tr.on) fprintf(stderr, "[vga-trace] poa: %zu problems gave up waiting for chunks (or need more contiguous state than a region holds): classic pass\n", too_big.size());
        too_big.clear();
        todo.push_back({a, order.size(), cur.general, false});
    }
}

// the list records of a finished sub-batch join the call's, for one maker; a list that found no room in the buffer is built here,
// from what fetch_text brought back (the operations and the gathered node sequences; the query is the problem's view of the read)
void poa_call::collect_lists(const list_maker &m, const sub_t &cur, const poa_slot::out_set &S)
{
    const oplist_rec *recs = m.lists->launch_recs(cur.slot, cur.oset);
    for (uint64_t i = cur.i0; i < cur.i1; i++) {
        const uint32_t p = order[i];
        const poa_out &ho = S.h_outs.p[i - cur.i0];
        if (ho.status != POA_ST_OK) continue;
        const oplist_rec &r = recs[i - cur.i0];
        if ((r.flags & 3u) != 2u) { m.lists->keep(p, r); continue; }
        if (tr.on) fprintf(stderr, "[vga-trace] poa:   problem %u: no room for its %s, built from the operations\n", p, m.maker->text.list);
        m.maker->keep_from_ops(*m.lists, p, {S.h_ops.p + probs[p].ops0, S.h_orow.p + probs[p].ops0, ho.nops, G[p].first_row_p, G[p].n_ntab - 1, probs[p].N,
                                      feed.dev->of(p).h_handles + feed.dev->off[p].node0, ctx->index.node_start.data(), S.h_seq.p + probs[p].seq0,
                                      views[p].query});
    }
}

// CIGAR / cs strings / node paths of a finished sub-batch on the host threads, and its share of the call's totals
void poa_call::post_process(const sub_t &cur, const poa_slot::out_set &S)
{
    const uint64_t a0 = cur.i0, cnt = cur.i1 - cur.i0;
    const auto t_post0 = std::chrono::steady_clock::now();
    parallel_for(cnt, [&](uint64_t t) {
        const uint32_t p = order[a0 + t];
        poa_post_one(S, t, out[p], G[p], probs[p], views[p], feed.dev != nullptr, feed.keep_text);
    });
    if (tr.on)
        fprintf(stderr, "[vga-trace] poa:   CIGAR / cs strings of sub-batch [%llu, %llu): %.1f ms on the host, %zu launches in flight meanwhile, at %.1f ms\n",
                (unsigned long long)cur.i0, (unsigned long long)cur.i1, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_post0).count(),
                inflight.size(), ms_since_start());
    for (uint64_t i = cur.i0; i < cur.i1; i++) {
        const poa_out &ho = S.h_outs.p[i - cur.i0];
        if (ho.status == POA_ST_POOL || ho.status == POA_ST_RETRY) continue;
        all_cells += ho.cells; all_vcells += ho.vcells; all_ops += ho.nops;
        all_rows += G[order[i]].N; all_q += G[order[i]].qlen;
    }
}

// Software pipeline.  `todo` holds the launch-order ranges still to be enqueued (a sub-batch that overflowed its pool
// half goes back to the front); up to n_slots sub-batches are in flight, one per stream.  While the GPU works on them the
// host threads prepare the problems of the next sub-batch (the caller's subgraphs, node tables) and turn the op
// streams of the sub-batch that just finished into CIGAR / cs strings.
void poa_call::collect()
{
    P.match = params->match; P.mismatch = params->mismatch; P.o1 = params->gap_open1; P.e1 = params->gap_ext1;
    P.o2 = params->gap_open2; P.e2 = params->gap_ext2; P.banded = params->wb >= 0;
    t_total = vga_timer_begin(ctx, "poa_total", 0);
    sub_problems = pool.n_arenas ? 2048 : 4096;
    if (sw.has_sub) sub_problems = std::max<uint64_t>(1, sw.sub);
    todo.push_back({0, n, false, pool.n_arenas != 0});
    gave_up.assign(n, 0);
    fill();
    while (!inflight.empty()) {
        // look ahead: prepare the problems the next launch will start with while the GPU is busy
        if (!todo.empty()) ensure(todo.back().first, std::min<uint64_t>(todo.back().second, todo.back().first + 1536));
        const sub_t cur = take_finished();
        const hipError_t se = hipStreamSynchronize(sarr[cur.slot]);
        if (se != hipSuccess) { launch_err = se; break; }  // (finish drains every stream)
        if (tr.on) fprintf(stderr, "[vga-trace] poa: (at %.1f ms) the launch of [%llu, %llu) has finished\n", ms_since_start(), (unsigned long long)cur.i0, (unsigned long long)cur.i1);
        poa_slot::out_set &S = W.slot[cur.slot].outs[cur.oset];
        if (launch_err != hipSuccess) break;
        if (!fetch_text(cur, S)) break;
        for (const list_maker &m : makers) collect_lists(m, cur, S);
        bool pool_fail = false;
        for (uint64_t i = cur.i0; i < cur.i1; i++)
            if (S.h_outs.p[i - cur.i0].status == POA_ST_POOL) {
                if (cur.arena) {
                    if (gave_up[order[i]]++ == 0) again.push_back(order[i]);
                    else too_big.push_back(order[i]);
                } else pool_fail = true;
            }
        if (pool_fail) {
            slot_busy[cur.slot] = false;
            if (cur.i1 - cur.i0 == 1 && W.pool_scale >= 8.0) { rc_final = VGA_ERR_POOL; break; }
            W.pool_scale = std::min(16.0, W.pool_scale * 1.7);
            todo.push_back({cur.i0, cur.i1, cur.general, false});  // enqueue it again, in smaller pieces
            fill();
            continue;
        }
        if (cur.raw_est > 0) {
            const double ratio = (double)W.h_next.p[cur.slot] / cur.raw_est;
            // conservative on purpose: a sub-batch that overflows its half takes its unfinished problems down with it
            W.pool_scale = std::max(ratio * 1.15, 0.6 * W.pool_scale + 0.4 * ratio * 1.25);
        }
        if (sw.has_dump_rows) dump_rows(cur);
        if (tr.on) trace_sub_batch(cur, S);
        requeue_handed_back(cur, S);
        // refill the GPU first (the new sub-batch's results go to the slot's other result set), then post-process
        slot_busy[cur.slot] = false;
        fill();
        post_process(cur, S);
    }
}

// drains the streams, reports what went wrong, and accounts: timers, the DP kernel's byte model, what came back over PCIe
int poa_call::finish()
{
    trace_order();
    // drain every stream (also on the error paths: the slots belong to the context)
    for (int i = 1; i < n_slots; i++) (void)hipStreamSynchronize(sarr[i]);
    (void)hipStreamSynchronize(ctx->stream);
    if (launch_err != hipSuccess) return vga_set_error(ctx, VGA_ERR_HIP, "POA launch failed: %s", hipGetErrorString(launch_err));
    if (malformed) return malformed_error();
    if (dev_failed) return dev_rc;  // (sg_prepare_rest has set the message)
    vga_timer_end(ctx, t_total);
    tr.mark("dp + traceback + cigar (pipelined sub-batches)");
    const int rc = pool.check_and_trace_end();
    if (rc != VGA_OK) return rc;
    if (rc_final != VGA_OK)
        return vga_set_error(ctx, rc_final, "a single POA problem does not fit the %llu byte traceback pool", (unsigned long long)W.pool_size);
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    vga_timers_collect(ctx);
    // byte model of the DP kernel: graph bases + query + 1 direction byte per cell
    // + the value rows kept in HBM (6 B per cell), written once and read back at least once
    for (auto &a : ctx->last_times) {
        // (the traceback's 6 bytes per alignment column belong to whichever kernel walked: the DP kernel when fused)
        if (a.name == "poa_band_dp") a.bytes = all_rows + all_q + all_cells + 12 * all_vcells + (any_fused ? 6 * all_ops : 0);
        if (a.name == "poa_traceback") a.bytes = any_fused ? 0 : 6 * all_ops;
    }
    tm.ms_dp = vga_timer_sum(ctx, "poa_band_dp");
    tm.ms_tb = vga_timer_sum(ctx, "poa_traceback");
    tm.ms_total = (float)ms_since_start();
    tm.result_bytes = text_bytes;
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- VGA_TRACE, VGA_POA_DUMP_ROWS
// where the host's time goes between a launch ending and the next one starting
void poa_call::trace_setup(const launch_t &L, const char *what) const
{
    if (tr.on) fprintf(stderr, "[vga-trace] poa:     launch set-up: %-34s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - L.t0).count());
}

void poa_call::trace_shape(const launch_t &L, const poa_shape &sh, double mean_w, double max_w) const
{
    if (!tr.on) return;
    fprintf(stderr, "[vga-trace] poa: (at %.1f ms) launch %u problems, NT %d, %s, window %u of %u columns, width estimate mean %.0f max %.0f, LDS %zu B\n",
            ms_since_start(), L.nb, sh.fam_nt, family == POA_FAM_T5 ? "k_poa_dp_t5" : (family == POA_FAM_T4 ? "k_poa_dp_t4" : "k_poa_dp_lds"), sh.fam_cols,
            sh.lds_cols, mean_w, max_w, sh.fam_lds);
    if (sh.kernel == POA_K_T7) fprintf(stderr, "[vga-trace] poa:     k_poa_dp_t7<%d>: window %u columns, LDS %zu B\n", sh.nt, sh.hg_cols, sh.lds);
    if (sh.kernel == POA_K_T6) fprintf(stderr, "[vga-trace] poa:     k_poa_dp_t6<8>: one wave per problem, LDS %zu B\n", sh.lds);
}

void poa_call::trace_sub_batch(const sub_t &cur, const poa_slot::out_set &S) const
{
    const double nbd = (double)(cur.i1 - cur.i0);
    double worst = 0, lsum = 0, nsum = 0, csum = 0, vsum = 0, rsum = 0, esum = 0;
    uint32_t mx = 0, lmax = 0;
    uint64_t tb = ~0ull, te = 0, tsum = 0;
    // the longest-running workgroup of the launch: what a single problem costs (its rows are sequential)
    uint64_t worst_i = cur.i0, worst_t = 0;
    for (uint64_t i = cur.i0; i < cur.i1; i++) {
        const poa_out &ho = S.h_outs.p[i - cur.i0];
        const poa_prep &g = G[order[i]];
        worst = std::max(worst, (double)ho.maxw / estw[order[i]]);
        mx = std::max(mx, ho.maxw);
        lsum += g.life; nsum += (double)g.n_ntab; lmax = std::max(lmax, g.life);
        csum += (double)ho.cells; vsum += (double)ho.vcells; rsum += g.N; esum += est[order[i]];
        if (ho.t_end > ho.t_begin) {
            tb = std::min(tb, ho.t_begin); te = std::max(te, ho.t_end); tsum += ho.t_end - ho.t_begin;
            if (ho.t_end - ho.t_begin > worst_t) { worst_t = ho.t_end - ho.t_begin; worst_i = i; }
        }
    }
    fprintf(stderr, "[vga-trace] poa:   edge span (nodes): mean %.1f, max %u; nodes %.0f; rows %.0f, cells %.1f M, value cells %.1f M, "
                    "estimate %.1f MB per problem, pool scale %.2f\n", lsum / nbd, lmax, nsum / nbd, rsum / nbd, csum / nbd / 1e6,
            vsum / nbd / 1e6, esum / nbd / 1e6, W.pool_scale);
    const poa_out &ho = S.h_outs.p[worst_i - cur.i0];
    const poa_prep &g = G[order[worst_i]];
    fprintf(stderr, "[vga-trace] poa:   slowest problem: %.1f ms for %u rows (%.2f us per row), %u nodes, %.1f M cells (mean width %.0f, widest %u), "
                    "%.0f %% of them in kept rows, query %u\n", (double)worst_t / 1e5, g.N, (double)worst_t / 100.0 / (double)std::max(1u, g.N),
            g.n_ntab - 1, (double)ho.cells / 1e6, (double)ho.cells / (double)std::max(1u, g.N), ho.maxw, 100.0 * (double)ho.vcells / (double)std::max<uint64_t>(1, ho.cells), g.qlen);
    fprintf(stderr, "[vga-trace] poa: (at %.1f ms) sub-batch [%llu, %llu) done, pool %.1f GB, widest row %u columns, worst width / estimate %.3f; "
                    "DP %.1f ms, mean %.1f workgroups resident, on GPU clock %.3f .. %.3f s\n",
            ms_since_start(), (unsigned long long)cur.i0, (unsigned long long)cur.i1, (double)W.h_next.p[cur.slot] / 1e9, mx, worst,
            te > tb ? (double)(te - tb) / 1e5 : 0.0, te > tb ? (double)tsum / (double)(te - tb) : 0.0, (double)(tb % 100000000000ull) / 1e8,
            (double)(te % 100000000000ull) / 1e8);
}

void poa_call::trace_order() const
{
    if (!tr.on || !feed.proxy) return;
    for (uint64_t i = 0; i < order.size() && i < n; i += std::max<uint64_t>(1, n / 12))
        fprintf(stderr, "[vga-trace] poa:   launch position %llu: proxy %.3g, rows %u, longest path %d, query %u, estimate %.1f MB\n",
                (unsigned long long)i, feed.proxy[order[i]], G[order[i]].N, G[order[i]].longest, G[order[i]].qlen, est[order[i]] / 1e6);
}

// diagnostics: the row records of the launch's first problem
void poa_call::dump_rows(const sub_t &cur) const
{
    const poa_prob &pb0 = probs[order[cur.i0]];
    std::vector<poa_row> hr(pb0.N + 1);
    (void)hipMemcpy(hr.data(), W.slot[cur.slot].d_rows.p + pb0.row0, hr.size() * sizeof(poa_row), hipMemcpyDeviceToHost);
    FILE *f = fopen(sw.dump_rows.c_str(), "w");
    if (!f) return;
    for (size_t r = 0; r < hr.size(); r++) fprintf(f, "%zu %d %d %d %d %u %u %llu\n", r, hr[r].beg, hr[r].end, hr[r].lmax, hr[r].rmax, hr[r].pred, hr[r].npred, (unsigned long long)hr[r].voff);
    fclose(f);
}

}  // namespace

int poa_run(vga_ctx *ctx, poa_feed &feed, const vga_poa_params *params, std::vector<poa_item> &out, poa_timing &tm)
{
    poa_call c(ctx, feed, params, out, tm);
    int rc = c.validate();
    if (rc != VGA_OK || c.n == 0) return rc;
    if (!c.makers.empty()) {
        uint64_t total_q = 0;
        for (const poa_view &v : c.views) total_q += v.qlen;
        for (const auto &m : c.makers)
            if ((rc = m.lists->begin(ctx, c.n, total_q, c.sw.*m.maker->has_cap, c.sw.*m.maker->cap_words)) != VGA_OK) return rc;
    }
    if ((rc = c.order_problems()) != VGA_OK) return rc;
    if ((rc = c.size_pool()) != VGA_OK) return rc;
    if ((rc = c.obtain_pool()) != VGA_OK) return rc;
    c.collect();  // choose, stage, launch; fetch text, requeue, post-process -- pipelined over the sub-batches
    return c.finish();
}

// include/vga_hip.h.  Optional: what the first vga_align_batch call would allocate before its first kernel -- the state regions
// and about half of the chunk segments it is going to ask for -- starts to be allocated now, on a thread of its own.
extern "C" int vga_align_prepare(vga_ctx *ctx, uint64_t n_reads, uint32_t max_read_len)
{
    if (!ctx) return VGA_ERR_ARG;
    if (n_reads == 0 || max_read_len == 0 || max_read_len >= (1u << 24)) return VGA_OK;
    const poa_switches sw = poa_read_switches();
    if (sw.arenas_off) return VGA_OK;  // (classic mode sizes its pool itself)
    if (4ull * ((uint64_t)max_read_len + 8) > POA_CHUNK) return VGA_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return vga_set_error(ctx, VGA_ERR_HIP, "vga_align_prepare: hipSetDevice failed");
    vga_ctx_scope scope(ctx);
    poa_pool_prepare(ctx, sw, n_reads, max_read_len);
    return VGA_OK;
}

extern "C" void vga_poa_result_free(vga_poa_result *r)
{
    if (!r) return;
    free(r->ok); free(r->best_score); free(r->path_off); free(r->abpoa_nodes); free(r->graph_nodes);
    free(r->aln_start_offset); free(r->aln_end_offset); free(r->n_aligned_bases); free(r->cigar_off);
    free(r->cigar); free(r->cs_off); free(r->cs); free(r->n_rows); free(r->n_cells); free(r->n_value_cells);
    free(r);
}

static int vga_poa_batch_impl(vga_ctx *ctx, uint64_t n, const uint64_t *node_ptr, const uint64_t *node_off,
                             const char *nodes_concat, const uint64_t *edge_ptr, const uint32_t *edge_src,
                             const uint32_t *edge_dst, const uint64_t *query_off, const char *queries_concat,
                             const vga_poa_params *params, vga_poa_result **out)
{
    if (!ctx || !out || !params || (n && (!node_ptr || !node_off || !nodes_concat || !edge_ptr || !query_off || !queries_concat)))
        return VGA_ERR_ARG;
    *out = nullptr;
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    vga_release_deferred(ctx);  // (buffers of this context that grew during an earlier call: freed now, while it has nothing in flight)
    poa_feed feed;
    std::vector<poa_view> &views = feed.views;
    views.resize(n);
    for (uint64_t p = 0; p < n; p++) {
        const uint64_t ql = query_off[p + 1] - query_off[p];
        if (ql >= (1ull << 24)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "query %llu too long", (unsigned long long)p);
        views[p] = {node_off + node_ptr[p], nodes_concat, node_ptr[p + 1] - node_ptr[p], edge_src + edge_ptr[p], edge_dst + edge_ptr[p],
                    edge_ptr[p + 1] - edge_ptr[p], queries_concat + query_off[p], (uint32_t)ql};
    }
    std::vector<poa_item> items;
    poa_timing tm;
    int rc = poa_run(ctx, feed, params, items, tm);
    if (rc != VGA_OK) return rc;
    vga_poa_result *res = (vga_poa_result *)calloc(1, sizeof(vga_poa_result));
    if (!res) return vga_set_error(ctx, VGA_ERR_NOMEM, "out of host memory (POA result)");
    auto nomem = [&]() { vga_poa_result_free(res); return vga_set_error(ctx, VGA_ERR_NOMEM, "out of host memory (POA result of %llu problems)", (unsigned long long)n); };
    res->n = n;
    res->ok = pmalloc<uint8_t>(n);
    res->best_score = pmalloc<int32_t>(n);
    res->path_off = pmalloc<uint64_t>(n + 1);
    res->aln_start_offset = pmalloc<uint32_t>(n);
    res->aln_end_offset = pmalloc<uint32_t>(n);
    res->n_aligned_bases = pmalloc<uint32_t>(n);
    res->cigar_off = pmalloc<uint64_t>(n + 1);
    res->cs_off = pmalloc<uint64_t>(n + 1);
    res->n_rows = pmalloc<uint64_t>(n);
    res->n_cells = pmalloc<uint64_t>(n);
    res->n_value_cells = pmalloc<uint64_t>(n);
    if (!res->ok || !res->best_score || !res->path_off || !res->aln_start_offset || !res->aln_end_offset || !res->n_aligned_bases ||
        !res->cigar_off || !res->cs_off || !res->n_rows || !res->n_cells || !res->n_value_cells)
        return nomem();
    uint64_t tp = 0, tc = 0, ts = 0;
    for (uint64_t p = 0; p < n; p++) {
        res->path_off[p] = tp; res->cigar_off[p] = tc; res->cs_off[p] = ts;
        tp += items[p].rows.size(); tc += items[p].cigar.size() + 1; ts += items[p].cs.size() + 1;
    }
    res->path_off[n] = tp; res->cigar_off[n] = tc; res->cs_off[n] = ts;
    res->abpoa_nodes = pmalloc<uint32_t>(tp);
    res->graph_nodes = pmalloc<uint32_t>(tp);
    res->cigar = pmalloc<char>(tc);
    res->cs = pmalloc<char>(ts);
    if (!res->abpoa_nodes || !res->graph_nodes || !res->cigar || !res->cs) return nomem();
    for (uint64_t p = 0; p < n; p++) {
        const poa_item &it = items[p];
        res->ok[p] = it.ok; res->best_score[p] = it.score; res->aln_start_offset[p] = it.start_off;
        res->aln_end_offset[p] = it.end_off; res->n_aligned_bases[p] = it.aligned; res->n_rows[p] = it.n_rows;
        res->n_cells[p] = it.n_cells; res->n_value_cells[p] = it.n_vcells;
        if (!it.rows.empty()) {
            memcpy(res->abpoa_nodes + res->path_off[p], it.rows.data(), it.rows.size() * 4);
            memcpy(res->graph_nodes + res->path_off[p], it.gnodes.data(), it.gnodes.size() * 4);
        }
        memcpy(res->cigar + res->cigar_off[p], it.cigar.c_str(), it.cigar.size() + 1);
        memcpy(res->cs + res->cs_off[p], it.cs.c_str(), it.cs.size() + 1);
    }
    res->ms_dp = tm.ms_dp;
    res->ms_traceback = tm.ms_tb;
    res->ms_total = tm.ms_total;
    *out = res;
    return VGA_OK;
}

extern "C" int vga_poa_batch(vga_ctx *ctx, uint64_t n, const uint64_t *node_ptr, const uint64_t *node_off,
                             const char *nodes_concat, const uint64_t *edge_ptr, const uint32_t *edge_src,
                             const uint32_t *edge_dst, const uint64_t *query_off, const char *queries_concat,
                             const vga_poa_params *params, vga_poa_result **out)
{
    // nothing throws across the C ABI: an allocation failure inside becomes VGA_ERR_NOMEM
    try {
        return vga_poa_batch_impl(ctx, n, node_ptr, node_off, nodes_concat, edge_ptr, edge_src, edge_dst, query_off, queries_concat, params, out);
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_poa_batch: out of host memory");
    } catch (const std::exception &e) {
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_poa_batch: %s", e.what());
    }
}
