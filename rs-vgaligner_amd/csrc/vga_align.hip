// vga_align.hip -- chain -> subgraph -> POA problem -> one alignment record per read.
//
// Stands in for best_alignment_for_query / obtain_base_level_alignment (src/align.rs:34-145):
//   find_range_chain ............ src/align.rs:267-402   (u64::from(Handle) read as the node id)
//   extend_range_chain_2 ........ src/align.rs:523-665
//   find_nodes_edges_for_abpoa .. src/align.rs:670-724
//   create_align_safe ........... src/align.rs:202        -> poa_run (vga_poa_run.hip)
//   generate_alignment .......... src/align.rs:1096-1168  (fields only; the GAF text is host code)
// The subgraph extraction and the POA node tables are built on the GPU (vga_subgraph.hip: one wave per chain over the
// index's CSR arrays in HBM); the host only reduces each chain's anchors to their extremes -- the same pass that fixes
// the launch order (vga_align_plan.hpp).  VGA_SUBGRAPH=host selects the host-thread walk instead (vga_subgraph_host.hip),
// which the GPU tests use as a second opinion.  The ./subgraphs/*.gfa export side effect of align.rs:104-111 is a debugging
// aid and is not reproduced.
#include "vga_align_plan.hpp"
#include "vga_common.hpp"
#include "vga_coverage.hpp"
#include "vga_path_edit.hpp"
#include "vga_path_support.hpp"
#include "vga_pileup.hpp"
#include "vga_insertion.hpp"
#include "vga_poa_internal.hpp"
#include "vga_subgraph_host.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>

extern "C" void vga_align_result_free(vga_align_result *r)
{
    if (!r) return;
    free(r->aligned); free(r->path_off); free(r->path_handles); free(r->path_length); free(r->path_start);
    free(r->path_end); free(r->block_length); free(r->best_score); free(r->cigar_off); free(r->cigar);
    free(r->cs_off); free(r->cs);
    free(r);
}

namespace {

// The state of one vga_align_batch call.  vga_align_batch_impl below is the sequence of its stages.
struct align_call {
    vga_ctx *const ctx;
    vga_batch *const b;
    const vga_map_result *const m;
    const uint32_t align_best_n;
    const vga_poa_params *const params;
    const uint64_t R;
    const align_switches sw = align_read_switches();
    const bool on_device = !sw.sg_host;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    vga_trace tr{"align"};
    ps_state *const ps;  // path support is scored: it reads the run lists that coverage makes
    // ---- plan (vga_align_plan.hpp); the per-problem arrays are in launch order on the device route, in list order on the host's
    std::vector<uint64_t> prob_read, prob_chain, read_prob0;
    std::vector<uint32_t> slot_of;  // where the q-th (read, chain) pair of the selection sits among the problems
    std::vector<double> proxy;
    std::vector<float> west;
    std::vector<sg_desc> descs;
    std::vector<uint64_t> q_src;
    uint64_t n = 0;
    // ---- subgraphs and POA
    poa_feed feed;
    sg_store store;                      // device route
    std::vector<uint8_t> klass;          // 1: a very long problem (by its actual rows, known once its part of the store is ready), launched apart
    std::vector<uint32_t> launch_order;
    std::unique_ptr<sg_host_walk> walk;  // host route
    double sub_ms = 0;
    std::vector<poa_item> items;
    poa_timing tm;
    // ---- records
    std::vector<int64_t> pick;  // per read: the problem whose record is reported, or -1
    std::vector<uint32_t> path_n;
    vga_result_guard<vga_align_result, vga_align_result_free> res;

    align_call(vga_batch *batch, const vga_map_result *chains, uint32_t best_n, const vga_poa_params *p)
        : ctx(batch->ctx), b(batch), m(chains), align_best_n(best_n), params(p), R(batch->n_reads), ps(ps_active(batch->ctx)) {}

    uint32_t qlen(uint64_t r) const { return (uint32_t)(b->read_off[r + 1] - b->read_off[r]); }
    // VGA_STRANDS_BOTH: a read whose chains came from its reverse complement is aligned as that sequence
    uint64_t q_off(uint64_t r) const { return (m->strand && m->strand[r] ? b->total_bases : 0) + b->read_off[r]; }
    int nomem() { return vga_set_error(ctx, VGA_ERR_NOMEM, "out of host memory (align result of %llu reads)", (unsigned long long)R); }

    int reverse_complements();
    int plan();
    int device_store();
    void classify(uint64_t i0, uint64_t i1);
    int device_store_rest();
    void host_walk();
    int run_poa();
    int begin_result();
    void pick_winners();
    int count_winners();
    int fill_result();
};

// The reverse complements sit in the half of the batch behind the forward bases (vga_strand.hip) -- on the device for the
// subgraph and text kernels, on the host for the host routes and the POA staging.  Built here if this batch was never mapped
// with VGA_STRANDS_BOTH.
int align_call::reverse_complements()
{
    bool any_rev = false;
    if (m->strand)
        for (uint64_t r = 0; r < R && !any_rev; r++) any_rev = m->strand[r] != 0;
    if (!any_rev) return VGA_OK;
    const int rc = vga_batch_revcomp_device(b);
    if (rc != VGA_OK) return rc;
    vga_batch_revcomp_host(b);
    tr.mark("reverse complement");
    return VGA_OK;
}

// Which (read, chain) pairs become POA problems, what the subgraph kernels are told about each, and the launch order: largest
// footprint first (poa_run's stable sort by proxy).  The device store is filled in that order, in two parts, so the problems are
// permuted into launch order here and poa_run's sort keeps them; the host route leaves the ordering to poa_run.
int align_call::plan()
{
    // the list makers read the subgraph store's handles on the device
    const char *refused = nullptr;
    for (const oplist_maker *mk : oplist_makers()) {
        if (on_device || refused) break;
        refused = mk->counting(ctx) ? mk->text.refusal : mk == &cov_maker() && ps ? OPLIST_REFUSAL_PATHS : nullptr;
    }
    if (refused) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_REFUSED, refused);
    align_select(m, align_best_n, prob_read, prob_chain, read_prob0);
    n = prob_read.size();
    proxy.resize(n);
    west.resize(n);
    descs.resize(n);
    std::atomic<int> has_reverse{0};
    vga_parallel_for(n, [&](uint64_t p) {
        const align_prob a = align_plan_problem(m, prob_read[p], prob_chain[p], qlen(prob_read[p]), ctx->index.k, sw);
        proxy[p] = a.proxy; west[p] = a.west; descs[p] = a.desc;
        if (a.reverse) has_reverse = 1;
    });
    std::vector<uint32_t> ord(n);
    std::iota(ord.begin(), ord.end(), 0u);
    if (on_device) {
        ord = align_launch_order(proxy);
        align_permute(prob_read, ord); align_permute(prob_chain, ord); align_permute(proxy, ord); align_permute(west, ord); align_permute(descs, ord);
    }
    slot_of = align_slot_of(ord);
    if (has_reverse)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED,
                             "a chain to be aligned holds reverse-strand anchors: RangeOrient::Reverse / Both (src/align.rs:365-387) is not supported");
    feed.views.resize(n);
    q_src.resize(on_device ? n : 0);
    for (uint64_t p = 0; p < n; p++) {
        const uint64_t r = prob_read[p];
        feed.views[p] = {nullptr, nullptr, 0, nullptr, nullptr, 0, b->reads.data() + q_off(r), qlen(r)};
        if (on_device) q_src[p] = q_off(r);
    }
    feed.proxy = proxy.data();
    return VGA_OK;
}

// The device route: the first part of the subgraph store now, the second (device_store_rest) when poa_run first needs it.
int align_call::device_store()
{
    vga_timers_reset(ctx);
    feed.keep_timers = true;
    auto ta = std::chrono::steady_clock::now();
    double mean_west = 0;
    const uint64_t split = align_store_split(west, sw, &mean_west);
    if (sw.trace)
        fprintf(stderr, "[vga-trace] align: mean width term of the launch-order proxy %.0f: the subgraph store is built in %s\n", mean_west,
                split == n ? "one part" : "two parts");
    const int rc = sg_prepare(ctx, descs.data(), q_src.data(), prob_read.data(), n, split, b->d_reads, params->remain_rule, store);
    if (rc != VGA_OK) return rc;
    sub_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
    feed.dev = &store;
    feed.want_rows = false;  // (this caller reads the deduplicated path, its length and the strings: k_poa_text may write them)
    feed.keep_text = true;   // ... and copies each string once, from where it came back (poa_item::cs_p) into the result below
    // The rows of the first part's problems are known now.  Very long ones (config 3's longest have 21 000 rows; a chain
    // that spans 100 kbp of the linearisation has 110 000, all sequential) decide how long the call takes: they go
    // first, in a launch of their own with 512 threads and an 8 192-column window (poa_run).  The order inside the
    // first part is free -- the store is addressed by problem index.
    klass.assign(n, 0);
    launch_order.resize(n);
    std::iota(launch_order.begin(), launch_order.end(), 0u);
    classify(0, store.split);
    feed.order = launch_order.data();
    feed.klass = klass.data();
    feed.dev_rest = [this]() { return device_store_rest(); };
    tr.mark("subgraphs on the GPU");
    return VGA_OK;
}

// problems [i0, i1) of the store, whose part is ready: the very long ones move to the front of that stretch of the launch order
void align_call::classify(uint64_t i0, uint64_t i1)
{
    for (uint64_t i = i0; i < i1; i++)
        klass[i] = align_is_giant(store.sum[i].N, store.sum[i].longest, feed.views[i].qlen, params->wb, params->wf, sw);
    std::stable_sort(launch_order.begin() + (long)i0, launch_order.begin() + (long)i1, [&](uint32_t x, uint32_t y) { return klass[x] > klass[y]; });
}

// poa_feed::dev_rest (called from inside poa_run; none of the second part's problems has been staged yet)
int align_call::device_store_rest()
{
    auto tb = std::chrono::steady_clock::now();
    const int rc = sg_prepare_rest(ctx, store);
    sub_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tb).count();
    if (rc == VGA_OK) classify(store.split, n);
    return rc;
}

// The host route: subgraphs built by the host threads on request, one sub-batch ahead of the GPU (poa_feed::prepare).
void align_call::host_walk()
{
    walk.reset(new sg_host_walk(ctx, b, m, prob_read, prob_chain));
    feed.prepare = [this](const uint32_t *ids, uint64_t cnt) {
        auto ta = std::chrono::steady_clock::now();
        walk->build(ids, cnt, feed.views.data());
        sub_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ta).count();
    };
}

int align_call::run_poa()
{
    tr.mark("launch order");
    if (n > 0) {
        const int rc = poa_run(ctx, feed, params, items, tm);
        if (rc != VGA_OK) return rc;
    }
    tr.mark("poa_run");
    return VGA_OK;
}

int align_call::begin_result()
{
    res.p = (vga_align_result *)calloc(1, sizeof(vga_align_result));
    if (!res.p) return vga_set_error(ctx, VGA_ERR_NOMEM, "out of host memory (align result)");
    res->n_reads = R;
    res->aligned = xmalloc<uint8_t>(R);
    res->path_off = xmalloc<uint64_t>(R + 1);
    res->path_length = xmalloc<uint32_t>(R);
    res->path_start = xmalloc<uint32_t>(R);
    res->path_end = xmalloc<uint32_t>(R);
    res->block_length = xmalloc<uint32_t>(R);
    res->best_score = xmalloc<int32_t>(R);
    res->cigar_off = xmalloc<uint64_t>(R + 1);
    res->cs_off = xmalloc<uint64_t>(R + 1);
    if (!res->aligned || !res->path_off || !res->path_length || !res->path_start || !res->path_end || !res->block_length || !res->best_score ||
        !res->cigar_off || !res->cs_off)
        return nomem();
    return VGA_OK;
}

// per read: keep the candidate with the longest path (stable, align.rs:52-54)
void align_call::pick_winners()
{
    pick.assign(R, -1);
    path_n.assign(R, 0);
    vga_parallel_for(R, [&](uint64_t r) {
        int64_t best = -1;
        for (uint64_t q = read_prob0[r]; q < read_prob0[r + 1]; q++) {
            const uint64_t p = slot_of[q];
            if (!items[p].ok) continue;
            if (best < 0 || items[p].n_path > items[best].n_path) best = (int64_t)p;
        }
        pick[r] = best;
        if (best >= 0) {
            // graph_nodes.dedup() (align.rs:1114): count the runs
            const poa_item &ib = items[best];
            const uint32_t *gn = ib.gnodes_p ? ib.gnodes_p : ib.gnodes.data();
            const size_t gnn = ib.gnodes_p ? ib.gnodes_n : ib.gnodes.size();
            uint32_t c = 0;
            for (size_t t = 0; t < gnn; t++) c += (t == 0 || gn[t] != gn[t - 1]);
            path_n[r] = c;
        }
    });
}

// The list makers, in the table's order, and path support count the reported record of every read and nothing else.  Per maker:
// the winners' lists are staged, and added while its counters are on; path support scores from the run lists coverage staged.
int align_call::count_winners()
{
    if (std::none_of(oplist_makers().begin(), oplist_makers().end(), [&](const oplist_maker *mk) { return mk->making(ctx) != nullptr; })) return VGA_OK;
    std::vector<uint32_t> winners, reads;
    for (uint64_t r = 0; r < R; r++)
        if (pick[r] >= 0) { winners.push_back((uint32_t)pick[r]); reads.push_back((uint32_t)r); }
    int rc = VGA_OK;
    for (const oplist_maker *mk : oplist_makers()) {
        oplist_state *s = mk->making(ctx);
        if (!s) continue;
        if (!winners.empty() && (rc = s->lists.stage_winners(ctx, winners, mk->text)) != VGA_OK) return rc;
        if (mk->counting(ctx)) {
            if (!winners.empty() && (rc = mk->add(ctx, s, winners.size())) != VGA_OK) return rc;
            tr.mark(mk->text.mark);
        }
        if (mk == &cov_maker() && ps) {
            std::vector<uint64_t> off;
            std::vector<uint32_t> len;
            if (ps->pe)  // the edit distance is on: where each winner's query sits in the batch on the device
                for (uint32_t r : reads) { off.push_back(q_off(r)); len.push_back(qlen(r)); }
            const pe_queries q = {b->d_reads, off.data(), len.data()};
            if ((rc = ps_score_winners(ctx, ps, cov_staged_winners(cov_lists_active(ctx), winners.size()), reads, R, &q)) != VGA_OK) return rc;
            tr.mark("path support");
        }
    }
    return VGA_OK;
}

int align_call::fill_result()
{
    uint64_t tp = 0, tc = 0, ts = 0;
    for (uint64_t r = 0; r < R; r++) {
        res->path_off[r] = tp; res->cigar_off[r] = tc; res->cs_off[r] = ts;
        tp += path_n[r];
        tc += pick[r] >= 0 ? (items[pick[r]].cs_p ? items[pick[r]].cigar_n : items[pick[r]].cigar.size()) + 1 : 1;
        ts += pick[r] >= 0 ? (items[pick[r]].cs_p ? items[pick[r]].cs_n : items[pick[r]].cs.size()) + 1 : 1;
    }
    res->path_off[R] = tp; res->cigar_off[R] = tc; res->cs_off[R] = ts;
    res->path_handles = xmalloc<uint64_t>(tp);
    res->cigar = xmalloc<char>(tc);
    res->cs = xmalloc<char>(ts);
    if (!res->path_handles || !res->cigar || !res->cs) return nomem();
    vga_parallel_for(R, [&](uint64_t r) {
        res->aligned[r] = pick[r] >= 0;
        res->path_length[r] = res->path_start[r] = res->path_end[r] = res->block_length[r] = 0;
        res->best_score[r] = 0;
        if (pick[r] < 0) {
            res->cigar[res->cigar_off[r]] = 0;
            res->cs[res->cs_off[r]] = 0;
            return;
        }
        const uint64_t p = (uint64_t)pick[r];
        const poa_item &it = items[p];
        uint64_t o = res->path_off[r];
        const uint32_t *gn = it.gnodes_p ? it.gnodes_p : it.gnodes.data();
        const size_t gnn = it.gnodes_p ? it.gnodes_n : it.gnodes.size();
        const uint32_t *handles = on_device ? store.of(p).h_handles + store.off[p].node0 : walk->handles(p);
        for (size_t t = 0; t < gnn; t++)
            if (t == 0 || gn[t] != gn[t - 1])  // align.rs:1120-1123
                res->path_handles[o++] = handles[gn[t]];
        res->path_length[r] = it.n_path;
        res->path_start[r] = it.start_off;
        res->path_end[r] = it.end_off;
        res->block_length[r] = it.aligned;
        res->best_score[r] = it.score;
        if (it.cs_p) {  // (device text, where it came back: the one copy of the strings on the host)
            memcpy(res->cigar + res->cigar_off[r], it.cigar_p, it.cigar_n); res->cigar[res->cigar_off[r] + it.cigar_n] = 0;
            memcpy(res->cs + res->cs_off[r], it.cs_p, it.cs_n); res->cs[res->cs_off[r] + it.cs_n] = 0;
        } else {
            memcpy(res->cigar + res->cigar_off[r], it.cigar.c_str(), it.cigar.size() + 1);
            memcpy(res->cs + res->cs_off[r], it.cs.c_str(), it.cs.size() + 1);
        }
    });
    res->poa_problems = n;
    for (uint64_t p = 0; p < n; p++) {
        res->poa_rows += items[p].n_rows; res->poa_cells += items[p].n_cells; res->poa_value_cells += items[p].n_vcells;
    }
    res->ms_subgraph = (float)sub_ms;  // GPU kernels before the first DP launch (VGA_SUBGRAPH=host: host threads, overlapped with the GPU)
    res->ms_dp = tm.ms_dp;
    res->ms_traceback = tm.ms_tb;
    res->result_bytes = tm.result_bytes;
    res->ms_total = (float)std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    tr.mark("assemble records");
    if (tr.on && !on_device) sg_host_walk::trace_thread_time();
    return VGA_OK;
}

}  // namespace

static int vga_align_batch_impl(vga_batch *b, const vga_map_result *m, uint32_t align_best_n, const vga_poa_params *params,
                               vga_align_result **out)
{
    if (!b || !m || !params || !out || !b->ctx) return VGA_ERR_ARG;  // b->ctx == nullptr: the context was destroyed
    vga_ctx *ctx = b->ctx;
    *out = nullptr;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_align_batch: no index uploaded");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    vga_release_deferred(ctx);  // (buffers of this context that grew during an earlier call: freed now, while it has nothing in flight)
    if (m->n_reads != b->n_reads) return vga_set_error(ctx, VGA_ERR_ARG, "vga_align_batch: chains belong to a different batch");
    align_call c(b, m, align_best_n, params);
    int rc;
    if ((rc = c.reverse_complements()) != VGA_OK) return rc;
    if ((rc = c.plan()) != VGA_OK) return rc;
    if (c.on_device) {
        if ((rc = c.device_store()) != VGA_OK) return rc;
    } else
        c.host_walk();
    if ((rc = c.run_poa()) != VGA_OK) return rc;
    if ((rc = c.begin_result()) != VGA_OK) return rc;
    c.pick_winners();
    if ((rc = c.count_winners()) != VGA_OK) return rc;
    if ((rc = c.fill_result()) != VGA_OK) return rc;
    *out = c.res.release();
    return VGA_OK;
}

extern "C" int vga_align_batch(vga_batch *b, const vga_map_result *m, uint32_t align_best_n, const vga_poa_params *params,
                               vga_align_result **out)
{
    // nothing throws across the C ABI: an allocation failure inside becomes VGA_ERR_NOMEM
    try {
        return vga_align_batch_impl(b, m, align_best_n, params, out);
    } catch (const std::bad_alloc &) {
        return vga_set_error((b ? b->ctx : nullptr), VGA_ERR_NOMEM, "vga_align_batch: out of host memory");
    } catch (const std::exception &e) {
        return vga_set_error((b ? b->ctx : nullptr), VGA_ERR_ARG, "vga_align_batch: %s", e.what());
    }
}

