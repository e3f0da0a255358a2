// vga_subgraph_host.hip -- the subgraph of a chain from host threads (VGA_SUBGRAPH=host): the second opinion the GPU tests hold
// vga_subgraph.hip's kernels against.
//
//   find_range_chain ............ src/align.rs:267-402   (u64::from(Handle) read as the node id)
//   extend_range_chain_2 ........ src/align.rs:523-665
//   find_nodes_edges_for_abpoa .. src/align.rs:670-724
#include "vga_subgraph_host.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <thread>

namespace {

typedef uint32_t handle_t;  // (id << 1) | is_reverse

struct index_view {
    const vga_dev_index &ix;
    explicit index_view(const vga_dev_index &i) : ix(i) {}

    // get_bv_rank over the node-start bit vector (src/index.rs:427-439): starts <= pos
    uint32_t rank(uint32_t pos) const
    {
        return (uint32_t)(std::upper_bound(ix.node_start.begin(), ix.node_start.end(), pos) - ix.node_start.begin());
    }
    // handle_from_seqpos for a Forward position (src/index.rs:415-423)
    handle_t handle_from_fwd_pos(uint32_t pos) const { return rank(pos) * 2; }
    // get_bv_select (src/index.rs:461-480)
    uint32_t select(uint32_t element_no) const
    {
        if (element_no == 0 || element_no > ix.n_nodes + 1) return 0;
        return ix.node_start[element_no - 1];
    }
    uint32_t node_len(handle_t h) const
    {
        uint32_t id = h >> 1;
        return ix.node_start[id] - ix.node_start[id - 1];
    }
    // incoming_edges_from_handle / outgoing_edges_from_handle (src/index.rs:559-606)
    void incoming(handle_t h, std::vector<handle_t> &out) const
    {
        out.clear();
        uint32_t pos = (h >> 1) - 1;
        if (!(h & 1)) {
            uint32_t s = ix.edge_idx[pos], n = ix.edges_to[pos];
            for (uint32_t i = 0; i < n; i++) out.push_back(ix.edges[s + i]);
        } else {
            outgoing(h ^ 1, out);
            for (auto &x : out) x ^= 1;
            std::reverse(out.begin(), out.end());
        }
    }
    void outgoing(handle_t h, std::vector<handle_t> &out) const
    {
        out.clear();
        uint32_t pos = (h >> 1) - 1;
        if (!(h & 1)) {
            uint32_t s = ix.edge_idx[pos] + ix.edges_to[pos], e = ix.edge_idx[pos + 1];
            for (uint32_t i = s; i < e; i++) out.push_back(ix.edges[i]);
        } else {
            incoming(h ^ 1, out);
            for (auto &x : out) x ^= 1;
            std::reverse(out.begin(), out.end());
        }
    }
    // dna.rs:19-33
    static char complement(char c)
    {
        switch (c) {
        case 'a': return 't'; case 'c': return 'g'; case 't': return 'a'; case 'g': return 'c'; case 'u': return 'a';
        case 'A': return 'T'; case 'C': return 'G'; case 'T': return 'A'; case 'G': return 'C'; case 'U': return 'A';
        default: return 'N';
        }
    }
    // seq_from_handle (src/index.rs:503-533); the reverse strand is derived as dna.rs:19-33 does
    void append_seq(handle_t h, std::string &out) const
    {
        uint32_t id = h >> 1;
        uint32_t s = ix.node_start[id - 1], e = ix.node_start[id];
        if (!(h & 1)) out.append(ix.seq_fwd.data() + s, e - s);
        else
            for (uint32_t i = e; i-- > s;) out.push_back(complement(ix.seq_fwd[i]));
    }
};

struct subgraph_t {
    std::vector<handle_t> handles;  // sorted, deduplicated (src/align.rs:658-659)
    std::vector<uint64_t> node_off; // per node: offset into seqs (n+1)
    std::string seqs;
    std::vector<uint32_t> esrc, edst;
};

struct scratch_t {
    std::vector<uint32_t> best;      // per packed handle: largest remaining budget seen
    std::vector<handle_t> touched;
    std::vector<std::pair<uint32_t, handle_t>> cur, next;
    std::vector<handle_t> nb, lo, hi;
};

// one direction of src/align.rs:551-591 / 616-656.  The reference's walk keeps no visited set (its
// frontier grows exponentially on bubble chains); a handle ends up in the range iff it is reachable
// with a positive remaining budget, which is what the per-handle best-budget relaxation computes (a handle is
// re-expanded only when it is reached with a larger budget than before).
void extend_dir(const index_view &iv, handle_t from, uint32_t diff, bool incoming, std::vector<handle_t> &hs, scratch_t &sc)
{
    const vga_dev_index &ix = iv.ix;
    // neighbours of a handle in walk direction, straight from the edge lists when the handle is forward (it always is
    // with only_forward; the general accessor covers the rest)
    auto for_each_nb = [&](handle_t h, auto &&f) {
        if (!(h & 1)) {
            const uint32_t pos = (h >> 1) - 1;
            const uint32_t s = incoming ? ix.edge_idx[pos] : ix.edge_idx[pos] + ix.edges_to[pos];
            const uint32_t e = incoming ? ix.edge_idx[pos] + ix.edges_to[pos] : ix.edge_idx[pos + 1];
            for (uint32_t i = s; i < e; i++) f(ix.edges[i]);
        } else {
            if (incoming) iv.incoming(h, sc.nb); else iv.outgoing(h, sc.nb);
            for (handle_t x : sc.nb) f(x);
        }
    };
    sc.cur.clear();
    for_each_nb(from, [&](handle_t x) { sc.cur.emplace_back(diff, x); });
    while (!sc.cur.empty()) {
        sc.next.clear();
        for (auto &it : sc.cur) {
            const uint32_t left = it.first;
            const handle_t h = it.second;
            if (sc.best[h] >= left) continue;
            if (sc.best[h] == 0) { hs.push_back(h); sc.touched.push_back(h); }
            sc.best[h] = left;
            const uint32_t len = iv.node_len(h);
            if (len < left) {
                const uint32_t rem = left - len;
                for_each_nb(h, [&](handle_t x) { if (sc.best[x] < rem) sc.next.emplace_back(rem, x); });
            }
        }
        sc.cur.swap(sc.next);
    }
    for (handle_t h : sc.touched) sc.best[h] = 0;
    sc.touched.clear();
}

// find_range_chain + extend_range_chain_2 + find_nodes_edges_for_abpoa for one chain
static std::atomic<long long> g_ns_range{0}, g_ns_extend{0}, g_ns_seq{0}, g_ns_edges{0};  // VGA_TRACE: where the time goes
void build_subgraph(const index_view &iv, const vga_map_result *m, uint64_t read, uint64_t chain, uint32_t k, uint32_t qlen,
                    subgraph_t &sg, scratch_t &sc)
{
    auto tnow = []() { return std::chrono::steady_clock::now(); };
    auto t_a = tnow();
    const uint64_t a0 = m->anchor_off[read];
    const uint64_t c0 = m->chain_anchor_off[chain], c1 = m->chain_anchor_off[chain + 1];
    // smallest / largest handle over the anchors' begin and inclusive end positions (align.rs:286-308).  The position ->
    // handle map is monotonic, so it is enough to look the extreme positions up.
    uint32_t pmin = 0xFFFFFFFFu, pmax = 0;
    for (uint64_t t = c0; t < c1; t++) {
        const uint64_t ai = a0 + m->chain_anchor_idx[t];
        const uint32_t s = m->target_begin[ai], e = m->target_end[ai] - 1;  // get_end_seqpos_inclusive, chain.rs:65-70
        pmin = std::min(pmin, std::min(s, e));
        pmax = std::max(pmax, std::max(s, e));
    }
    const handle_t min_h = iv.handle_from_fwd_pos(pmin), max_h = iv.handle_from_fwd_pos(pmax);
    sg.handles.clear();
    for (uint32_t x = min_h >> 1; x <= (max_h >> 1); x++) sg.handles.push_back(x * 2);  // align.rs:358-364
    const handle_t first_handle = sg.handles.front(), last_handle = sg.handles.back();
    auto t_b = tnow();
    const uint64_t fa = a0 + m->chain_anchor_idx[c0], la = a0 + m->chain_anchor_idx[c1 - 1];
    // align.rs:536-547
    uint32_t prefix_diff = m->query_begin[fa];
    uint32_t start_prefix_on_node = m->target_begin[fa] - iv.select(first_handle >> 1);
    if (start_prefix_on_node < prefix_diff) prefix_diff -= start_prefix_on_node; else prefix_diff = 0;
    if (prefix_diff > 0) extend_dir(iv, first_handle, prefix_diff, true, sg.handles, sc);
    // align.rs:593-612
    uint32_t suffix_diff = qlen - (m->query_begin[la] + k);
    uint32_t end_suffix_on_node = iv.select((last_handle >> 1) + 1) - 1 - (m->target_end[la] - 1);
    if (end_suffix_on_node > suffix_diff) suffix_diff = 0; else suffix_diff -= end_suffix_on_node;
    if (suffix_diff > 0) extend_dir(iv, last_handle, suffix_diff, false, sg.handles, sc);
    // sort + dedup (align.rs:658-659).  The id range is sorted already and the walks only add forward handles, so the
    // result is  sorted(added below the range) + range + sorted(added above it);  anything else takes the general route.
    {
        const size_t n_range = (size_t)((last_handle - first_handle) / 2 + 1);
        bool simple = true;
        sc.lo.clear();
        sc.hi.clear();
        for (size_t i = n_range; i < sg.handles.size(); i++) {
            const handle_t h = sg.handles[i];
            if (h < first_handle) sc.lo.push_back(h);
            else if (h > last_handle) sc.hi.push_back(h);
            else if (h & 1) simple = false;  // a reverse handle inside the range (not reachable with only_forward)
        }
        if (simple) {
            std::sort(sc.lo.begin(), sc.lo.end());
            sc.lo.erase(std::unique(sc.lo.begin(), sc.lo.end()), sc.lo.end());
            std::sort(sc.hi.begin(), sc.hi.end());
            sc.hi.erase(std::unique(sc.hi.begin(), sc.hi.end()), sc.hi.end());
            sg.handles.resize(n_range);
            sg.handles.insert(sg.handles.begin(), sc.lo.begin(), sc.lo.end());
            sg.handles.insert(sg.handles.end(), sc.hi.begin(), sc.hi.end());
        } else {
            std::sort(sg.handles.begin(), sg.handles.end());
            sg.handles.erase(std::unique(sg.handles.begin(), sg.handles.end()), sg.handles.end());
        }
    }
    auto t_c = tnow();
    // align.rs:670-724
    sg.seqs.clear();
    sg.node_off.assign(1, 0);
    for (handle_t h : sg.handles) { iv.append_seq(h, sg.seqs); sg.node_off.push_back(sg.seqs.size()); }
    auto t_d = tnow();
    sg.esrc.clear();
    sg.edst.clear();
    // position of a handle in the sorted list: a dense map over the handles (sc.best is free between extensions),
    // stored as position + 1
    for (uint32_t i = 0; i < sg.handles.size(); i++) sc.best[sg.handles[i]] = i + 1;
    for (uint32_t i = 0; i < sg.handles.size(); i++) {
        iv.outgoing(sg.handles[i], sc.nb);
        for (handle_t t : sc.nb) {
            const uint32_t e1 = sc.best[t];
            if (e1 == 0) continue;  // the neighbour is not in the range
            if (i < e1 - 1) { sg.esrc.push_back(i); sg.edst.push_back(e1 - 1); }  // RangeOrient::Forward, align.rs:718
        }
    }
    for (handle_t h : sg.handles) sc.best[h] = 0;
    auto t_e = tnow();
    g_ns_range += std::chrono::duration_cast<std::chrono::nanoseconds>(t_b - t_a).count();
    g_ns_extend += std::chrono::duration_cast<std::chrono::nanoseconds>(t_c - t_b).count();
    g_ns_seq += std::chrono::duration_cast<std::chrono::nanoseconds>(t_d - t_c).count();
    g_ns_edges += std::chrono::duration_cast<std::chrono::nanoseconds>(t_e - t_d).count();
}

}  // namespace

struct sg_host_walk::impl {
    std::vector<subgraph_t> SG;      // per problem
    std::vector<scratch_t> scratch;  // per thread
};

sg_host_walk::sg_host_walk(vga_ctx *c, const vga_batch *batch, const vga_map_result *chains, const std::vector<uint64_t> &pr,
                           const std::vector<uint64_t> &pc)
    : ctx(c), b(batch), m(chains), prob_read(pr), prob_chain(pc), d(new impl)
{
    const uint64_t n = prob_read.size();
    d->SG.resize(n);
    d->scratch.resize(std::max(1u, vga_host_threads(n)));
    for (auto &sc : d->scratch) sc.best.assign((size_t)(ctx->index.n_nodes + 2) * 2, 0);
}

sg_host_walk::~sg_host_walk() { delete d; }

void sg_host_walk::build(const uint32_t *ids, uint64_t cnt, poa_view *views)
{
    const unsigned nt = std::min<uint64_t>(d->scratch.size(), cnt);
    std::vector<std::thread> th;
    for (unsigned t = 0; t < nt; t++)
        th.emplace_back([&, t]() {
            index_view iv(ctx->index);
            scratch_t &sc = d->scratch[t];
            for (uint64_t q = t; q < cnt; q += nt) {
                const uint32_t p = ids[q];
                const uint64_t r = prob_read[p];
                subgraph_t &sg = d->SG[p];
                build_subgraph(iv, m, r, prob_chain[p], ctx->index.k, (uint32_t)(b->read_off[r + 1] - b->read_off[r]), sg, sc);
                poa_view &v = views[p];
                v.node_off = sg.node_off.data(); v.nodes = sg.seqs.data(); v.n_nodes = sg.handles.size();
                v.esrc = sg.esrc.data(); v.edst = sg.edst.data(); v.n_edges = sg.esrc.size();
            }
        });
    for (auto &x : th) x.join();
}

const uint32_t *sg_host_walk::handles(uint64_t p) const { return d->SG[p].handles.data(); }

void sg_host_walk::trace_thread_time()
{
    fprintf(stderr, "[vga-trace] align: subgraph thread time: range %.1f ms, extension %.1f ms, node strings %.1f ms, edges %.1f ms\n",
            g_ns_range.exchange(0) / 1e6, g_ns_extend.exchange(0) / 1e6, g_ns_seq.exchange(0) / 1e6, g_ns_edges.exchange(0) / 1e6);
}
