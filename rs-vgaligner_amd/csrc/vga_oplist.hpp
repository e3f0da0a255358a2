// vga_oplist.hpp -- what the four list makers share: coverage's k_cov_runs (vga_coverage.hip), the pileup's k_pu_events
// (vga_pileup.hip), the insertion table's k_ia_events (vga_insertion.hip) and the deletion store's k_dl_events (vga_deletion.hip) condense the traceback of every finished problem into
// a short list, and the winners' lists are counted once the host has picked them.  Here is the one copy of the walk over the
// operations (device, and host for a list that found no room), of the record of a list, of the per-call store of lists and of the
// host frame of a maker: the base of its state, the enqueue of its list kernel, the add of the staged winners, its begin / reset /
// end, and the descriptor (oplist_maker) through which poa_run and vga_align_batch reach it.  Each maker keeps what is its own:
// what counts as "in a run", what else it lists, its kernels, its counters and what it reads out.  A new maker is a .hip with
// those, an oplist_text and an oplist_maker, and one entry of oplist_makers.
//
// There is a fourth reader of the same operation stream: k_poa_text (vga_poa_text.hpp, compiled into vga_poa.hip).  It is on the
// path of every alignment, carries other state from block to block (the text's run lengths) and keeps its own copy of the
// prologue, of node_of and of "a row opens a node when npred != 0".  Whoever changes the meaning of an operation, of a row record
// or of the node table changes it there too.
#pragma once

#include <algorithm>
#include <array>

#include "vga_common.hpp"
#include "vga_oplist_text.hpp"
#include "vga_poa_launch.hpp"
#include "vga_subgraph.hpp"

// one problem's list: n_a words of the first kind, then n_b words of the second, at word `off` of its buffer (vga_coverage.hpp,
// vga_pileup.hpp and vga_insertion.hpp say what the kinds are)
struct oplist_rec {
    uint32_t off, n_a, n_b;
    uint32_t flags;  // low two bits: 0 nothing (the problem has no alignment yet), 1 in the call's device buffer, 2 no room there,
                     // 3 built by the host; bit 2 (pileup and insertion table): the alignment starts with an insertion (it belongs to no base);
                     // from bit 2 up (deletion store): the number of end runs of the record
};
#define PU_LEADING 4u

// ---------------------------------------------------------------------------------------------------------- device: the walk
// the value of the lane below; lane 0 takes `carry` (the last lane of the previous block)
__device__ __forceinline__ uint32_t opl_shr1(uint32_t v, uint32_t carry, int lane)
{
    const uint32_t t = (uint32_t)__shfl_up((int)v, 1);
    return lane == 0 ? carry : t;
}
__device__ __forceinline__ uint64_t opl_below(int lane) { return (1ull << lane) - 1ull; }  // the lanes below this one

// a problem of a finished launch as the walk sees it
struct opl_prob {
    uint32_t nops, N, qlen, nv;  // nv: entries of the node table incl. the virtual source (entry 0)
    const uint8_t *op_p;
    const uint32_t *or_p;
    const poa_row *R;
    const uint4 *ntab;
    const uint32_t *hd;  // the problem's slice of the subgraph store's handles
    const uint32_t *node_start;
    uint32_t n_graph_nodes;
    const char *bases, *q;  // (QUERY only) row r is bases[r - 1]
    __device__ __forceinline__ uint32_t node_of(uint32_t row) const  // 0-based index of the real node that holds `row`
    {
        uint32_t lo = 1, hi = nv;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (ntab[mid].x <= row) lo = mid; else hi = mid;
        }
        return lo - 1;
    }
};

// The prologue of a list maker's wave: problem pi of the launch.  False: the problem has no alignment, its record says "nothing"
// and the wave is done.  ids[2 i] is problem i's index in the subgraph store.  A maker that reads no bases passes QUERY = false
// and null for seq and queries.
template <bool QUERY>
__device__ __forceinline__ bool opl_open(opl_prob &P, uint32_t pi, int lane, const poa_prob *probs, const poa_out *outs, const uint8_t *ops,
                                         const uint32_t *orow, const poa_row *rows, const uint4 *node_tab, const char *seq, const char *queries,
                                         const uint32_t *ids, const sg_off *offs, uint32_t split, const uint32_t *handles0, const uint32_t *handles1,
                                         const uint32_t *node_start, uint32_t n_graph_nodes, oplist_rec *recs)
{
    const poa_prob pb = probs[pi];
    const poa_out po = outs[pi];
    if (po.status != POA_ST_OK) {
        if (lane == 0) recs[pi] = oplist_rec{0u, 0u, 0u, 0u};
        return false;
    }
    const uint32_t p = ids[2 * pi];
    P.hd = (p >= split ? handles1 : handles0) + offs[p].node0;
    P.nops = po.nops; P.N = pb.N; P.qlen = pb.qlen; P.nv = pb.n_nodes;
    P.op_p = ops + pb.ops0;
    P.or_p = orow + pb.ops0;
    P.R = rows + pb.row0;
    P.ntab = node_tab + pb.node0;
    P.node_start = node_start; P.n_graph_nodes = n_graph_nodes;
    P.bases = nullptr; P.q = nullptr;
    if constexpr (QUERY) { P.bases = seq + pb.seq0; P.q = queries + pb.q0; }
    return true;
}

// what a pass carries from block to block for opl_block: the open node's offset  position - row, the query bases consumed
struct opl_carry { uint32_t c_delta = 0, qi0 = 0; };

// this lane's operation of a block of 64
struct opl_lane {
    uint32_t op, row;
    bool valid, cg;    // an operation of the alignment / one that consumes a graph base (M or D on a row of the graph)
    bool opens;        // its row opens a node: the path enters node `id` (1-based id of the graph) here
    uint32_t id, g;    // g: position on the linearised graph (seq_fwd) of a cg operation
    uint64_t omask;    // the lanes that open a node
    bool cq;           // (QUERY) consumes a query base: the qi-th, qb; gb is the graph base of a cg operation
    uint32_t qi;
    char gb, qb;
};

// One block of the walk: the operations are stored sink -> source and read forward, 64 at a time; the block at `base` may lie
// behind the last operation (the closing block: no lane is valid, nothing is loaded).  A row opens a node exactly when its row
// record has predecessors of its own (k_poa_text's rule); only those rows look their node up (binary search over the node table,
// handle from the subgraph store, start from the index), every other row takes the offset of the latest opening row before it.
template <bool QUERY>
__device__ __forceinline__ opl_lane opl_block(const opl_prob &P, uint32_t base, int lane, opl_carry &c)
{
    opl_lane o = {};
    const uint32_t f = base + (uint32_t)lane;
    o.valid = f < P.nops;
    o.op = 3;
    if (o.valid) { o.op = P.op_p[P.nops - 1 - f]; o.row = P.or_p[P.nops - 1 - f]; }
    // (an invalid lane has op 3; evaluated without branches: the loads that follow then overlap)
    o.cg = ((o.op == 0) | (o.op == 2)) & (o.row - 1u < P.N);  // row in [1, N]
    if constexpr (QUERY) {
        o.cq = o.valid && (o.op == 0 || o.op == 1);
        const uint64_t qmask = __builtin_amdgcn_ballot_w64(o.cq);
        o.qi = c.qi0 + (uint32_t)__builtin_popcountll(qmask & opl_below(lane));
        c.qi0 += (uint32_t)__builtin_popcountll(qmask);
        o.gb = o.cg ? P.bases[o.row - 1] : (char)0;
        o.qb = (o.cq && o.qi < P.qlen) ? P.q[o.qi] : (char)0;
    }
    o.opens = o.cg && P.R[o.row].npred != 0u;
    uint32_t my_delta = 0;
    if (o.opens) {
        o.id = P.hd[P.node_of(o.row)] >> 1;
        if (o.id < 1u || o.id > P.n_graph_nodes) o.id = 1u;  // (cannot happen with a store built from this index)
        my_delta = P.node_start[o.id - 1] - o.row;
    }
    o.omask = __builtin_amdgcn_ballot_w64(o.opens);
    const uint64_t o_le = o.omask & (opl_below(lane) | (1ull << lane));
    const uint32_t got = (uint32_t)__shfl((int)my_delta, o_le ? 63 - __builtin_clzll(o_le) : 0);
    o.g = o.row + (o_le ? got : c.c_delta);
    if (o.omask) c.c_delta = (uint32_t)__shfl((int)my_delta, 63 - __builtin_clzll(o.omask));
    return o;
}

// The run cutter: runs of "in a run" operations on consecutive positions become event words, position << 1 where a run starts,
// (position behind its last base) << 1 | 1 where it ends.  Lanes ascend; the word that ends the run before a lane precedes the
// word that starts this lane's.  Carried from block to block: was the last operation in a run, and its position.
struct opl_runs {
    uint32_t c_m = 0, c_g = 0;
    uint32_t n = 0;  // event words of the pass so far
    struct cut {
        bool start, end;
        uint32_t slot, p_g;  // where this lane's words go among the pass's events; the position of the lane below
        __device__ __forceinline__ void put(uint32_t *ev_w, uint32_t g) const
        {
            uint32_t *w = ev_w + slot;
            if (end) *w++ = ((p_g + 1u) << 1) | 1u;
            if (start) *w = g << 1;
        }
    };
    __device__ __forceinline__ cut step(uint32_t in_run, uint32_t g, int lane)
    {
        const uint32_t p_m = opl_shr1(in_run, c_m, lane), p_g = opl_shr1(g, c_g, lane);
        const bool cont = in_run && p_m && p_g + 1u == g;
        const bool start = in_run && !cont, end = p_m && !cont;
        const uint64_t stmask = __builtin_amdgcn_ballot_w64(start), enmask = __builtin_amdgcn_ballot_w64(end), below = opl_below(lane);
        const cut k = {start, end, n + (uint32_t)(__builtin_popcountll(stmask & below) + __builtin_popcountll(enmask & below)), p_g};
        n += (uint32_t)(__builtin_popcountll(stmask) + __builtin_popcountll(enmask));
        c_m = (uint32_t)__builtin_amdgcn_readlane((int)in_run, 63);
        c_g = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
        return k;
    }
};

// The claim between the two passes: one atomic add by lane 0, broadcast.  False: no room, the record says so (flags 2, with the
// maker's `extra` bits) and the wave is done; else T.off is where the list goes.
__device__ __forceinline__ bool opl_claim(oplist_rec &T, uint32_t pi, int lane, uint32_t extra, uint32_t list_words, unsigned long long *cursor,
                                          oplist_rec *recs)
{
    const uint32_t words = T.n_a + T.n_b;
    unsigned long long at = 0;
    if (lane == 0) at = atomicAdd(cursor, (unsigned long long)words);
    at = (unsigned long long)__shfl((long long)at, 0);
    if (at + words > (unsigned long long)list_words) {
        T.flags = 2u | extra;
        if (lane == 0) recs[pi] = T;
        return false;
    }
    T.off = (uint32_t)at;
    return true;
}

// The block scan of the two read kernels (one workgroup of 1024 threads): thread t takes the contiguous piece [a, b) of diff[0, n)
// and gets diff[0] + ... + diff[a - 1]; the pieces' sums are scanned in LDS.
__device__ __forceinline__ uint32_t opl_block_scan(const uint32_t *__restrict__ diff, uint32_t n, uint32_t &a, uint32_t &b)
{
    __shared__ uint32_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t piece = (n + 1023u) / 1024u;
    const uint64_t a64 = (uint64_t)tid * piece, b64 = a64 + piece;
    a = a64 < n ? (uint32_t)a64 : n; b = b64 < n ? (uint32_t)b64 : n;
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
    return tid ? part[tid - 1] : 0u;
}

// ------------------------------------------------------------------------------------------------------ host: the list store
// The lists of the vga_align_batch call in progress, for one maker.
struct oplist_call {
    vga_dbuf<uint32_t> d_lists;                // the lists the maker's kernel writes, claimed through d_cur
    uint32_t list_words = 0;
    vga_dbuf<unsigned long long> d_cur;
    vga_dbuf<oplist_rec> d_recs[POA_SLOTS];    // per staged problem of the slot's launch
    vga_hbuf<oplist_rec> h_recs[POA_SLOTS][2];
    std::vector<oplist_rec> recs;              // per problem of the call
    std::vector<uint32_t> host_lists;          // lists the host built (flags 3)
    vga_dbuf<uint32_t> d_host_lists;
    vga_dbuf<oplist_rec> d_win;
    vga_hbuf<oplist_rec> h_win;

    // start of a poa_run call of n problems whose queries hold total_q bases: the buffer of lists is sized (cap_words caps it when
    // has_cap) and its cursor zeroed.  About a word per read base is what coverage needs on a graph of short nodes with reads of
    // 10 % errors, the pileup 0.4.  Not a bound -- a problem that finds no room says so and the host builds its list
    // (VGA_COV_LIST_WORDS, VGA_PILEUP_LIST_WORDS, VGA_INS_LIST_WORDS and VGA_DEL_LIST_WORDS cap the buffers: the tests force that route with them)
    int begin(vga_ctx *ctx, uint64_t n, uint64_t total_q, bool has_cap, uint64_t cap_words)
    {
        uint64_t words = std::min<uint64_t>(total_q + 256ull * n + 4096ull, 0xFFFFFF00ull);
        if (has_cap) words = std::min<uint64_t>(words, cap_words);
        VGA_HIP_CHECK(ctx, d_lists.reserve(words + 1));
        VGA_HIP_CHECK(ctx, d_cur.reserve(1));
        list_words = (uint32_t)words;
        VGA_HIP_CHECK(ctx, hipMemsetAsync(d_cur.p, 0, sizeof(unsigned long long), ctx->stream));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the launches' streams do not wait for the context's)
        recs.assign(n, oplist_rec{0u, 0u, 0u, 0u});
        host_lists.clear();
        return VGA_OK;
    }
    // the records of a finished launch (valid once its stream is synchronised)
    const oplist_rec *launch_recs(int slot, int oset) const { return h_recs[slot][oset].p; }
    // keeps the record of problem p (a later run of the same problem replaces it)
    void keep(uint32_t p, const oplist_rec &r) { recs[p] = r; }
    // the same for a list the host built: words of the first kind, of the second
    void keep_host(uint32_t p, const std::vector<uint32_t> &a, const std::vector<uint32_t> &b, uint32_t extra_flags)
    {
        recs[p] = oplist_rec{(uint32_t)host_lists.size(), (uint32_t)a.size(), (uint32_t)b.size(), 3u | extra_flags};
        host_lists.insert(host_lists.end(), a.begin(), a.end());
        host_lists.insert(host_lists.end(), b.begin(), b.end());
    }
    // the records of the winners (problem indices of the call that just ended; at least one) and the lists the host built go to
    // the device, on the context's stream.  `t` names the maker and its list in the error for a winner without a list.
    int stage_winners(vga_ctx *ctx, const std::vector<uint32_t> &winners, const oplist_text &t)
    {
        const size_t nw = winners.size();
        VGA_HIP_CHECK(ctx, h_win.reserve(nw));
        VGA_HIP_CHECK(ctx, d_win.reserve(nw));
        for (size_t i = 0; i < nw; i++) {
            const oplist_rec &r = recs[winners[i]];
            if ((r.flags & 3u) != 1u && (r.flags & 3u) != 3u) return vga_set_error(ctx, VGA_ERR_HIP, OPLIST_ERR_NO_LIST, t.who, i, t.what, r.flags);
            h_win.p[i] = r;
        }
        hipStream_t st = ctx->stream;
        VGA_HIP_CHECK(ctx, d_host_lists.reserve(host_lists.size() + 1));
        if (!host_lists.empty())
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_host_lists.p, host_lists.data(), host_lists.size() * 4, hipMemcpyHostToDevice, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_win.p, h_win.p, nw * sizeof(oplist_rec), hipMemcpyHostToDevice, st));
        return VGA_OK;
    }
};

// ---------------------------------------------------------------------------------------------- host: the walk, for no room
// a problem's operations as they came back (stored sink -> source) and what places them on the graph; bases[r - 1] is the base of
// graph row r and query the sequence that was aligned (both only read by a walk with QUERY)
struct oplist_ops {
    const uint8_t *ops;
    const uint32_t *orow;
    uint32_t nops;
    const uint32_t *first_row;  // of the problem's n_nodes nodes
    uint32_t n_nodes, n_rows;
    const uint32_t *handles;
    const uint32_t *node_start;
    const char *bases, *query;
};
struct oplist_op {
    uint32_t op;
    bool cg, enters;   // consumes a graph base (M or D on a row of the graph) / is the first of node `id` on the path
    uint32_t id, g;    // of a cg operation: its node and its position on the linearised graph
    char gb, qb;       // (QUERY) of an M that is cg: the graph base and the read base
};
// the host's copy of the walk: f(oplist_op) per operation, source to sink
template <bool QUERY, class F>
void oplist_walk_host(const oplist_ops &o, F &&f)
{
    uint32_t v = 0, qi = 0;
    for (uint32_t x = o.nops; x > 0; x--) {
        oplist_op k = {o.ops[x - 1], false, false, 0u, 0u, (char)0, (char)0};
        const uint32_t r = o.orow[x - 1];
        if ((k.op == 0 || k.op == 2) && r >= 1 && r <= o.n_rows) {
            while (v + 1 < o.n_nodes && o.first_row[v + 1] <= r) v++;  // rows ascend along the path
            k.cg = true;
            k.enters = r == o.first_row[v];
            k.id = o.handles[v] >> 1;
            k.g = o.node_start[k.id - 1] + (r - o.first_row[v]);
            if (QUERY && k.op == 0) { k.gb = o.bases[r - 1]; k.qb = o.query[qi]; }
        }
        if (k.op == 0 || k.op == 1) qi++;
        f(k);
    }
}
// the run cutter's host side: step() per operation, close() behind the last
struct oplist_runs_host {
    std::vector<uint32_t> ev;
    bool prev_m = false;
    uint32_t pg = 0;
    void close()
    {
        if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
        prev_m = false;
    }
    void step(bool in_run, uint32_t g)
    {
        if (!in_run) return close();
        if (!(prev_m && pg + 1 == g)) { close(); ev.push_back(g << 1); }
        prev_m = true;
        pg = g;
    }
};

// ------------------------------------------------------------------------------------------------ host: the frame of a maker
// What the three states share; a maker derives its own from it and adds its counters.
struct oplist_state {
    uint32_t seq_length = 0;
    uint64_t n_alignments = 0;  // counted since begin / reset
    oplist_call lists;          // of the vga_align_batch call in progress
};

// what poa_run hands a maker's enqueue: the nb problems staged on a slot, whose records go into the slot's result set `oset`
struct oplist_launch {
    hipStream_t st; int slot, oset; uint32_t nb;
    const poa_launch_bufs &b;
    const uint32_t *ids;
    const sg_store &store;
};

// a buffer of a maker's 32-bit counters: begin reserves `words`, begin and reset zero them unless the buffer is scratch of its read
struct oplist_counter { vga_dbuf<uint32_t> *buf; size_t words; bool zeroed; };

// One per maker, handed out by a function of its .hip (cov_maker(), pu_maker(), ia_maker(), dl_maker(): a constant at namespace scope would be
// emitted for the device too, where its hooks do not exist); oplist_makers() (vga_oplist.hip) is the table poa_run and
// vga_align_batch walk, in the order in which the winners are counted.  The frame below calls the hooks.
struct oplist_maker {
    const oplist_text &text;
    oplist_state *(*making)(vga_ctx *ctx);    // the state while poa_run makes its lists, else null
    oplist_state *(*counting)(vga_ctx *ctx);  // ... while its counters are on (between its begin and end), else null
    bool poa_switches::*has_cap; uint64_t poa_switches::*cap_words;  // its VGA_*_LIST_WORDS
    hipError_t (*enqueue)(vga_ctx *ctx, oplist_call &lists, const oplist_launch &L);  // its list kernel behind k_poa_text: oplist_enqueue
    void (*keep_from_ops)(oplist_call &lists, uint32_t p, const oplist_ops &o);       // the host route for a list that found no room
    int (*add)(vga_ctx *ctx, oplist_state *s, size_t nw);                             // its add kernel over the nw staged winners: oplist_add_staged
    bool (*fits)(const vga_dev_index &ix);                        // the graph is within oplist_text::limit
    int (*acquire)(vga_ctx *ctx, const char *fn);                 // the state exists and counts (oplist_make), for the entry point fn
    void (*release)(vga_ctx *ctx);
    std::vector<oplist_counter> (*counters)(const vga_dev_index &ix, oplist_state *s);  // its device counters for this index (seq_length is set)
    void (*zero_own)(oplist_state *s);                            // its own host counters start again (null: it has none)
};
const std::array<const oplist_maker *, 4> &oplist_makers();

// vga_<name>_begin / _reset / _end for the entry point fn (its __func__)
int oplist_begin(vga_ctx *ctx, const oplist_maker &m, const char *fn);
int oplist_reset(vga_ctx *ctx, const oplist_maker &m, const char *fn);
int oplist_end(vga_ctx *ctx, const oplist_maker &m);
// the state while the maker counts; else (and for a null context) null, and the error of fn is set: the caller returns VGA_ERR_ARG
oplist_state *oplist_on(vga_ctx *ctx, const oplist_maker &m, const char *fn);
// VGA_ERR_UNSUPPORTED once a 32-bit counter may have wrapped
int oplist_wrapped(vga_ctx *ctx, const oplist_state *s, const char *fn);

// oplist_maker::acquire of a maker that owns its slot of the index alone
template <class S>
int oplist_make(vga_ctx *ctx, vga_owned<S> &slot, const char *fn)
{
    if (!slot && !(slot = vga_make_owned<S>())) return vga_set_error(ctx, VGA_ERR_NOMEM, OPLIST_ERR_NO_MEMORY, fn);
    return VGA_OK;
}

// oplist_maker::enqueue: `kernel` over the problems of L on its stream, timed as `timer`, and the copy of their records to the host.
// The argument pack is the one every list kernel takes; QUERY: the gathered node sequences and the queries go in (opl_open<true>)
template <bool QUERY, typename... P>
hipError_t oplist_enqueue(vga_ctx *ctx, oplist_call &lists, const oplist_launch &L, const char *timer, void (*kernel)(P...))
{
    vga_dbuf<oplist_rec> &d_recs = lists.d_recs[L.slot];
    vga_hbuf<oplist_rec> &h_recs = lists.h_recs[L.slot][L.oset];
    hipError_t e;
    if ((e = d_recs.reserve(L.nb)) != hipSuccess) return e;
    if ((e = h_recs.reserve(L.nb)) != hipSuccess) return e;
    auto launch = [&](auto... query_side) {
        return vga_launch_on(ctx, L.st, timer, 0, kernel, dim3(L.nb), dim3(64), L.nb, L.b.probs, L.b.outs, L.b.ops, L.b.orow, L.b.rows, L.b.ntab, query_side..., L.ids,
                             L.store.d_off, (uint32_t)L.store.split, L.store.part[0].d_handles, L.store.part[1].d_handles, ctx->index.d_node_start,
                             (uint32_t)ctx->index.n_nodes, lists.d_lists.p, lists.list_words, lists.d_cur.p, d_recs.p);
    };
    if constexpr (QUERY) e = launch((const char *)L.b.seq32, L.b.q);
    else e = launch();
    if (e != hipSuccess) return e;
    return hipMemcpyAsync(h_recs.p, d_recs.p, L.nb * sizeof(oplist_rec), hipMemcpyDeviceToHost, L.st);
}

// oplist_maker::add: `kernel` (n, records, lists, host lists, own ...) over the nw staged winners on the context's stream, then
// before_wait() on the same stream (a failing one still drains it), the wait, and the call's timers once more with this launch
template <class Step, typename... P, typename... A>
int oplist_add_staged(vga_ctx *ctx, oplist_state *s, size_t nw, const char *name, void (*kernel)(P...), Step &&before_wait, A... own)
{
    int rc = vga_launch(ctx, name, 0, kernel, dim3((unsigned)nw), dim3(64), (uint32_t)nw, s->lists.d_win.p, s->lists.d_lists.p, s->lists.d_host_lists.p, own...);
    if (rc != VGA_OK) return rc;
    if ((rc = before_wait()) != VGA_OK) { (void)hipStreamSynchronize(ctx->stream); return rc; }
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    s->n_alignments += nw;
    vga_timers_collect(ctx);  // (poa_run collected before this launch: once more, with it)
    return VGA_OK;
}

// ------------------------------------------------------------------------------------ host: the calls over a finished table
// What vga_variant.hip and vga_insertion.hip share beyond vga_launch and OPLIST_ERR_WIDE: n items of a table of the caller's
// go to the device on the context's stream (nothing for n == 0)
template <typename T, typename H>
int table_upload(vga_ctx *ctx, vga_dbuf<T> &d, const H *host, size_t n)
{
    static_assert(sizeof(T) == sizeof(H), "a copy, not a conversion");
    if (n == 0) return VGA_OK;
    VGA_HIP_CHECK_OOM(ctx, d.reserve(n));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d.p, host, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return VGA_OK;
}
