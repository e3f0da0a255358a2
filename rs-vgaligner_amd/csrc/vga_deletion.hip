// vga_deletion.hip -- deletions of several graph bases as one event each: k_dl_events, k_dl_keep, the kernels of the call
// (k_dl_keys, k_dl_gather, k_dl_heads, k_dl_starts, k_dl_group, k_dl_emit, between them the sort and the scan of
// vga_sort_scan.hpp) and the C entry points vga_deletion_begin / _read / _reset / _end / _call / _call_table / _state.  See
// vga_deletion.hpp for the shape and the rule.
//
// Meaning (include/vga_hip.h): along the reported record of a read, a maximal run of D operations is one event (first, len, last)
// unless the record has no M operation before it or none behind it (an end run, counted in n_end_runs).  The events of the
// reported alignments are appended to the context's store in the order of the alignments and, within one, along it.  The call
// sorts the store's events by (first, len, last), counts each distinct one (reads), takes the depth of its first base from the
// pileup table and applies dl_rule.  Everything is an integer and every sum is a count of equal keys, so the result does not
// depend on the order of the store.
#include "vga_deletion.hpp"

#include "vga_pileup.hpp"
#include "vga_sort_scan.hpp"
#include "vga_variant.hpp"

namespace {

// One wave per problem of a finished launch.  Walks the traceback's operations twice (vga_oplist.hpp: opl_block) and writes the
// problem's list: three words per run of D operations that has an M operation before it and one behind it.  The event is emitted
// at the lane that CLOSES the run -- its own operation is not D, the operation of the lane below (or the one carried from the
// previous block) is -- so that a run may start any number of blocks before it ends; the loop runs one virtual closing block
// behind the last operation, whose first invalid lane closes a run that ends the alignment.  Of the closing lane,
//   first = the position of the latest run-start lane below it, or the one carried from the previous blocks (the run that is
//           open at a block's end is the one that started last);
//   last  = the position of the lane below, or the carry;
//   len   = the graph-consuming operations before it minus those before the run's first D (D consumes a graph base, and a run
//           holds nothing else);
//   before = an M operation below it, or in an earlier block (a carried flag).
// Whether an M follows is known at the end of the first pass: `tail` counts the events closed since the last M, and the last
// `tail` events of the record are end runs.  All carried state is wave-uniform.  Two passes: the count first, one atomic add
// claims the words, then the words.
__global__ __launch_bounds__(64) void k_dl_events(uint32_t n, const poa_prob *__restrict__ probs, const poa_out *__restrict__ outs,
                                                   const uint8_t *__restrict__ ops, const uint32_t *__restrict__ orow, const poa_row *__restrict__ rows,
                                                   const uint4 *__restrict__ node_tab, const uint32_t *__restrict__ ids, const sg_off *__restrict__ offs,
                                                   uint32_t split, const uint32_t *__restrict__ handles0, const uint32_t *__restrict__ handles1,
                                                   const uint32_t *__restrict__ node_start, uint32_t n_graph_nodes, uint32_t *__restrict__ lists,
                                                   uint32_t list_words, unsigned long long *__restrict__ cursor, dl_rec *__restrict__ recs)
{
    const uint32_t pi = blockIdx.x;
    if (pi >= n) return;
    const int lane = threadIdx.x;
    opl_prob P;
    if (!opl_open<false>(P, pi, lane, probs, outs, ops, orow, rows, node_tab, nullptr, nullptr, ids, offs, split, handles0, handles1, node_start,
                         n_graph_nodes, recs))
        return;
    dl_rec T = {0u, 0u, 0u, 0u};
    uint32_t *list_w = nullptr;
    const uint64_t below = opl_below(lane);
    uint32_t n_keep = 0, n_end = 0;  // the events of the list; the record's end runs
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        opl_carry c;
        // carried from block to block: was the last operation a D and its position, the position of the first D of the run that
        // started last and the graph bases consumed before it, the graph bases consumed so far, was there an M
        uint32_t c_d = 0, c_g = 0, c_first = 0, c_gi_first = 0, c_gi0 = 0, c_has_m = 0;
        uint32_t n_ev = 0, tail = 0, lead = 0;
        for (uint32_t base = 0; base <= P.nops; base += 64) {
            const opl_lane o = opl_block<false>(P, base, lane, c);
            const uint32_t is_d = (o.cg && o.op == 2u) ? 1u : 0u;  // (an invalid lane has op 3)
            const bool is_m = o.valid && o.op == 0u;
            const uint32_t p_d = opl_shr1(is_d, c_d, lane), p_g = opl_shr1(o.g, c_g, lane);
            const bool starts = is_d && !p_d, closes = !is_d && p_d;
            const uint64_t gmask = __builtin_amdgcn_ballot_w64(o.cg);
            const uint32_t gi = c_gi0 + (uint32_t)__builtin_popcountll(gmask & below);
            const uint64_t smask = __builtin_amdgcn_ballot_w64(starts), s_lt = smask & below;
            const int s_at = s_lt ? 63 - __builtin_clzll(s_lt) : 0;
            const uint32_t first_s = (uint32_t)__shfl((int)o.g, s_at), gi_s = (uint32_t)__shfl((int)gi, s_at);
            const uint32_t first = s_lt ? first_s : c_first, gi_first = s_lt ? gi_s : c_gi_first;
            const uint64_t mmask = __builtin_amdgcn_ballot_w64(is_m);
            const bool before = (mmask & below) != 0ull || c_has_m != 0u;
            const bool ev = closes && before;
            const uint64_t emask = __builtin_amdgcn_ballot_w64(ev);
            const uint32_t idx = n_ev + (uint32_t)__builtin_popcountll(emask & below);
            if (wr && ev && idx < n_keep) {
                uint32_t *w = list_w + DL_EVENT_WORDS * idx;
                w[0] = first;
                w[1] = gi - gi_first;
                w[2] = p_g;
            }
            n_ev += (uint32_t)__builtin_popcountll(emask);
            lead += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(closes && !before));
            // the events closed behind the block's last M, or all of them on top of the carry
            if (mmask) tail = (uint32_t)__builtin_popcountll(emask & ~((2ull << (63 - __builtin_clzll(mmask))) - 1ull));
            else tail += (uint32_t)__builtin_popcountll(emask);
            // ---- carries
            c_d = (uint32_t)__builtin_amdgcn_readlane((int)is_d, 63);
            c_g = (uint32_t)__builtin_amdgcn_readlane((int)o.g, 63);
            if (smask) {
                const int s_top = 63 - __builtin_clzll(smask);
                c_first = (uint32_t)__shfl((int)o.g, s_top);
                c_gi_first = (uint32_t)__shfl((int)gi, s_top);
            }
            c_gi0 += (uint32_t)__builtin_popcountll(gmask);
            if (mmask) c_has_m = 1u;
        }
        if (!wr) {
            n_keep = n_ev - tail;
            n_end = lead + tail;
            T.n_a = DL_EVENT_WORDS * n_keep; T.n_b = 0u;
            if (!opl_claim(T, pi, lane, n_end << DL_END_SHIFT, list_words, cursor, recs)) return;
            list_w = lists + T.off;
        }
    }
    T.flags = 1u | (n_end << DL_END_SHIFT);
    if (lane == 0) recs[pi] = T;
}

// One wave per reported alignment: the words of its events go to the store at dst[wi].
__global__ __launch_bounds__(64) void k_dl_keep(uint32_t n, const dl_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                 const uint32_t *__restrict__ host_lists, const uint32_t *__restrict__ dst, uint32_t *__restrict__ store)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const dl_rec rc = recs[wi];
    const uint32_t *ev = ((rc.flags & 3u) == 3u ? host_lists : lists) + rc.off;
    uint32_t *out = store + dst[wi];
    for (uint32_t i = threadIdx.x; i < rc.n_a; i += 64u) out[i] = ev[i];
}

// ------------------------------------------------------------------------------------------------------------------ the call
// the first sort's key of event i: its last base; the payload is the event's index.  *max_len: the longest event (an unsigned
// maximum: no order in it).
__global__ __launch_bounds__(DL_BLOCK) void k_dl_keys(const uint32_t *__restrict__ ev, uint32_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val,
                                                       uint32_t *__restrict__ max_len)
{
    const uint32_t i = blockIdx.x * DL_BLOCK + threadIdx.x;
    uint32_t len = 0;
    if (i < n) {
        key[i] = ev[(size_t)DL_EVENT_WORDS * i + 2];
        val[i] = i;
        len = ev[(size_t)DL_EVENT_WORDS * i + 1];
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) len = max(len, (uint32_t)__shfl_xor((int)len, off));
    // (a wave whose longest is no longer than what is there already adds nothing: the value only grows, so a stale read costs an
    // atomic and never loses one -- 200 000 atomics on one word took 2.4 ms of a 4.6 ms call)
    if ((threadIdx.x & 63u) == 0u && len > *(volatile uint32_t *)max_len) atomicMax(max_len, len);
}

// the second sort's key of place j of the order by last: first << len_bits | len of the event that stands there
__global__ __launch_bounds__(DL_BLOCK) void k_dl_gather(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ val, uint32_t n, uint32_t len_bits,
                                                         uint64_t *__restrict__ key)
{
    const uint32_t j = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t *e = ev + (size_t)DL_EVENT_WORDS * val[j];
    key[j] = ((uint64_t)e[0] << len_bits) | e[1];
}

// head[j] = 1 where the event at place j of the sorted order differs from the one before it
__global__ __launch_bounds__(DL_BLOCK) void k_dl_heads(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ val, uint32_t n, uint64_t *__restrict__ head)
{
    const uint32_t j = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (j >= n) return;
    bool h = j == 0u;
    if (!h) {
        const uint32_t *a = ev + (size_t)DL_EVENT_WORDS * val[j], *b = ev + (size_t)DL_EVENT_WORDS * val[j - 1u];
        h = a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
    }
    head[j] = h ? 1ull : 0ull;
}

// start[g] = the place of the head of group g (gidx: the exclusive scan of head)
__global__ __launch_bounds__(DL_BLOCK) void k_dl_starts(const uint64_t *__restrict__ head, const uint64_t *__restrict__ gidx, uint32_t n, uint32_t *__restrict__ start)
{
    const uint32_t j = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (j < n && head[j]) start[gidx[j]] = j;
}

struct dl_params {
    uint32_t E;
    uint64_t min_depth, min_qual;
};
struct dl_call {
    uint32_t first, len, last, state, qual;
    uint64_t depth, reads;
    bool reported, wide;
};

// group g of n_groups: its event, its size, the depth of its first base from row `first` of the pileup table, the rule
template <typename T>
__device__ __forceinline__ dl_call dl_eval(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ val, const uint32_t *__restrict__ start, uint32_t g,
                                           uint32_t n_groups, uint32_t n, const T *__restrict__ counts, uint32_t n_bases, const dl_params &P)
{
    dl_call c;
    const uint32_t s = start[g], e = g + 1u < n_groups ? start[g + 1u] : n;
    const uint32_t *w = ev + (size_t)DL_EVENT_WORDS * val[s];
    c.first = w[0]; c.len = w[1]; c.last = w[2];
    c.reads = e - s;
    c.depth = 0;
    c.wide = false;
    if (c.first < n_bases) {
        const T *row = counts + (size_t)c.first * PU_COLS;
#pragma unroll
        for (uint32_t k = 0; k < PU_COL_INS; k++) {
            const unsigned long long v = row[k];
            c.wide = c.wide || v >= DL_MAX_COUNT;
            c.depth += v;
        }
    }
    c.state = dl_rule(c.reads, c.depth, P.E, &c.qual);
    c.reported = !c.wide && dl_reported(c.state, c.qual, c.depth, P.min_depth, P.min_qual);
    return c;
}

// A thread per group (n_groups = gidx[n], read on the device): rep[g] = the group is reported; a thread behind the last group
// writes 0.  flags bit 0: a 64-bit counter of DL_MAX_COUNT or more.
template <typename T>
__global__ __launch_bounds__(DL_BLOCK) void k_dl_group(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ val, const uint32_t *__restrict__ start,
                                                        const uint64_t *__restrict__ gidx, uint32_t n, const T *__restrict__ counts, uint32_t n_bases, dl_params P,
                                                        uint64_t *__restrict__ rep, uint32_t *__restrict__ flags)
{
    const uint32_t g = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (g >= n) return;
    const uint32_t n_groups = (uint32_t)gidx[n];
    if (g >= n_groups) { rep[g] = 0ull; return; }
    const dl_call c = dl_eval<T>(ev, val, start, g, n_groups, n, counts, n_bases, P);
    rep[g] = c.reported ? 1ull : 0ull;
    if (sizeof(T) == 8 && c.wide) atomicOr(flags, 1u);
}

// The reported groups evaluate once more and write their call at roff[g] (the exclusive scan of rep), as long as that is below cap.
template <typename T>
__global__ __launch_bounds__(DL_BLOCK) void k_dl_emit(const uint32_t *__restrict__ ev, const uint32_t *__restrict__ val, const uint32_t *__restrict__ start,
                                                       uint32_t n_groups, uint32_t n, const T *__restrict__ counts, uint32_t n_bases, dl_params P,
                                                       const uint64_t *__restrict__ rep, const uint64_t *__restrict__ roff, uint32_t cap,
                                                       uint32_t *__restrict__ out_ev, uint8_t *__restrict__ state, uint32_t *__restrict__ qual,
                                                       unsigned long long *__restrict__ depth_reads)
{
    const uint32_t g = blockIdx.x * DL_BLOCK + threadIdx.x;
    if (g >= n_groups || !rep[g]) return;
    const uint64_t at = roff[g];
    if (at >= cap) return;
    const dl_call c = dl_eval<T>(ev, val, start, g, n_groups, n, counts, n_bases, P);
    out_ev[DL_EVENT_WORDS * at] = c.first;
    out_ev[DL_EVENT_WORDS * at + 1] = c.len;
    out_ev[DL_EVENT_WORDS * at + 2] = c.last;
    state[at] = (uint8_t)c.state;
    qual[at] = c.qual;
    depth_reads[2 * at] = c.depth;
    depth_reads[2 * at + 1] = c.reads;
}

}  // namespace

// The store of a context's index while it is on (vga_dev_index::dl: released with the index, and with the pileup), and the lists
struct dl_state : oplist_state {
    uint32_t *d_words = nullptr;
    uint64_t cap = 0, n_words = 0;
    uint64_t n_end_runs = 0;
    vga_hbuf<uint32_t> h_dst;
    vga_dbuf<uint32_t> d_dst;
    ~dl_state()
    {
        if (d_words) (void)hipFree(d_words);
    }
};

static dl_state *dl_active(vga_ctx *ctx) { return ctx && ctx->index.loaded && ctx->index.pu ? ctx->index.dl.get() : nullptr; }

static void dl_keep_from_ops(oplist_call &lists, uint32_t p, const oplist_ops &o)
{
    std::vector<uint32_t> ev;
    bool in_run = false, has_m = false, before = false;
    uint32_t first = 0, last = 0, len = 0, lead = 0;
    size_t since_m = 0;  // the words of ev behind the last M
    auto close = [&]() {
        if (!in_run) return;
        in_run = false;
        if (!before) { lead++; return; }
        ev.push_back(first); ev.push_back(len); ev.push_back(last);
    };
    oplist_walk_host<false>(o, [&](const oplist_op &k) {
        if (k.cg && k.op == 2) {
            if (!in_run) { in_run = true; before = has_m; first = k.g; len = 0; }
            last = k.g;
            len++;
            return;
        }
        close();
        if (k.op == 0) { has_m = true; since_m = ev.size(); }
    });
    close();
    const uint32_t tail = (uint32_t)((ev.size() - since_m) / DL_EVENT_WORDS);
    ev.resize(since_m);
    lists.keep_host(p, ev, std::vector<uint32_t>(), (lead + tail) << DL_END_SHIFT);
}

// the store makes room for `at` words: it doubles, and what is stored moves on the context's stream
static int dl_store_grow(vga_ctx *ctx, dl_state *dl, uint64_t at)
{
    if (at <= dl->cap) return VGA_OK;
    uint64_t cap = dl->cap ? dl->cap : DL_STORE_EVENTS0 * DL_EVENT_WORDS;
    while (cap < at) cap *= 2;
    cap = std::min<uint64_t>(cap, DL_MAX_WORDS);
    uint32_t *grown = nullptr;
    {
        vga_alloc_urgent urgent;
        if (hipMalloc((void **)&grown, cap * 4) != hipSuccess) {
            (void)hipGetLastError();
            return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_align_batch: the deletion store cannot grow to %llu words: %llu alignments kept", (unsigned long long)cap,
                                 (unsigned long long)dl->n_alignments);
        }
    }
    if (dl->n_words) {
        const hipError_t e = hipMemcpyAsync(grown, dl->d_words, dl->n_words * 4, hipMemcpyDeviceToDevice, ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(grown);
            return vga_set_error(ctx, VGA_ERR_HIP, "vga_align_batch: moving the deletion store: %s", hipGetErrorString(e));
        }
    }
    if (dl->d_words) vga_defer_release(dl->d_words, nullptr, nullptr, 0);
    if (getenv("VGA_TRACE")) fprintf(stderr, "[vga-trace] deletions: the store grows from %llu to %llu words\n", (unsigned long long)dl->cap, (unsigned long long)cap);
    dl->d_words = grown;
    dl->cap = cap;
    return VGA_OK;
}

static int dl_add(vga_ctx *ctx, oplist_state *s, size_t nw)
{
    dl_state *dl = static_cast<dl_state *>(s);
    VGA_HIP_CHECK(ctx, dl->h_dst.reserve(nw));
    VGA_HIP_CHECK(ctx, dl->d_dst.reserve(nw));
    uint64_t at = dl->n_words, ends = 0;
    for (size_t i = 0; i < nw; i++) {
        dl->h_dst.p[i] = (uint32_t)at;
        at += dl->lists.h_win.p[i].n_a;
        ends += dl->lists.h_win.p[i].flags >> DL_END_SHIFT;
        if (at > DL_MAX_WORDS)
            return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_align_batch: the deletion store would pass 2^32 - 1 words: %llu alignments kept",
                                 (unsigned long long)dl->n_alignments);
    }
    int rc = dl_store_grow(ctx, dl, at);
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(dl->d_dst.p, dl->h_dst.p, nw * 4, hipMemcpyHostToDevice, ctx->stream));
    rc = oplist_add_staged(ctx, dl, nw, "k_dl_keep", k_dl_keep, [] { return VGA_OK; }, (const uint32_t *)dl->d_dst.p, dl->d_words);
    if (rc == VGA_OK) { dl->n_words = at; dl->n_end_runs += ends; }
    return rc;
}

const oplist_maker &dl_maker()
{
    static const oplist_maker m = {
        OPLIST_TEXT_DL,
        [](vga_ctx *ctx) -> oplist_state * { return dl_active(ctx); },
        [](vga_ctx *ctx) -> oplist_state * { return dl_active(ctx); },
        &poa_switches::has_del_words, &poa_switches::del_words,
        [](vga_ctx *ctx, oplist_call &lists, const oplist_launch &L) { return oplist_enqueue<false>(ctx, lists, L, "k_dl_events", k_dl_events); },
        dl_keep_from_ops,
        dl_add,
        [](const vga_dev_index &ix) { return ix.seq_length < PU_MAX_SEQ && ix.n_nodes < (1ull << 31); },
        [](vga_ctx *ctx, const char *fn) { return oplist_make(ctx, ctx->index.dl, fn); },
        [](vga_ctx *ctx) { ctx->index.dl.reset(); },
        [](const vga_dev_index &, oplist_state *) { return std::vector<oplist_counter>(); },  // (no counters: the store grows with the events)
        [](oplist_state *s) { static_cast<dl_state *>(s)->n_words = static_cast<dl_state *>(s)->n_end_runs = 0; },
    };
    return m;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_deletion_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    if (ctx->index.loaded && !ctx->index.pu)
        return vga_set_error(ctx, VGA_ERR_ARG, "%s: the pileup is not counted (vga_pileup_begin): the call takes its depth from it", __func__);
    return oplist_begin(ctx, dl_maker(), __func__);
}
extern "C" int vga_deletion_reset(vga_ctx *ctx) { return oplist_reset(ctx, dl_maker(), __func__); }
extern "C" int vga_deletion_end(vga_ctx *ctx) { return oplist_end(ctx, dl_maker()); }

extern "C" int vga_deletion_read(vga_ctx *ctx, uint32_t *events, uint64_t *n_alignments, uint64_t *n_events, uint64_t *n_end_runs)
{
    dl_state *dl = static_cast<dl_state *>(oplist_on(ctx, dl_maker(), __func__));
    if (!dl) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (events && dl->n_words) {
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(events, dl->d_words, dl->n_words * 4, hipMemcpyDeviceToHost, ctx->stream));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n_alignments) *n_alignments = dl->n_alignments;
    if (n_events) *n_events = dl->n_words / DL_EVENT_WORDS;
    if (n_end_runs) *n_end_runs = dl->n_end_runs;
    return VGA_OK;
}

extern "C" uint32_t vga_deletion_state(uint64_t reads, uint64_t depth, uint32_t error, uint32_t *qual)
{
    uint32_t q = 0;
    const uint32_t s = dl_rule(reads, depth, error, &q);
    if (qual) *qual = q;
    return s;
}

namespace {

struct dl_out {
    uint64_t cap;
    uint32_t *first, *len, *last;
    uint8_t *state;
    uint32_t *qual;
    uint64_t *depth, *reads, *n_distinct, *n_calls;
};

uint32_t dl_bits(uint64_t v)  // the bits that hold v, at least one
{
    uint32_t b = 1;
    while (b < 64u && (v >> b)) b++;
    return b;
}

unsigned dl_grid(uint64_t n) { return (unsigned)((n + DL_BLOCK - 1u) / DL_BLOCK); }

// the call over n events and a pileup table of n_bases rows that are on the device; the first min(n_calls, cap) calls go back
template <typename T>
int dl_run(vga_ctx *ctx, const char *who, const uint32_t *d_ev, uint64_t n64, const T *d_counts, uint32_t n_bases, const dl_params &P, const dl_out &o)
{
    hipStream_t st = ctx->stream;
    uint64_t n_distinct = 0, n_calls = 0;
    vga_timers_reset(ctx);
    if (n64) {
        const uint32_t n = (uint32_t)n64;
        ix_build B{ctx, {}, st, who};
        uint64_t *key = B.mem.get<uint64_t>(n), *head = B.mem.get<uint64_t>(n + 1), *gidx = B.mem.get<uint64_t>(n + 1), *rep = B.mem.get<uint64_t>(n + 1),
                 *roff = B.mem.get<uint64_t>(n + 1);
        uint32_t *val = B.mem.get<uint32_t>(n), *start = B.mem.get<uint32_t>(n), *small = B.mem.get<uint32_t>(2);
        if (!key || !head || !gidx || !rep || !roff || !val || !start || !small) return B.nomem("the call", n);
        uint32_t *max_len = small, *flags = small + 1;
        VGA_HIP_CHECK(ctx, hipMemsetAsync(small, 0, 8, st));
        int rc = vga_launch(ctx, "k_dl_keys", (uint64_t)n * 24, k_dl_keys, dim3(dl_grid(n)), dim3(DL_BLOCK), d_ev, n, key, val, max_len);
        if (rc != VGA_OK) return rc;
        uint32_t h_max_len = 0;
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(&h_max_len, max_len, 4, hipMemcpyDeviceToHost, st));
        // two stable rounds: by last, then by (first, len); the digit passes cover the bits the graph and the longest event need
        int t = vga_timer_begin(ctx, "k_dl_sort_last", (uint64_t)n * 24);
        rc = B.radix(key, val, n, dl_bits(n_bases ? n_bases - 1u : 0u));
        vga_timer_end(ctx, t);
        if (rc != VGA_OK) return rc;
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));  // (the longest event)
        const uint32_t len_bits = dl_bits(h_max_len), first_bits = dl_bits(n_bases ? n_bases - 1u : 0u);
        uint64_t *key2 = B.mem.get<uint64_t>(n);
        if (!key2) return B.nomem("the call", n);
        rc = vga_launch(ctx, "k_dl_gather", (uint64_t)n * 24, k_dl_gather, dim3(dl_grid(n)), dim3(DL_BLOCK), d_ev, (const uint32_t *)val, n, len_bits, key2);
        if (rc != VGA_OK) return rc;
        t = vga_timer_begin(ctx, "k_dl_sort_first", (uint64_t)n * 24);
        rc = B.radix(key2, val, n, len_bits + first_bits);
        vga_timer_end(ctx, t);
        if (rc != VGA_OK) return rc;
        rc = vga_launch(ctx, "k_dl_heads", (uint64_t)n * 36, k_dl_heads, dim3(dl_grid(n)), dim3(DL_BLOCK), d_ev, (const uint32_t *)val, n, head);
        if (rc != VGA_OK) return rc;
        t = vga_timer_begin(ctx, "k_dl_scan", (uint64_t)n * 32);
        rc = B.scan(head, n, gidx);
        vga_timer_end(ctx, t);
        if (rc != VGA_OK) return rc;
        rc = vga_launch(ctx, "k_dl_starts", (uint64_t)n * 20, k_dl_starts, dim3(dl_grid(n)), dim3(DL_BLOCK), (const uint64_t *)head, (const uint64_t *)gidx, n, start);
        if (rc == VGA_OK)
            rc = vga_launch(ctx, "k_dl_group", (uint64_t)n * 24, k_dl_group<T>, dim3(dl_grid(n)), dim3(DL_BLOCK), d_ev, (const uint32_t *)val, (const uint32_t *)start,
                            (const uint64_t *)gidx, n, d_counts, n_bases, P, rep, flags);
        if (rc != VGA_OK) return rc;
        t = vga_timer_begin(ctx, "k_dl_scan", (uint64_t)n * 32);
        rc = B.scan(rep, n, roff);
        vga_timer_end(ctx, t);
        if (rc != VGA_OK) return rc;
        uint32_t h_flags = 0;
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(&n_distinct, gidx + n, 8, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(&n_calls, roff + n, 8, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        if (h_flags & 1u) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_WIDE, who);
        const uint64_t m = std::min<uint64_t>(n_calls, o.cap);
        if (m) {
            uint32_t *d_out = B.mem.get<uint32_t>(m * DL_EVENT_WORDS), *d_qual = B.mem.get<uint32_t>(m);
            uint8_t *d_state = B.mem.get<uint8_t>(m);
            unsigned long long *d_dr = B.mem.get<unsigned long long>(2 * m);
            if (!d_out || !d_qual || !d_state || !d_dr) return B.nomem("the calls", m);
            rc = vga_launch(ctx, "k_dl_emit", m * 33, k_dl_emit<T>, dim3(dl_grid(n_distinct)), dim3(DL_BLOCK), d_ev, (const uint32_t *)val, (const uint32_t *)start,
                            (uint32_t)n_distinct, n, d_counts, n_bases, P, (const uint64_t *)rep, (const uint64_t *)roff, (uint32_t)m, d_out, d_state, d_qual, d_dr);
            if (rc != VGA_OK) return rc;
            std::vector<uint32_t> h_out(m * DL_EVENT_WORDS);
            std::vector<unsigned long long> h_dr(2 * m);
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(h_out.data(), d_out, m * DL_EVENT_WORDS * 4, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(h_dr.data(), d_dr, m * 16, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.state, d_state, m, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.qual, d_qual, m * 4, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
            for (uint64_t i = 0; i < m; i++) {
                o.first[i] = h_out[DL_EVENT_WORDS * i]; o.len[i] = h_out[DL_EVENT_WORDS * i + 1]; o.last[i] = h_out[DL_EVENT_WORDS * i + 2];
                o.depth[i] = h_dr[2 * i]; o.reads[i] = h_dr[2 * i + 1];
            }
        }
        vga_timers_collect(ctx);
    }
    if (o.n_distinct) *o.n_distinct = n_distinct;
    if (o.n_calls) *o.n_calls = n_calls;
    return VGA_OK;
}

int dl_check(vga_ctx *ctx, const char *who, uint32_t E, uint64_t min_depth, const dl_out &o)
{
    if (E < VC_MIN_ERROR || E > VC_MAX_ERROR) return vga_set_error(ctx, VGA_ERR_ARG, "%s: error cost %u, %u to %u are served", who, E, VC_MIN_ERROR, VC_MAX_ERROR);
    if (min_depth < 1) return vga_set_error(ctx, VGA_ERR_ARG, "%s: min_depth is at least 1", who);
    if (o.cap && (!o.first || !o.len || !o.last || !o.state || !o.qual || !o.depth || !o.reads))
        return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with cap %llu", who, (unsigned long long)o.cap);
    return VGA_OK;
}

}  // namespace

extern "C" int vga_deletion_call(vga_ctx *ctx, uint32_t E, uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *first, uint32_t *len, uint32_t *last,
                                 uint8_t *state, uint32_t *qual, uint64_t *depth, uint64_t *reads, uint64_t *n_distinct, uint64_t *n_calls)
{
    if (!ctx) return VGA_ERR_ARG;
    const dl_out o = {cap, first, len, last, state, qual, depth, reads, n_distinct, n_calls};
    int rc = dl_check(ctx, __func__, E, min_depth, o);
    if (rc != VGA_OK) return rc;
    dl_state *dl = static_cast<dl_state *>(oplist_on(ctx, dl_maker(), __func__));
    if (!dl) return VGA_ERR_ARG;
    pu_state *pu = pu_active(ctx);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    const uint32_t *table = nullptr;
    uint32_t n_bases = 0;
    if ((rc = pu_finish_device(ctx, pu, __func__, &table, &n_bases)) != VGA_OK) return rc;
    const dl_params P = {E, min_depth, min_qual};
    return dl_run<uint32_t>(ctx, __func__, dl->d_words, dl->n_words / DL_EVENT_WORDS, table, n_bases, P, o);
}

extern "C" int vga_deletion_call_table(vga_ctx *ctx, uint64_t n_events, const uint32_t *events, uint64_t n_bases, const uint64_t *counts, uint32_t E,
                                       uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *first, uint32_t *len, uint32_t *last, uint8_t *state,
                                       uint32_t *qual, uint64_t *depth, uint64_t *reads, uint64_t *n_distinct, uint64_t *n_calls)
{
    if (!ctx) return VGA_ERR_ARG;
    const dl_out o = {cap, first, len, last, state, qual, depth, reads, n_distinct, n_calls};
    int rc = dl_check(ctx, __func__, E, min_depth, o);
    if (rc != VGA_OK) return rc;
    if ((n_events && !events) || (n_bases && !counts)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null table", __func__);
    if (n_events >= DL_MAX_EVENTS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu events, 2^32 - 2 at most", __func__, (unsigned long long)n_events);
    if (n_bases >= VC_MAX_BASES) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu bases, positions are 31-bit", __func__, (unsigned long long)n_bases);
    for (uint64_t i = 0; i < n_events; i++) {
        const uint32_t *e = events + DL_EVENT_WORDS * i;
        if (e[0] >= n_bases || e[2] >= n_bases || e[1] < 1u)
            return vga_set_error(ctx, VGA_ERR_ARG, "%s: event %llu is (%u, %u, %u), the table has %llu bases", __func__, (unsigned long long)i, e[0], e[1], e[2],
                                 (unsigned long long)n_bases);
    }
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vga_dbuf<uint32_t> d_ev;
    vga_dbuf<unsigned long long> d_counts;
    if ((rc = table_upload(ctx, d_ev, events, (size_t)n_events * DL_EVENT_WORDS)) != VGA_OK) return rc;
    if ((rc = table_upload(ctx, d_counts, counts, (size_t)n_bases * PU_COLS)) != VGA_OK) return rc;
    const dl_params P = {E, min_depth, min_qual};
    return dl_run<unsigned long long>(ctx, __func__, d_ev.p, n_events, d_counts.p, (uint32_t)n_bases, P, o);
}
