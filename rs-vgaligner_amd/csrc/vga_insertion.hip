// vga_insertion.hip -- how long the runs are that reads insert behind a graph base, and their first letters: k_ia_events,
// k_ia_add, k_ia_call and the six C entry points vga_insertion_begin / _read / _reset / _end / _call / _call_table.  See
// vga_insertion.hpp for the shape.
//
// Meaning (include/vga_hip.h): along the reported record of a read, a run of L I operations belongs to the graph base consumed
// most recently before it (covered or deleted), as in the pileup.  It adds one to the base's bin of its length (1 .. 8, or `more`)
// and, for j < min(L, 8), one to the counter of its j-th letter at position j (A C G T, anything else N).  A run with no base
// before it adds one to the context's n_leading.  All counters are 32-bit integers added with vector atomics: sums of integers do
// not depend on order, so the table is exact and repeatable.
#include "vga_insertion.hpp"

namespace {

// code of a letter: a c g t in either case 0 .. 3, anything else N
__host__ __device__ __forceinline__ uint32_t ia_code(char c)
{
    const char l = (char)(c | 0x20);
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : 4u;
}

// the two words of a run of L letters behind the base at `at`; q + q0 is its first letter, and q holds qlen letters
__host__ __device__ __forceinline__ void ia_event(uint32_t at, uint32_t L, const char *q, uint32_t q0, uint32_t qlen, uint32_t &w0, uint32_t &w1)
{
    w0 = (at << 4) | (L < IA_BINS ? L : IA_BINS);
    w1 = 0;
#pragma unroll
    for (uint32_t j = 0; j < IA_MAX_LEN; j++) {
        const bool in = j < L && q0 + j < qlen;
        w1 |= (in ? ia_code(q[q0 + j]) : IA_NO_LETTER) << (3u * j);
    }
}

// One wave per problem of a finished launch.  Walks the traceback's operations twice (vga_oplist.hpp: opl_block, with the query
// base count of each lane) and writes the problem's list: one event per run of I operations that has a graph base before it.  The
// event is emitted at the lane that CLOSES the run -- its own operation is not I, the operation of the lane below (or the one
// carried from the previous block) is -- so that a run may start one, two or three blocks before it ends: the loop runs one virtual
// closing block behind the last operation, whose first invalid lane closes a run that ends the alignment.  Of the closing lane,
//   L        = the query bases consumed before it, minus those before the run's first I: the latest run-start lane below it, or the
//              one carried from the previous blocks (the run that is open at a block's end is the one that started last);
//   at, has  = the latest graph-consuming lane below it, or the carry: I operations consume no graph base, so that is the base
//              the pileup names at the run's first I.
// All carried state is wave-uniform.  A run with no base before it sets PU_LEADING instead.  Two passes: the count first, one
// atomic add claims the words, then the words.
__global__ __launch_bounds__(64) void k_ia_events(uint32_t n, const poa_prob *__restrict__ probs, const poa_out *__restrict__ outs,
                                                   const uint8_t *__restrict__ ops, const uint32_t *__restrict__ orow, const poa_row *__restrict__ rows,
                                                   const uint4 *__restrict__ node_tab, const char *__restrict__ seq, const char *__restrict__ queries,
                                                   const uint32_t *__restrict__ ids, const sg_off *__restrict__ offs, uint32_t split,
                                                   const uint32_t *__restrict__ handles0, const uint32_t *__restrict__ handles1,
                                                   const uint32_t *__restrict__ node_start, uint32_t n_graph_nodes, uint32_t *__restrict__ lists,
                                                   uint32_t list_words, unsigned long long *__restrict__ cursor, ia_rec *__restrict__ recs)
{
    const uint32_t pi = blockIdx.x;
    if (pi >= n) return;
    const int lane = threadIdx.x;
    opl_prob P;
    if (!opl_open<true>(P, pi, lane, probs, outs, ops, orow, rows, node_tab, seq, queries, ids, offs, split, handles0, handles1, node_start,
                        n_graph_nodes, recs))
        return;
    ia_rec T = {0u, 0u, 0u, 0u};
    uint32_t *list_w = nullptr;
    const uint64_t below = opl_below(lane);
    uint32_t leading = 0;
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        opl_carry c;
        // carried from block to block: the last operation, the position of the last graph-consuming one and whether there was
        // one, the query bases consumed before the first I of the run that started last
        uint32_t c_op = 3, c_last = 0, c_has = 0, c_q0 = 0;
        uint32_t n_ev = 0;
        for (uint32_t base = 0; base <= P.nops; base += 64) {
            const opl_lane o = opl_block<true>(P, base, lane, c);
            const uint32_t p_op = opl_shr1(o.op, c_op, lane);
            const bool ins0 = o.valid && o.op == 1 && p_op != 1u;  // first operation of a run of insertions
            const bool closes = o.op != 1u && p_op == 1u;          // (an invalid lane has op 3)
            const uint64_t smask = __builtin_amdgcn_ballot_w64(ins0), s_lt = smask & below;
            const uint32_t q0s = (uint32_t)__shfl((int)o.qi, s_lt ? 63 - __builtin_clzll(s_lt) : 0);
            const uint32_t q0 = s_lt ? q0s : c_q0;
            const uint64_t gmask = __builtin_amdgcn_ballot_w64(o.cg), g_lt = gmask & below;
            const uint32_t lg = (uint32_t)__shfl((int)o.g, g_lt ? 63 - __builtin_clzll(g_lt) : 0);
            const bool has = g_lt != 0ull || c_has != 0u;
            const uint32_t at = g_lt ? lg : c_last;
            const bool emits = closes && has;
            const uint64_t emask = __builtin_amdgcn_ballot_w64(emits);
            if (wr && emits) {
                uint32_t w0, w1;
                ia_event(at, o.qi - q0, P.q, q0, P.qlen, w0, w1);
                uint32_t *w = list_w + IA_EVENT_WORDS * (n_ev + (uint32_t)__builtin_popcountll(emask & below));
                w[0] = w0;
                w[1] = w1;
            }
            n_ev += (uint32_t)__builtin_popcountll(emask);
            if (__builtin_amdgcn_ballot_w64(closes && !has)) leading = PU_LEADING;
            // ---- carries
            c_op = (uint32_t)__builtin_amdgcn_readlane((int)o.op, 63);
            if (smask) c_q0 = (uint32_t)__shfl((int)o.qi, 63 - __builtin_clzll(smask));
            if (gmask) { c_last = (uint32_t)__shfl((int)o.g, 63 - __builtin_clzll(gmask)); c_has = 1u; }
        }
        if (!wr) {
            T.n_a = IA_EVENT_WORDS * n_ev; T.n_b = 0u;
            if (!opl_claim(T, pi, lane, leading, list_words, cursor, recs)) return;
            list_w = lists + T.off;
        }
    }
    T.flags = 1u | leading;
    if (lane == 0) recs[pi] = T;
}

// One wave per reported alignment: its events go into the table, one atomic into the length bin and one per kept letter.  A
// position, a bin or a code the table has no cell for adds nothing.
__global__ __launch_bounds__(64) void k_ia_add(uint32_t n, const ia_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                const uint32_t *__restrict__ host_lists, uint32_t seq_length, uint32_t *__restrict__ counts)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const int lane = threadIdx.x;
    const ia_rec rc = recs[wi];
    const uint32_t *ev = ((rc.flags & 3u) == 3u ? host_lists : lists) + rc.off;
    const uint32_t n_ev = rc.n_a / IA_EVENT_WORDS;
    for (uint32_t i = (uint32_t)lane; i < n_ev; i += 64) {
        const uint32_t w0 = ev[IA_EVENT_WORDS * i], w1 = ev[IA_EVENT_WORDS * i + 1];
        const uint32_t at = w0 >> 4, bin = w0 & 15u;
        if (at >= seq_length || bin < 1u || bin > IA_BINS) continue;
        uint32_t *row = counts + (size_t)at * IA_COLS;
        atomicAdd(row + (bin - 1u), 1u);
#pragma unroll
        for (uint32_t j = 0; j < IA_MAX_LEN; j++) {
            const uint32_t code = (w1 >> (3u * j)) & 7u;
            if (j < bin && code < IA_LETTERS) atomicAdd(row + IA_BINS + j * IA_LETTERS + code, 1u);
        }
    }
}

// A thread per site: the call from row pos[s] of `table` (pos null: from row s).  The longest bin wins the length, the shorter on
// a tie, `more` being the longest; per kept position the most frequent letter, A < C < G < T < N on a tie.  Every loop is
// unrolled, so no count is indexed by a run-time value.  A 64-bit counter of IA_MAX_COUNT or more sets bit 0 of *flags.
template <typename T>
__global__ __launch_bounds__(IA_BLOCK) void k_ia_call(const T *__restrict__ table, const uint32_t *__restrict__ pos, uint32_t n, uint8_t *__restrict__ length,
                                                       unsigned long long *__restrict__ length_reads, uint8_t *__restrict__ seq,
                                                       unsigned long long *__restrict__ seq_reads, unsigned long long *__restrict__ rows_out,
                                                       uint32_t *__restrict__ flags)
{
    const uint32_t s = blockIdx.x * IA_BLOCK + threadIdx.x;
    if (s >= n) return;
    const T *row = table + (size_t)(pos ? pos[s] : s) * IA_COLS;
    unsigned long long top = 0;
    uint32_t len = 0;
    bool wide = false;
#pragma unroll
    for (uint32_t b = 0; b < IA_BINS; b++) {
        const unsigned long long v = row[b];
        wide = wide || v >= IA_MAX_COUNT;
        if (v > top) { top = v; len = b + 1u; }
    }
    length[s] = (uint8_t)len;
    length_reads[s] = top;
#pragma unroll
    for (uint32_t j = 0; j < IA_MAX_LEN; j++) {
        unsigned long long best = 0;
        uint32_t code = 0;
#pragma unroll
        for (uint32_t c = 0; c < IA_LETTERS; c++) {
            const unsigned long long v = row[IA_BINS + j * IA_LETTERS + c];
            wide = wide || v >= IA_MAX_COUNT;
            if (c == 0u || v > best) { best = v; code = c; }
        }
        const bool kept = j < len;
        const char letter = code == 0u ? 'A' : code == 1u ? 'C' : code == 2u ? 'G' : code == 3u ? 'T' : 'N';
        seq[(size_t)s * IA_MAX_LEN + j] = kept ? (uint8_t)letter : (uint8_t)0;
        seq_reads[(size_t)s * IA_MAX_LEN + j] = kept ? best : 0ull;
    }
    if (rows_out) {
#pragma unroll
        for (uint32_t c = 0; c < IA_COLS; c++) rows_out[(size_t)s * IA_COLS + c] = row[c];
    }
    if (sizeof(T) == 8 && wide) atomicOr(flags, 1u);
}

}  // namespace

// The counters of a context's index while counting is on (vga_dev_index::ia: released with the index), and the lists
struct ia_state : oplist_state {
    vga_dbuf<uint32_t> d_counts;
    uint64_t n_events = 0, n_leading = 0;
};

static ia_state *ia_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? ctx->index.ia.get() : nullptr; }

// (the walk hands out the read base of an M only: the lambda counts the query bases itself, operations 0 and 1 consume one)
static void ia_keep_from_ops(oplist_call &lists, uint32_t p, const oplist_ops &o)
{
    std::vector<uint32_t> ev;
    bool has = false, leading = false, in_run = false;
    uint32_t last = 0, qi = 0, q0 = 0;
    auto close = [&]() {
        if (!in_run) return;
        in_run = false;
        if (!has) { leading = true; return; }
        uint32_t w0, w1;
        ia_event(last, qi - q0, o.query, q0, qi, w0, w1);
        ev.push_back(w0);
        ev.push_back(w1);
    };
    oplist_walk_host<true>(o, [&](const oplist_op &k) {
        if (k.op != 1) close();
        else if (!in_run) { in_run = true; q0 = qi; }
        if (k.cg) { has = true; last = k.g; }
        if (k.op == 0 || k.op == 1) qi++;
    });
    close();
    lists.keep_host(p, ev, std::vector<uint32_t>(), leading ? PU_LEADING : 0u);
}

static int ia_add(vga_ctx *ctx, oplist_state *s, size_t nw)
{
    ia_state *ia = static_cast<ia_state *>(s);
    uint64_t leading = 0, events = 0;
    for (size_t i = 0; i < nw; i++) {
        leading += (ia->lists.h_win.p[i].flags & PU_LEADING) ? 1u : 0u;
        events += ia->lists.h_win.p[i].n_a / IA_EVENT_WORDS;
    }
    const int rc = oplist_add_staged(ctx, ia, nw, "k_ia_add", k_ia_add, [] { return VGA_OK; }, ia->seq_length, ia->d_counts.p);
    if (rc == VGA_OK) { ia->n_events += events; ia->n_leading += leading; }
    return rc;
}

const oplist_maker &ia_maker()
{
    static const oplist_maker m = {
        OPLIST_TEXT_IA,
        [](vga_ctx *ctx) -> oplist_state * { return ia_active(ctx); },
        [](vga_ctx *ctx) -> oplist_state * { return ia_active(ctx); },
        &poa_switches::has_ins_words, &poa_switches::ins_words,
        [](vga_ctx *ctx, oplist_call &lists, const oplist_launch &L) { return oplist_enqueue<true>(ctx, lists, L, "k_ia_events", k_ia_events); },
        ia_keep_from_ops,
        ia_add,
        [](const vga_dev_index &ix) { return ix.seq_length < IA_MAX_SEQ && ix.n_nodes < (1ull << 31); },
        [](vga_ctx *ctx, const char *fn) { return oplist_make(ctx, ctx->index.ia, fn); },
        [](vga_ctx *ctx) { ctx->index.ia.reset(); },
        [](const vga_dev_index &, oplist_state *s) { return std::vector<oplist_counter>{{&static_cast<ia_state *>(s)->d_counts, (size_t)s->seq_length * IA_COLS + 1, true}}; },
        [](oplist_state *s) { static_cast<ia_state *>(s)->n_events = static_cast<ia_state *>(s)->n_leading = 0; },
    };
    return m;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_insertion_begin(vga_ctx *ctx) { return oplist_begin(ctx, ia_maker(), __func__); }
extern "C" int vga_insertion_reset(vga_ctx *ctx) { return oplist_reset(ctx, ia_maker(), __func__); }
extern "C" int vga_insertion_end(vga_ctx *ctx) { return oplist_end(ctx, ia_maker()); }

extern "C" int vga_insertion_read(vga_ctx *ctx, uint32_t *counts, uint64_t *n_alignments, uint64_t *n_events, uint64_t *n_leading)
{
    ia_state *ia = static_cast<ia_state *>(oplist_on(ctx, ia_maker(), __func__));
    if (!ia) return VGA_ERR_ARG;
    const int rc = oplist_wrapped(ctx, ia, __func__);
    if (rc != VGA_OK) return rc;
    (void)hipSetDevice(ctx->device);
    if (counts && ia->seq_length) {
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(counts, ia->d_counts.p, (size_t)ia->seq_length * IA_COLS * 4, hipMemcpyDeviceToHost, ctx->stream));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n_alignments) *n_alignments = ia->n_alignments;
    if (n_events) *n_events = ia->n_events;
    if (n_leading) *n_leading = ia->n_leading;
    return VGA_OK;
}

namespace {

struct ia_out {
    uint8_t *length;
    uint64_t *length_reads;
    uint8_t *seq;
    uint64_t *seq_reads, *rows;
};

// k_ia_call over n sites of a table that is on the device (d_pos null: row s is site s), and the calls back to the host
template <typename T>
int ia_run(vga_ctx *ctx, const char *who, const T *d_table, const uint32_t *d_pos, uint64_t n, const ia_out &o)
{
    hipStream_t st = ctx->stream;
    vga_timers_reset(ctx);
    if (n == 0) return VGA_OK;
    vga_dbuf<uint8_t> d_bytes;                // length (n), seq (8 n)
    vga_dbuf<unsigned long long> d_wide;      // length_reads (n), seq_reads (8 n), rows (49 n)
    vga_dbuf<uint32_t> d_flags;
    VGA_HIP_CHECK_OOM(ctx, d_bytes.reserve((size_t)n * (1 + IA_MAX_LEN)));
    VGA_HIP_CHECK_OOM(ctx, d_wide.reserve((size_t)n * (1 + IA_MAX_LEN + (o.rows ? IA_COLS : 0u))));
    VGA_HIP_CHECK_OOM(ctx, d_flags.reserve(1));
    uint8_t *d_len = d_bytes.p, *d_seq = d_bytes.p + n;
    unsigned long long *d_lr = d_wide.p, *d_sr = d_wide.p + n, *d_rows = o.rows ? d_wide.p + n * (1 + IA_MAX_LEN) : nullptr;
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_flags.p, 0, 4, st));
    const int rc = vga_launch(ctx, "k_ia_call", n * (IA_COLS * sizeof(T) + 9 + 8 * 9), k_ia_call<T>, dim3((unsigned)((n + IA_BLOCK - 1u) / IA_BLOCK)), dim3(IA_BLOCK), d_table, d_pos,
                              (uint32_t)n, d_len, d_lr, d_seq, d_sr, d_rows, d_flags.p);
    if (rc != VGA_OK) return rc;
    uint32_t h_flags = 0;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(&h_flags, d_flags.p, 4, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    vga_timers_collect(ctx);
    if (h_flags & 1u) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_WIDE, who);
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.length, d_len, n, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.length_reads, d_lr, n * 8, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.seq, d_seq, n * IA_MAX_LEN, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.seq_reads, d_sr, n * IA_MAX_LEN * 8, hipMemcpyDeviceToHost, st));
    if (o.rows) VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.rows, d_rows, n * IA_COLS * 8, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    return VGA_OK;
}

int ia_check(vga_ctx *ctx, const char *who, uint64_t n, const ia_out &o)
{
    if (n && (!o.length || !o.length_reads || !o.seq || !o.seq_reads)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with %llu sites", who, (unsigned long long)n);
    if (n >= (1ull << 31)) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu sites, 2^31 - 1 at most", who, (unsigned long long)n);
    return VGA_OK;
}

}  // namespace

extern "C" int vga_insertion_call(vga_ctx *ctx, uint64_t n, const uint32_t *pos, uint8_t *length, uint64_t *length_reads, uint8_t *seq, uint64_t *seq_reads,
                                  uint64_t *rows)
{
    if (!ctx) return VGA_ERR_ARG;
    const ia_out o = {length, length_reads, seq, seq_reads, rows};
    int rc = ia_check(ctx, __func__, n, o);
    if (rc != VGA_OK) return rc;
    ia_state *ia = static_cast<ia_state *>(oplist_on(ctx, ia_maker(), __func__));
    if (!ia) return VGA_ERR_ARG;
    if ((rc = oplist_wrapped(ctx, ia, __func__)) != VGA_OK) return rc;
    if (n && !pos) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null positions", __func__);
    for (uint64_t s = 0; s < n; s++)
        if (pos[s] >= ia->seq_length)
            return vga_set_error(ctx, VGA_ERR_ARG, "%s: position %u of site %llu, the graph has %u bases", __func__, pos[s], (unsigned long long)s, ia->seq_length);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    vga_dbuf<uint32_t> d_pos;
    if ((rc = table_upload(ctx, d_pos, pos, (size_t)n)) != VGA_OK) return rc;
    return ia_run<uint32_t>(ctx, __func__, ia->d_counts.p, d_pos.p, n, o);
}

extern "C" int vga_insertion_call_table(vga_ctx *ctx, uint64_t n, const uint64_t *rows_in, uint8_t *length, uint64_t *length_reads, uint8_t *seq,
                                        uint64_t *seq_reads, uint64_t *rows)
{
    if (!ctx) return VGA_ERR_ARG;
    const ia_out o = {length, length_reads, seq, seq_reads, rows};
    int rc = ia_check(ctx, __func__, n, o);
    if (rc != VGA_OK) return rc;
    if (n && !rows_in) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null rows", __func__);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vga_dbuf<unsigned long long> d_rows;
    if ((rc = table_upload(ctx, d_rows, rows_in, (size_t)n * IA_COLS)) != VGA_OK) return rc;
    return ia_run<unsigned long long>(ctx, __func__, d_rows.p, nullptr, n, o);
}
