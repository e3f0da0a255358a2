// vga_pileup.hip -- per-base read alleles, deletions and insertions: k_pu_events, k_pu_add, k_pu_finish and the four C entry
// points vga_pileup_begin / _read / _reset / _end.  See vga_pileup.hpp for the shape.
//
// Meaning (include/vga_hip.h): along the reported record of a read, an M operation adds one at its graph base to the column of
// the read's letter (A C G T, anything else N) -- for a match that is the base's own letter --, a D operation one to `del` of its
// base, a run of I operations one to `ins` of the graph base consumed most recently before it (covered or deleted), or to the
// context's leading_ins when no base was consumed yet.  All counters are 32-bit integers added with vector atomics: sums of
// integers do not depend on order, so the table is exact and repeatable.
#include "vga_pileup.hpp"
#include "vga_phase.hpp"

namespace {

// column of a letter: a c g t in either case, anything else N
__host__ __device__ __forceinline__ uint32_t pu_col(char c)
{
    const char l = (char)(c | 0x20);
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : PU_COL_N;
}

// One wave per problem of a finished launch.  Walks the traceback's operations twice (vga_oplist.hpp: opl_block, with the graph
// base and the read base of each) and writes the problem's list: one event word per end of a run of MATCHES on consecutive
// positions of the linearised graph, then one word  position << 3 | column  per mismatch (column of the read's letter), deleted
// base (del) and run of insertions (ins, at the base consumed last before it: the latest graph-consuming lane below, or the one
// carried from the previous block).  A run of insertions with no base before it sets PU_LEADING instead.  Two passes: lengths
// first, one atomic add claims the words, then the words.
__global__ __launch_bounds__(64) void k_pu_events(uint32_t n, const poa_prob *__restrict__ probs, const poa_out *__restrict__ outs,
                                                   const uint8_t *__restrict__ ops, const uint32_t *__restrict__ orow, const poa_row *__restrict__ rows,
                                                   const uint4 *__restrict__ node_tab, const char *__restrict__ seq, const char *__restrict__ queries,
                                                   const uint32_t *__restrict__ ids, const sg_off *__restrict__ offs, uint32_t split,
                                                   const uint32_t *__restrict__ handles0, const uint32_t *__restrict__ handles1,
                                                   const uint32_t *__restrict__ node_start, uint32_t n_graph_nodes, uint32_t *__restrict__ lists,
                                                   uint32_t list_words, unsigned long long *__restrict__ cursor, pu_rec *__restrict__ recs)
{
    const uint32_t pi = blockIdx.x;
    if (pi >= n) return;
    const int lane = threadIdx.x;
    opl_prob P;
    if (!opl_open<true>(P, pi, lane, probs, outs, ops, orow, rows, node_tab, seq, queries, ids, offs, split, handles0, handles1, node_start,
                        n_graph_nodes, recs))
        return;
    pu_rec T = {0u, 0u, 0u, 0u};
    uint32_t *list_w = nullptr;  // the problem's words: T.n_a events, then the sparse words
    const uint64_t below = opl_below(lane), upto = below | (1ull << lane);  // the lanes below this one / up to and including it
    uint32_t leading = 0;
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        opl_carry c;
        opl_runs runs;
        // carried from block to block: the last operation, the position of the last graph-consuming one and whether there was one
        uint32_t c_op = 3, c_last = 0, c_has = 0;
        uint32_t n_sp = 0;
        for (uint32_t base = 0; base <= P.nops; base += 64) {
            const opl_lane o = opl_block<true>(P, base, lane, c);
            // ---- runs of matches
            const uint32_t is_m = o.cg && o.op == 0 && o.gb == o.qb ? 1u : 0u;
            const opl_runs::cut k = runs.step(is_m, o.g, lane);
            if (wr) k.put(list_w, o.g);
            // ---- the sparse operations
            const uint32_t p_op = opl_shr1(o.op, c_op, lane);
            const bool ins0 = o.valid && o.op == 1 && p_op != 1u;  // first operation of a run of insertions
            const uint64_t gmask = __builtin_amdgcn_ballot_w64(o.cg), g_le = gmask & upto;
            const uint32_t lg = (uint32_t)__shfl((int)o.g, g_le ? 63 - __builtin_clzll(g_le) : 0);
            const bool has = g_le != 0ull || c_has != 0u;
            const uint32_t at = g_le ? lg : c_last;
            bool sp = false;
            uint32_t word = 0;
            if (o.cg && o.op == 0 && !is_m) { sp = true; word = (o.g << 3) | pu_col(o.qb); }
            else if (o.cg && o.op == 2) { sp = true; word = (o.g << 3) | PU_COL_DEL; }
            else if (ins0 && has) { sp = true; word = (at << 3) | PU_COL_INS; }
            const uint64_t smask = __builtin_amdgcn_ballot_w64(sp);
            if (wr && sp) list_w[T.n_a + n_sp + (uint32_t)__builtin_popcountll(smask & below)] = word;
            n_sp += (uint32_t)__builtin_popcountll(smask);
            if (__builtin_amdgcn_ballot_w64(ins0 && !has)) leading = PU_LEADING;
            // ---- carries
            c_op = (uint32_t)__builtin_amdgcn_readlane((int)o.op, 63);
            if (gmask) { c_last = (uint32_t)__shfl((int)o.g, 63 - __builtin_clzll(gmask)); c_has = 1u; }
        }
        if (!wr) {
            T.n_a = runs.n; T.n_b = n_sp;
            if (!opl_claim(T, pi, lane, leading, list_words, cursor, recs)) return;
            list_w = lists + T.off;
        }
    }
    T.flags = 1u | leading;
    if (lane == 0) recs[pi] = T;
}

// One wave per reported alignment: its list goes into the counters.  Per event of a run of matches +1 or -1 into the difference
// array of match depth (seq_length + 1 words), per sparse word +1 into its cell of the table.  Nine tenths of the operations are
// matches, and 10 000 reads on 22 595 graph bases would put them all on the same few hundred lines: they cost two atomics per run,
// and only the mismatches, deleted bases and insertions one each.
__global__ __launch_bounds__(64) void k_pu_add(uint32_t n, const pu_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                const uint32_t *__restrict__ host_lists, uint32_t seq_length, uint32_t *__restrict__ mdiff,
                                                uint32_t *__restrict__ counts)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const int lane = threadIdx.x;
    const pu_rec rc = recs[wi];
    const uint32_t *mt = ((rc.flags & 3u) == 3u ? host_lists : lists) + rc.off;
    const uint32_t *sp = mt + rc.n_a;
    for (uint32_t i = (uint32_t)lane; i < rc.n_a; i += 64) {
        const uint32_t w = mt[i];
        if ((w >> 1) <= seq_length) atomicAdd(mdiff + (w >> 1), (w & 1u) ? 0xFFFFFFFFu : 1u);
    }
    for (uint32_t i = (uint32_t)lane; i < rc.n_b; i += 64) {
        const uint32_t w = sp[i];
        if ((w >> 3) < seq_length && (w & 7u) < PU_COLS) atomicAdd(counts + (size_t)(w >> 3) * PU_COLS + (w & 7u), 1u);
    }
}

// out[i][c] = counts[i][c], plus mdiff[0] + ... + mdiff[i] in the column of base i's own letter: one workgroup, a contiguous piece
// per thread (opl_block_scan).  The counters themselves stay as they are (a read does not reset).
__global__ __launch_bounds__(1024) void k_pu_finish(const uint32_t *__restrict__ mdiff, const uint32_t *__restrict__ counts, const char *__restrict__ seq_fwd,
                                                     uint32_t *__restrict__ out, uint32_t n)
{
    uint32_t a, b;
    uint32_t run = opl_block_scan(mdiff, n, a, b);
    for (uint32_t i = a; i < b; i++) {
        run += mdiff[i];
        const uint32_t own = pu_col(seq_fwd[i]);
        const size_t o = (size_t)i * PU_COLS;
        for (uint32_t c = 0; c < PU_COLS; c++) out[o + c] = counts[o + c] + (c == own ? run : 0u);
    }
}

}  // namespace

// The counters of a context's index while counting is on (vga_dev_index::pu: released with the index), and the lists
struct pu_state : oplist_state {
    vga_dbuf<uint32_t> d_mdiff, d_counts, d_out;
    uint64_t leading_ins = 0;
};

pu_state *pu_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? ctx->index.pu.get() : nullptr; }

static void pu_keep_from_ops(oplist_call &lists, uint32_t p, const oplist_ops &o)
{
    std::vector<uint32_t> sp;
    oplist_runs_host runs;
    bool has = false, leading = false;
    uint32_t last = 0, prev_op = 3;
    oplist_walk_host<true>(o, [&](const oplist_op &k) {
        const bool match = k.cg && k.op == 0 && k.gb == k.qb;
        runs.step(match, k.g);
        if (k.op == 1 && prev_op != 1) {
            if (has) sp.push_back((last << 3) | PU_COL_INS);
            else leading = true;
        }
        if (k.cg) {
            if (k.op == 2) sp.push_back((k.g << 3) | PU_COL_DEL);
            else if (!match) sp.push_back((k.g << 3) | pu_col(k.qb));
            has = true;
            last = k.g;
        }
        prev_op = k.op;
    });
    runs.close();
    lists.keep_host(p, runs.ev, sp, leading ? PU_LEADING : 0u);
}

static int pu_add(vga_ctx *ctx, oplist_state *s, size_t nw)
{
    pu_state *pu = static_cast<pu_state *>(s);
    uint64_t leading = 0;
    for (size_t i = 0; i < nw; i++) leading += (pu->lists.h_win.p[i].flags & PU_LEADING) ? 1u : 0u;
    // the phase store keeps the lists that were just staged (vga_phase.hpp), behind k_pu_add on the same stream
    const auto keep = [&]() { ph_state *ph = ph_active(ctx); return ph ? ph_keep_winners(ctx, ph, pu->lists, nw) : VGA_OK; };
    const int rc = oplist_add_staged(ctx, pu, nw, "k_pu_add", k_pu_add, keep, pu->seq_length, pu->d_mdiff.p, pu->d_counts.p);
    if (rc == VGA_OK) pu->leading_ins += leading;
    return rc;
}

static std::vector<oplist_counter> pu_counters(const vga_dev_index &, oplist_state *s)
{
    pu_state *pu = static_cast<pu_state *>(s);
    const size_t cells = (size_t)pu->seq_length * PU_COLS + 1;
    return {{&pu->d_mdiff, (size_t)pu->seq_length + 1, true}, {&pu->d_counts, cells, true}, {&pu->d_out, cells, false}};
}

const oplist_maker &pu_maker()
{
    static const oplist_maker m = {
        OPLIST_TEXT_PU,
        [](vga_ctx *ctx) -> oplist_state * { return pu_active(ctx); },
        [](vga_ctx *ctx) -> oplist_state * { return pu_active(ctx); },
        &poa_switches::has_pileup_words, &poa_switches::pileup_words,
        [](vga_ctx *ctx, oplist_call &lists, const oplist_launch &L) { return oplist_enqueue<true>(ctx, lists, L, "k_pu_events", k_pu_events); },
        pu_keep_from_ops,
        pu_add,
        [](const vga_dev_index &ix) { return ix.seq_length < PU_MAX_SEQ && ix.n_nodes < (1ull << 31); },
        [](vga_ctx *ctx, const char *fn) { return oplist_make(ctx, ctx->index.pu, fn); },
        // (the phase store keeps the pileup's lists and the deletion call takes its depth from the table: they end with it)
        [](vga_ctx *ctx) { ctx->index.ph.reset(); ctx->index.dl.reset(); ctx->index.pu.reset(); },
        pu_counters,
        [](oplist_state *s) { static_cast<pu_state *>(s)->leading_ins = 0; },
    };
    return m;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_pileup_begin(vga_ctx *ctx) { return oplist_begin(ctx, pu_maker(), __func__); }
extern "C" int vga_pileup_reset(vga_ctx *ctx) { return oplist_reset(ctx, pu_maker(), __func__); }
extern "C" int vga_pileup_end(vga_ctx *ctx) { return oplist_end(ctx, pu_maker()); }

int pu_finish_device(vga_ctx *ctx, pu_state *pu, const char *who, const uint32_t **table, uint32_t *seq_length)
{
    const int rc = oplist_wrapped(ctx, pu, who);
    if (rc != VGA_OK) return rc;
    if (pu->seq_length) {
        hipLaunchKernelGGL(k_pu_finish, dim3(1), dim3(1024), 0, ctx->stream, pu->d_mdiff.p, pu->d_counts.p, ctx->index.d_seq_fwd, pu->d_out.p, pu->seq_length);
        VGA_HIP_CHECK(ctx, hipGetLastError());
    }
    *table = pu->d_out.p;
    *seq_length = pu->seq_length;
    return VGA_OK;
}

extern "C" int vga_pileup_read(vga_ctx *ctx, uint32_t *counts, uint64_t *n_alignments, uint64_t *leading_ins)
{
    pu_state *pu = static_cast<pu_state *>(oplist_on(ctx, pu_maker(), __func__));
    if (!pu) return VGA_ERR_ARG;
    int rc = oplist_wrapped(ctx, pu, __func__);  // (also without a table to read)
    if (rc != VGA_OK) return rc;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (counts && pu->seq_length) {
        const uint32_t *table = nullptr;
        uint32_t n = 0;
        if ((rc = pu_finish_device(ctx, pu, __func__, &table, &n)) != VGA_OK) return rc;
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(counts, table, (size_t)n * PU_COLS * 4, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (n_alignments) *n_alignments = pu->n_alignments;
    if (leading_ins) *leading_ins = pu->leading_ins;
    return VGA_OK;
}
