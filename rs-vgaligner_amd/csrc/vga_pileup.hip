// vga_pileup.hip -- per-base read alleles, deletions and insertions: k_pu_events, k_pu_add, k_pu_finish and the four C entry
// points vga_pileup_begin / _read / _reset / _end.  See vga_pileup.hpp for the shape.
//
// Meaning (include/vga_hip.h): along the reported record of a read, an M operation adds one at its graph base to the column of
// the read's letter (A C G T, anything else N) -- for a match that is the base's own letter --, a D operation one to `del` of its
// base, a run of I operations one to `ins` of the graph base consumed most recently before it (covered or deleted), or to the
// context's leading_ins when no base was consumed yet.  All counters are 32-bit integers added with vector atomics: sums of
// integers do not depend on order, so the table is exact and repeatable.
#include "vga_pileup.hpp"

#include <algorithm>

namespace {

// ---- wave helpers (64 lanes)
// the value of the lane below; lane 0 takes `carry` (the last lane of the previous block)
__device__ __forceinline__ uint32_t pu_shr1(uint32_t v, uint32_t carry, int lane)
{
    const uint32_t t = (uint32_t)__shfl_up((int)v, 1);
    return lane == 0 ? carry : t;
}
// column of a letter: a c g t in either case, anything else N
__host__ __device__ __forceinline__ uint32_t pu_col(char c)
{
    const char l = (char)(c | 0x20);
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : PU_COL_N;
}

// One wave per problem of a finished launch.  Reads the traceback's operations once per pass, forward, 64 at a time (they are
// stored sink -> source), with the graph base and the read base of each (k_poa_text's arithmetic: the query index is a popcount
// over the query-consuming lanes below, and so is the place of a word among those its block writes; a row opens a node exactly when
// its row record has predecessors of its own, every other row takes the offset  position - row  of the latest opening row before
// it).  The list: one event word per end of a run of
// MATCHES on consecutive positions of the linearised graph (position << 1 where it starts, (position behind its last base) << 1 | 1
// where it ends), then one word  position << 3 | column  per mismatch (column of the read's letter), deleted base (del) and run
// of insertions (ins, at the base consumed last before it: the latest graph-consuming lane below, or the one carried from the
// previous block).  A run of insertions with no base before it sets PU_LEADING instead.  Two passes: lengths first, one atomic
// add claims the words, then the words.  ids[2 i] is problem i's index in the subgraph store.
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
    const poa_prob pb = probs[pi];
    const poa_out po = outs[pi];
    pu_rec T = {0u, 0u, 0u, 0u};
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
    const char *bases = seq + pb.seq0;  // row r is bases[r - 1]
    const char *q = queries + pb.q0;
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
    uint32_t *list_w = nullptr;  // the problem's words: T.n_match events, then the sparse words
    const uint64_t below = (1ull << lane) - 1ull, upto = below | (1ull << lane);  // the lanes below this one / up to and including it
    uint32_t leading = 0;
    for (int pass = 0; pass < 2; pass++) {
        const bool wr = pass == 1;
        // carried from block to block: was the last operation a match, its position, the open node's offset; the last operation, the
        // position of the last graph-consuming one and whether there was one; the query bases consumed
        uint32_t c_m = 0, c_g = 0, c_delta = 0, c_op = 3, c_last = 0, c_has = 0, qi0 = 0;
        uint32_t n_mt = 0, n_sp = 0;
        for (uint32_t base = 0; base <= nops; base += 64) {
            const uint32_t f = base + (uint32_t)lane;
            const bool valid = f < nops;
            uint32_t op = 3, row = 0;
            if (valid) { op = op_p[nops - 1 - f]; row = or_p[nops - 1 - f]; }
            const bool cq = valid && (op == 0 || op == 1);
            const bool cg = valid && (op == 0 || op == 2) && row >= 1u && row <= pb.N;
            const uint64_t qmask = __builtin_amdgcn_ballot_w64(cq);
            const uint32_t qi = qi0 + (uint32_t)__builtin_popcountll(qmask & below);
            const char gb = cg ? bases[row - 1] : (char)0, qb = (cq && qi < pb.qlen) ? q[qi] : (char)0;
            // ---- position on the linearised graph
            const bool opens = cg && R[row].npred != 0u;
            uint32_t my_delta = 0;
            if (opens) {
                uint32_t my_id = hd[node_of(row)] >> 1;
                if (my_id < 1u || my_id > n_graph_nodes) my_id = 1u;  // (cannot happen with a store built from this index)
                my_delta = node_start[my_id - 1] - row;
            }
            const uint64_t omask = __builtin_amdgcn_ballot_w64(opens), o_le = omask & upto;
            const uint32_t got = (uint32_t)__shfl((int)my_delta, o_le ? 63 - __builtin_clzll(o_le) : 0);
            const uint32_t g = row + (o_le ? got : c_delta);
            // ---- runs of matches
            const uint32_t is_m = cg && op == 0 && gb == qb ? 1u : 0u;
            const uint32_t p_m = pu_shr1(is_m, c_m, lane), p_g = pu_shr1(g, c_g, lane);
            const bool cont = is_m && p_m && p_g + 1u == g;
            const bool start = is_m && !cont, end = p_m && !cont;
            const uint64_t stmask = __builtin_amdgcn_ballot_w64(start), enmask = __builtin_amdgcn_ballot_w64(end);
            if (wr && (start || end)) {
                uint32_t *w = list_w + n_mt + (uint32_t)(__builtin_popcountll(stmask & below) + __builtin_popcountll(enmask & below));
                if (end) *w++ = ((p_g + 1u) << 1) | 1u;
                if (start) *w = g << 1;
            }
            n_mt += (uint32_t)(__builtin_popcountll(stmask) + __builtin_popcountll(enmask));
            // ---- the sparse operations
            const uint32_t p_op = pu_shr1(op, c_op, lane);
            const bool ins0 = valid && op == 1 && p_op != 1u;  // first operation of a run of insertions
            const uint64_t gmask = __builtin_amdgcn_ballot_w64(cg), g_le = gmask & upto;
            const uint32_t lg = (uint32_t)__shfl((int)g, g_le ? 63 - __builtin_clzll(g_le) : 0);
            const bool has = g_le != 0ull || c_has != 0u;
            const uint32_t at = g_le ? lg : c_last;
            bool sp = false;
            uint32_t word = 0;
            if (cg && op == 0 && !is_m) { sp = true; word = (g << 3) | pu_col(qb); }
            else if (cg && op == 2) { sp = true; word = (g << 3) | PU_COL_DEL; }
            else if (ins0 && has) { sp = true; word = (at << 3) | PU_COL_INS; }
            const uint64_t smask = __builtin_amdgcn_ballot_w64(sp);
            if (wr && sp) list_w[T.n_match + n_sp + (uint32_t)__builtin_popcountll(smask & below)] = word;
            n_sp += (uint32_t)__builtin_popcountll(smask);
            if (__builtin_amdgcn_ballot_w64(ins0 && !has)) leading = PU_LEADING;
            // ---- carries
            c_m = (uint32_t)__builtin_amdgcn_readlane((int)is_m, 63);
            c_g = (uint32_t)__builtin_amdgcn_readlane((int)g, 63);
            if (omask) c_delta = (uint32_t)__shfl((int)my_delta, 63 - __builtin_clzll(omask));
            c_op = (uint32_t)__builtin_amdgcn_readlane((int)op, 63);
            if (gmask) { c_last = (uint32_t)__shfl((int)g, 63 - __builtin_clzll(gmask)); c_has = 1u; }
            qi0 += (uint32_t)__builtin_popcountll(qmask);
        }
        if (!wr) {
            const uint32_t words = n_mt + n_sp;
            unsigned long long at = 0;
            if (lane == 0) at = atomicAdd(cursor, (unsigned long long)words);
            at = (unsigned long long)__shfl((long long)at, 0);
            T.n_match = n_mt; T.n_sparse = n_sp;
            if (at + words > (unsigned long long)list_words) {
                T.flags = 2u | leading;
                if (lane == 0) recs[pi] = T;
                return;
            }
            T.off = (uint32_t)at;
            list_w = lists + at;
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
    const uint32_t *sp = mt + rc.n_match;
    for (uint32_t i = (uint32_t)lane; i < rc.n_match; i += 64) {
        const uint32_t w = mt[i];
        if ((w >> 1) <= seq_length) atomicAdd(mdiff + (w >> 1), (w & 1u) ? 0xFFFFFFFFu : 1u);
    }
    for (uint32_t i = (uint32_t)lane; i < rc.n_sparse; i += 64) {
        const uint32_t w = sp[i];
        if ((w >> 3) < seq_length && (w & 7u) < PU_COLS) atomicAdd(counts + (size_t)(w >> 3) * PU_COLS + (w & 7u), 1u);
    }
}

// out[i][c] = counts[i][c], plus mdiff[0] + ... + mdiff[i] in the column of base i's own letter: one workgroup, a contiguous piece
// per thread, the pieces' sums scanned in LDS.  The counters themselves stay as they are (a read does not reset).
__global__ __launch_bounds__(1024) void k_pu_finish(const uint32_t *__restrict__ mdiff, const uint32_t *__restrict__ counts, const char *__restrict__ seq_fwd,
                                                     uint32_t *__restrict__ out, uint32_t n)
{
    __shared__ uint32_t part[1024];
    const uint32_t tid = threadIdx.x;
    const uint32_t piece = (n + 1023u) / 1024u;
    const uint64_t a64 = (uint64_t)tid * piece, b64 = a64 + piece;
    const uint32_t a = a64 < n ? (uint32_t)a64 : n, b = b64 < n ? (uint32_t)b64 : n;
    uint32_t s = 0;
    for (uint32_t i = a; i < b; i++) s += mdiff[i];
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024u; d <<= 1) {
        const uint32_t t = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += t;
        __syncthreads();
    }
    uint32_t run = tid ? part[tid - 1] : 0u;
    for (uint32_t i = a; i < b; i++) {
        run += mdiff[i];
        const uint32_t own = pu_col(seq_fwd[i]);
        const size_t o = (size_t)i * PU_COLS;
        for (uint32_t c = 0; c < PU_COLS; c++) out[o + c] = counts[o + c] + (c == own ? run : 0u);
    }
}

}  // namespace

// The counters of a context's index while counting is on (vga_dev_index::pu: released with the index), and the lists of the
// vga_align_batch call in progress.
struct pu_state {
    uint32_t seq_length = 0;
    vga_dbuf<uint32_t> d_mdiff, d_counts, d_out;
    uint64_t n_alignments = 0, leading_ins = 0;
    // ---- one call
    vga_dbuf<uint32_t> d_lists;            // the lists k_pu_events writes, claimed through d_cur
    uint32_t list_words = 0;
    vga_dbuf<unsigned long long> d_cur;
    vga_dbuf<pu_rec> d_recs[POA_SLOTS];    // per staged problem of the slot's launch
    vga_hbuf<pu_rec> h_recs[POA_SLOTS][2];
    std::vector<pu_rec> recs;              // per problem of the call
    std::vector<uint32_t> host_lists;      // lists the host built (flags 3)
    vga_dbuf<uint32_t> d_host_lists;
    vga_dbuf<pu_rec> d_win;
    vga_hbuf<pu_rec> h_win;
};

pu_state *pu_active(vga_ctx *ctx) { return ctx && ctx->index.loaded ? (pu_state *)ctx->index.pu : nullptr; }

static void pu_release(vga_ctx *ctx)
{
    if (ctx->index.pu && ctx->index.pu_free) ctx->index.pu_free(ctx->index.pu);
    ctx->index.pu = nullptr;
    ctx->index.pu_free = nullptr;
}

int pu_call_begin(vga_ctx *ctx, pu_state *pu, uint64_t n, uint64_t total_q, bool has_cap, uint64_t cap_words)
{
    // a list holds two words per run of matches and one per mismatch, deleted base and insertion: about 0.4 words per read base
    // with reads of 10 % errors.  Not a bound -- a problem that finds no room says so and the host builds its list
    // (VGA_PILEUP_LIST_WORDS caps the buffer: the tests force that route with it)
    uint64_t words = std::min<uint64_t>(total_q + 256ull * n + 4096ull, 0xFFFFFF00ull);
    if (has_cap) words = std::min<uint64_t>(words, cap_words);
    VGA_HIP_CHECK(ctx, pu->d_lists.reserve(words + 1));
    VGA_HIP_CHECK(ctx, pu->d_cur.reserve(1));
    pu->list_words = (uint32_t)words;
    VGA_HIP_CHECK(ctx, hipMemsetAsync(pu->d_cur.p, 0, sizeof(unsigned long long), ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));  // (the launches' streams do not wait for the context's)
    pu->recs.assign(n, pu_rec{0u, 0u, 0u, 0u});
    pu->host_lists.clear();
    return VGA_OK;
}

hipError_t pu_enqueue_events(vga_ctx *ctx, pu_state *pu, hipStream_t st, int slot, int oset, uint32_t nb, const poa_launch_bufs &b, const uint32_t *ids,
                             const sg_store &store)
{
    hipError_t e;
    if ((e = pu->d_recs[slot].reserve(nb)) != hipSuccess) return e;
    if ((e = pu->h_recs[slot][oset].reserve(nb)) != hipSuccess) return e;
    const int t = vga_timer_begin(ctx, "k_pu_events", 0, st);
    hipLaunchKernelGGL(k_pu_events, dim3(nb), dim3(64), 0, st, nb, b.probs, b.outs, b.ops, b.orow, b.rows, b.ntab, (const char *)b.seq32, b.q, ids,
                       store.d_off, (uint32_t)store.split, store.part[0].d_handles, store.part[1].d_handles, ctx->index.d_node_start,
                       (uint32_t)ctx->index.n_nodes, pu->d_lists.p, pu->list_words, pu->d_cur.p, pu->d_recs[slot].p);
    vga_timer_end(ctx, t);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return hipMemcpyAsync(pu->h_recs[slot][oset].p, pu->d_recs[slot].p, nb * sizeof(pu_rec), hipMemcpyDeviceToHost, st);
}

const pu_rec *pu_launch_recs(const pu_state *pu, int slot, int oset) { return pu->h_recs[slot][oset].p; }

void pu_keep(pu_state *pu, uint32_t p, const pu_rec &r) { pu->recs[p] = r; }

void pu_keep_from_ops(pu_state *pu, uint32_t p, const uint8_t *ops, const uint32_t *orow, uint32_t nops, const uint32_t *first_row, uint32_t n_nodes,
                      const uint32_t *handles, const std::vector<uint32_t> &node_start, const char *bases, uint32_t n_rows, const char *query)
{
    std::vector<uint32_t> ev, sp;
    bool prev_m = false, has = false, leading = false;
    uint32_t pg = 0, v = 0, qi = 0, last = 0, prev_op = 3;
    auto close = [&]() {
        if (prev_m) ev.push_back(((pg + 1) << 1) | 1u);
        prev_m = false;
    };
    for (uint32_t x = nops; x > 0; x--) {
        const uint32_t op = ops[x - 1], r = orow[x - 1];
        if (op == 1) {
            close();
            if (prev_op != 1) {
                if (has) sp.push_back((last << 3) | PU_COL_INS);
                else leading = true;
            }
            qi++;
        } else if ((op == 0 || op == 2) && r >= 1 && r <= n_rows) {
            while (v + 1 < n_nodes && first_row[v + 1] <= r) v++;  // rows ascend along the path
            const uint32_t id = handles[v] >> 1;
            const uint32_t g = node_start[id - 1] + (r - first_row[v]);
            if (op == 0) {
                const char gb = bases[r - 1], qb = query[qi++];
                if (gb == qb) {
                    if (!(prev_m && pg + 1 == g)) { close(); ev.push_back(g << 1); }
                    prev_m = true;
                    pg = g;
                } else {
                    close();
                    sp.push_back((g << 3) | pu_col(qb));
                }
            } else {
                close();
                sp.push_back((g << 3) | PU_COL_DEL);
            }
            has = true;
            last = g;
        } else {
            close();
            if (op == 0) qi++;
        }
        prev_op = op;
    }
    close();
    pu_rec rc = {(uint32_t)pu->host_lists.size(), (uint32_t)ev.size(), (uint32_t)sp.size(), 3u | (leading ? PU_LEADING : 0u)};
    pu->host_lists.insert(pu->host_lists.end(), ev.begin(), ev.end());
    pu->host_lists.insert(pu->host_lists.end(), sp.begin(), sp.end());
    pu->recs[p] = rc;
}

int pu_add_winners(vga_ctx *ctx, pu_state *pu, const std::vector<uint32_t> &winners)
{
    const size_t nw = winners.size();
    if (nw == 0) return VGA_OK;
    VGA_HIP_CHECK(ctx, pu->h_win.reserve(nw));
    VGA_HIP_CHECK(ctx, pu->d_win.reserve(nw));
    uint64_t leading = 0;
    for (size_t i = 0; i < nw; i++) {
        const pu_rec &r = pu->recs[winners[i]];
        if ((r.flags & 3u) != 1u && (r.flags & 3u) != 3u)
            return vga_set_error(ctx, VGA_ERR_HIP, "pileup: reported alignment %zu has no event list (flags %u)", i, r.flags);
        pu->h_win.p[i] = r;
        leading += (r.flags & PU_LEADING) ? 1u : 0u;
    }
    hipStream_t st = ctx->stream;
    VGA_HIP_CHECK(ctx, pu->d_host_lists.reserve(pu->host_lists.size() + 1));
    if (!pu->host_lists.empty())
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(pu->d_host_lists.p, pu->host_lists.data(), pu->host_lists.size() * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(pu->d_win.p, pu->h_win.p, nw * sizeof(pu_rec), hipMemcpyHostToDevice, st));
    const int t = vga_timer_begin(ctx, "k_pu_add", 0, st);
    hipLaunchKernelGGL(k_pu_add, dim3((unsigned)nw), dim3(64), 0, st, (uint32_t)nw, pu->d_win.p, pu->d_lists.p, pu->d_host_lists.p, pu->seq_length,
                       pu->d_mdiff.p, pu->d_counts.p);
    vga_timer_end(ctx, t);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    pu->n_alignments += nw;
    pu->leading_ins += leading;
    vga_timers_collect(ctx);  // (poa_run collected before this launch: once more, with it)
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
static int pu_zero(vga_ctx *ctx, pu_state *pu)
{
    VGA_HIP_CHECK(ctx, hipMemsetAsync(pu->d_mdiff.p, 0, ((size_t)pu->seq_length + 1) * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(pu->d_counts.p, 0, ((size_t)pu->seq_length * PU_COLS + 1) * 4, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    pu->n_alignments = 0;
    pu->leading_ins = 0;
    return VGA_OK;
}

extern "C" int vga_pileup_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_pileup_begin: no index uploaded");
    const vga_dev_index &ix = ctx->index;
    if (ix.seq_length >= PU_MAX_SEQ || ix.n_nodes >= (1ull << 31))
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_pileup_begin: graph too large for 29-bit positions");
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    try {
        if (!ctx->index.pu) {
            ctx->index.pu = new pu_state();
            ctx->index.pu_free = [](void *q) { delete (pu_state *)q; };
        }
    } catch (const std::bad_alloc &) {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_pileup_begin: out of host memory");
    }
    pu_state *pu = (pu_state *)ctx->index.pu;
    pu->seq_length = (uint32_t)ix.seq_length;
    hipError_t e = pu->d_mdiff.reserve((size_t)pu->seq_length + 1);
    if (e == hipSuccess) e = pu->d_counts.reserve((size_t)pu->seq_length * PU_COLS + 1);
    if (e == hipSuccess) e = pu->d_out.reserve((size_t)pu->seq_length * PU_COLS + 1);
    const int rc = e == hipSuccess ? pu_zero(ctx, pu) : vga_set_error(ctx, VGA_ERR_NOMEM, "vga_pileup_begin: %s", hipGetErrorString(e));
    if (rc != VGA_OK) pu_release(ctx);
    return rc;
}

extern "C" int vga_pileup_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    pu_state *pu = pu_active(ctx);
    if (!pu) return vga_set_error(ctx, VGA_ERR_ARG, "vga_pileup_reset: counting is off (vga_pileup_begin)");
    (void)hipSetDevice(ctx->device);
    return pu_zero(ctx, pu);
}

extern "C" int vga_pileup_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    pu_release(ctx);
    return VGA_OK;
}

int pu_finish_device(vga_ctx *ctx, pu_state *pu, const char *who, const uint32_t **table, uint32_t *seq_length)
{
    if (pu->n_alignments >= 0xFFFFFFFFull)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu alignments counted: a 32-bit counter may have wrapped", who,
                             (unsigned long long)pu->n_alignments);
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
    if (!ctx) return VGA_ERR_ARG;
    pu_state *pu = pu_active(ctx);
    if (!pu) return vga_set_error(ctx, VGA_ERR_ARG, "vga_pileup_read: counting is off (vga_pileup_begin)");
    if (pu->n_alignments >= 0xFFFFFFFFull)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_pileup_read: %llu alignments counted: a 32-bit counter may have wrapped",
                             (unsigned long long)pu->n_alignments);
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    if (counts && pu->seq_length) {
        const uint32_t *table = nullptr;
        uint32_t n = 0;
        const int rc = pu_finish_device(ctx, pu, "vga_pileup_read", &table, &n);
        if (rc != VGA_OK) return rc;
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(counts, table, (size_t)n * PU_COLS * 4, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    }
    if (n_alignments) *n_alignments = pu->n_alignments;
    if (leading_ins) *leading_ins = pu->leading_ins;
    return VGA_OK;
}
