// vga_index.hip -- the k-mer half of Index::build on the device (vga_index_build_kmers).
//
//   generate_kmers_parallel ... src/kmer.rs:277-505   k_ix_count / k_ix_emit (one work item per handle-orientation and
//                                                     start offset, a two-pass count -> exclusive scan -> emit)
//   stable sort + dedup ....... src/kmer.rs:816-828   k_ix_radix_* (stable LSD radix, 8-bit digits) + k_ix_dedup
//   generate_pos_on_ref_2 ..... src/kmer.rs:816-928   k_ix_radix_* on (start_orient, start, end_orient, end), then by
//                                                     k-mer; k_ix_groups writes the position table, k_ix_probe_* the
//                                                     direct-address probe tables vga_index_upload builds on the host
//
// The host builder (host/vgh_index.cpp: kmers_from_handle, Index::build) fixes the semantics; the emission order argument
// is in DESIGN.md ("The index build on the GPU").
#include "vga_common.hpp"
#include "vga_sort_scan.hpp"  // k_ix_scan_*, k_ix_radix_* and ix_build

#include <algorithm>

namespace {

constexpr int IX_NT = 128;           // walk kernels: threads per block (the DFS stacks live in LDS)
constexpr int IX_LEVELS = 16;        // DFS levels: every level adds >= 1 base, so at most k - 1 <= 14 are ever in use
constexpr uint32_t IX_VISIT_CAP = 1u << 22;  // DFS steps one work item may take before the build reports VGA_ERR_NOMEM

struct ix_graph {
    const char *seq;
    const uint32_t *node_start, *edge_idx, *edges_to, *edges;
    uint32_t n_nodes, L, k;
    uint64_t max_furc, max_deg;
};

struct ix_flags {
    uint32_t blown;      // some work item exceeded IX_VISIT_CAP
    uint32_t blown_item;
};

// 0..3 = A C G T, 4 = N (the host validated seq_fwd: only upper-case A C G T N occur)
__device__ __forceinline__ uint32_t ix_code(char c)
{
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : 4u;
}

// Appends `m` bases of handle (node n, orientation rev) from offset o to key; false when one of them is N.
__device__ __forceinline__ bool ix_bases(const ix_graph &g, uint32_t n, bool rev, uint32_t o, uint32_t m, uint32_t &key)
{
    const uint32_t s = g.node_start[n], len = g.node_start[n + 1] - s;
    bool ok = true;
    for (uint32_t t = 0; t < m; t++) {
        uint32_t c = rev ? ix_code(g.seq[s + len - 1 - (o + t)]) : ix_code(g.seq[s + o + t]);
        if (c == 4u) ok = false;
        c = rev ? 3u - c : c;
        key = (key << 2) | (c & 3u);
    }
    return ok;
}

// HashGraph::neighbors(h, Direction::Right) as a slice of edges: forward handles read the node's right list,
// reverse handles the flips of its left list (in that order).
__device__ __forceinline__ void ix_right(const ix_graph &g, uint32_t h, uint32_t &first, uint32_t &cnt)
{
    const uint32_t n = (h >> 1) - 1, e0 = g.edge_idx[n], to = g.edges_to[n];
    if (h & 1u) { first = e0; cnt = to; }
    else { first = e0 + to; cnt = g.edge_idx[n + 1] - e0 - to; }
}

// seq_pos (src/kmer.rs:752-770): where the handle's sequence starts on its strand
__device__ __forceinline__ uint32_t ix_seq_pos(const ix_graph &g, uint32_t h)
{
    const uint32_t n = (h >> 1) - 1, s = g.node_start[n], len = g.node_start[n + 1] - s;
    return (h & 1u) ? g.L - s - len : s;
}

// Work item t of [0, 2L): node n, orientation, index j inside the handle-orientation's [0, len) items.
__device__ __forceinline__ void ix_item(const ix_graph &g, uint64_t t, uint32_t &n, bool &rev, uint32_t &j, uint32_t &len)
{
    const uint32_t pos = (uint32_t)(t >> 1);  // node_start[n] <= t / 2 < node_start[n + 1] for t in node n's 2 * len items
    uint32_t lo = 0, hi = g.n_nodes;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (g.node_start[mid] <= pos) lo = mid; else hi = mid;
    }
    n = lo;
    const uint32_t s = g.node_start[n];
    len = g.node_start[n + 1] - s;
    const uint64_t local = t - 2ull * s;
    rev = local >= len;
    j = (uint32_t)(rev ? local - len : local);
}

struct ix_emit_out {
    const uint64_t *off;  // exclusive scan of the counts
    uint64_t *key;        // 2-bit packed k-mer
    uint32_t *val;        // emission index (the identity: the sort's payload)
    uint32_t *a, *b;      // start | start_orient << 31, end | end_orient << 31
    uint8_t *forks;
};

// The records one work item contributes, in the host's emission order: j < len - k + 1 is the in-node k-mer
// at offset i = j; the others are the start offsets i = len - 1 - (j - n_complete), i descending, each followed by its DFS
// over the neighbours in reverse order -- the order the host's LIFO stack pops them in.
template <bool EMIT>
__device__ uint64_t ix_walk(const ix_graph &g, uint64_t t, uint8_t *disc, ix_flags *flags, const ix_emit_out &o)
{
    __shared__ uint32_t s_first[IX_LEVELS][IX_NT], s_key[IX_LEVELS][IX_NT], s_rem[IX_LEVELS][IX_NT], s_meta[IX_LEVELS][IX_NT];
    const int tid = threadIdx.x;
    uint32_t n, j, len;
    bool rev;
    ix_item(g, t, n, rev, j, len);
    const uint32_t h = ((n + 1) << 1) | (rev ? 1u : 0u), ho = 2 * n + (rev ? 1u : 0u);
    if (EMIT && disc[ho]) return 0;
    uint32_t f0, c0;
    ix_right(g, h, f0, c0);
    if ((uint64_t)c0 > g.max_deg) return 0;  // kmer.rs:361-372: the handle-orientation emits nothing
    const uint32_t k = g.k, n_complete = len >= k ? len - k + 1 : 0;
    uint64_t base = EMIT ? o.off[t] : 0;
    const uint32_t hpos = ix_seq_pos(g, h), so = rev ? 0x80000000u : 0u;
    if (j < n_complete) {
        uint32_t key = 0;
        if (!ix_bases(g, n, rev, j, k, key)) { disc[ho] = 1; return 0; }  // kmer.rs:401-403
        if (EMIT) {
            o.key[base] = key;
            o.val[base] = (uint32_t)base;
            o.a[base] = (hpos + j) | so;
            o.b[base] = (hpos + j + k) | so;
            o.forks[base] = 0;
        }
        return 1;
    }
    const uint32_t i = len - 1 - (j - n_complete), cur0 = len - i;
    uint32_t key0 = 0;
    if (!ix_bases(g, n, rev, i, cur0, key0)) { disc[ho] = 1; return 0; }
    if (!((uint64_t)c0 < g.max_deg || 0 < g.max_furc) || c0 == 0) return 0;
    // level = one incomplete k-mer whose children are still to be popped: its first edge, key, children left, and
    // meta = bases | forks << 8 | (children > 1) << 16 | (its handle is reverse) << 17
    uint64_t count = 0;
    uint32_t visits = 0;
    int lv = 0;
    s_first[0][tid] = f0;
    s_key[0][tid] = key0;
    s_rem[0][tid] = c0;
    s_meta[0][tid] = cur0 | ((c0 > 1 ? 1u : 0u) << 16) | ((rev ? 1u : 0u) << 17);
    while (lv >= 0) {
        uint32_t rem = s_rem[lv][tid];
        if (rem == 0) { lv--; continue; }
        rem--;
        s_rem[lv][tid] = rem;
        const uint32_t meta = s_meta[lv][tid];
        const uint32_t child = g.edges[s_first[lv][tid] + rem] ^ ((meta >> 17) & 1u);
        const uint32_t cur = meta & 0xFFu, forks = ((meta >> 8) & 0xFFu) + ((meta >> 16) & 1u);
        const uint32_t cn = (child >> 1) - 1, clen = g.node_start[cn + 1] - g.node_start[cn];
        const uint32_t take = min(k - cur, clen);
        uint32_t key = s_key[lv][tid];
        if (!ix_bases(g, cn, (child & 1u) != 0, 0, take, key)) { disc[ho] = 1; return count; }  // kmer.rs:459-461
        if (++visits > IX_VISIT_CAP) {
            flags->blown = 1;
            flags->blown_item = (uint32_t)t;
            return count;
        }
        if (cur + take == k) {
            if (EMIT) {
                const uint64_t e = base + count;
                o.key[e] = key;
                o.val[e] = (uint32_t)e;
                o.a[e] = (hpos + i) | so;
                o.b[e] = (ix_seq_pos(g, child) + take) | ((child & 1u) << 31);
                o.forks[e] = (uint8_t)forks;
            }
            count++;
            continue;
        }
        uint32_t cf, cc;
        ix_right(g, child, cf, cc);
        if (cc == 0 || !((uint64_t)cc < g.max_deg || (uint64_t)forks < g.max_furc) || lv + 1 >= IX_LEVELS) continue;
        lv++;
        s_first[lv][tid] = cf;
        s_key[lv][tid] = key;
        s_rem[lv][tid] = cc;
        s_meta[lv][tid] = (cur + take) | (forks << 8) | ((cc > 1 ? 1u : 0u) << 16) | ((child & 1u) << 17);
    }
    return count;
}

__global__ __launch_bounds__(IX_NT) void k_ix_count(ix_graph g, uint64_t n_items, uint64_t *counts, uint8_t *disc, ix_flags *flags)
{
    const uint64_t t = (uint64_t)blockIdx.x * IX_NT + threadIdx.x;
    if (t >= n_items) return;
    counts[t] = ix_walk<false>(g, t, disc, flags, ix_emit_out());
}

// Any N visited discards the whole handle-orientation (kmer.rs:401-403, 459-461): its items count nothing.
__global__ void k_ix_mask(ix_graph g, uint64_t n_items, uint64_t *counts, const uint8_t *disc)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_items) return;
    uint32_t n, j, len;
    bool rev;
    ix_item(g, t, n, rev, j, len);
    if (disc[2 * n + (rev ? 1u : 0u)]) counts[t] = 0;
}

__global__ __launch_bounds__(IX_NT) void k_ix_emit(ix_graph g, uint64_t n_items, uint8_t *disc, ix_flags *flags, ix_emit_out o)
{
    const uint64_t t = (uint64_t)blockIdx.x * IX_NT + threadIdx.x;
    if (t >= n_items) return;
    (void)ix_walk<true>(g, t, disc, flags, o);
}


// ---------------------------------------------------------------- dedup, position order, output
// keep[p]: record p of the key-sorted order differs from its predecessor in some field (Vec::dedup, kmer.rs:828).
// (start, start_orient) <-> (first handle, begin offset) and (end, end_orient) <-> (last handle, end offset) are
// one-to-one (offsets < node length, resp. in [1, node length]), and handle_orient is the first handle's orientation.
__global__ void k_ix_dedup(const uint64_t *skey, const uint32_t *sval, uint64_t n, const uint32_t *a, const uint32_t *b,
                           const uint8_t *forks, uint64_t *keep)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    bool k = true;
    if (p > 0 && skey[p] == skey[p - 1]) {
        const uint32_t x = sval[p], y = sval[p - 1];
        k = a[x] != a[y] || b[x] != b[y] || forks[x] != forks[y];
    }
    keep[p] = k ? 1 : 0;
}

// survivors: their emission index and the (start_orient, start, end_orient, end) sort key, `pb` bits per coordinate
__global__ void k_ix_compact(const uint32_t *sval, uint64_t n, const uint64_t *keep_off, const uint32_t *a, const uint32_t *b,
                             uint32_t pb, uint64_t *pkey, uint32_t *pval)
{
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n || keep_off[p + 1] == keep_off[p]) return;
    const uint64_t s = keep_off[p];
    const uint32_t e = sval[p], x = a[e], y = b[e];
    const uint64_t st = ((uint64_t)(x >> 31) << pb) | (x & 0x7FFFFFFFu), en = ((uint64_t)(y >> 31) << pb) | (y & 0x7FFFFFFFu);
    pkey[s] = (st << (pb + 1)) | en;
    pval[s] = e;
}

__global__ void k_ix_gather_key(const uint32_t *pval, uint64_t n, const uint64_t *key, uint64_t *out)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < n) out[q] = key[pval[q]];
}

__global__ void k_ix_heads(const uint64_t *fkey, const uint32_t *fval, uint64_t n, const uint32_t *a, const uint32_t *b,
                           uint64_t *head, uint64_t *ff)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    head[q] = (q == 0 || fkey[q] != fkey[q - 1]) ? 1 : 0;
    const uint32_t e = fval[q];
    ff[q] = ((a[e] | b[e]) >> 31) ? 0 : 1;
}

// The position table: record q of group g at q + g, the delimiter {UINT64_MAX, UINT64_MAX, 1, 1} after each group
// (src/kmer.rs:740-749), kmer_starts[g] = head + g, the keys unpacked to characters.  Three u64 words per vga_kmerpos:
// the padding bytes are zero.
__global__ void k_ix_groups(const uint64_t *fkey, const uint32_t *fval, uint64_t n, uint32_t k, const uint32_t *a, const uint32_t *b,
                            const uint64_t *head, const uint64_t *head_off, uint64_t *table3, uint64_t *kmer_starts, char *kmer_keys,
                            uint64_t *ghead, uint64_t *gend)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint64_t g = head_off[q] + head[q] - 1;
    const uint32_t e = fval[q], x = a[e], y = b[e];
    uint64_t *r = table3 + 3 * (q + g);
    r[0] = x & 0x7FFFFFFFu;
    r[1] = y & 0x7FFFFFFFu;
    r[2] = (uint64_t)(x >> 31) | ((uint64_t)(y >> 31) << 8);
    if (head[q]) {
        ghead[g] = q;
        kmer_starts[g] = q + g;
        const uint64_t key = fkey[q];
        for (uint32_t t = 0; t < k; t++) kmer_keys[g * k + t] = "ACGT"[(key >> (2 * (k - 1 - t))) & 3u];
    }
    if (q + 1 == n || head[q + 1]) {
        gend[g] = q + 1;
        uint64_t *dl = table3 + 3 * (q + g + 1);
        dl[0] = UINT64_MAX;
        dl[1] = UINT64_MAX;
        dl[2] = 1u | (1u << 8);
    }
}

// forward/forward records per group -> header words (count + 1, or 0 when the group has none: a forward probe misses)
__global__ void k_ix_probe_count(const uint64_t *ghead, const uint64_t *gend, uint64_t n_groups, const uint64_t *ff_off,
                                 uint64_t *words)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint64_t c = ff_off[gend[g]] - ff_off[ghead[g]];
    words[g] = c ? c + 1 : 0;
}

// vga_dev_index's tables (vga_ctx.hip, vga_index_upload_impl): table[key] = header index, pos[h] = {count, 0}, then the
// records in table order.  `all`: every record with the orientations in bit 31, header at head + g.
__global__ void k_ix_probe_headers(const uint64_t *fkey, const uint64_t *ghead, const uint64_t *gend, uint64_t n_groups,
                                   const uint64_t *ff_off, const uint64_t *words_off, uint32_t *table, uint2 *pos,
                                   uint32_t *table_all, uint2 *pos_all)
{
    const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    const uint64_t h0 = ghead[g], h1 = gend[g], key = fkey[h0];
    const uint64_t c = ff_off[h1] - ff_off[h0];
    if (c) {
        table[key] = (uint32_t)words_off[g];
        pos[words_off[g]] = make_uint2((uint32_t)c, 0u);
    }
    if (table_all) {
        table_all[key] = (uint32_t)(h0 + g);
        pos_all[h0 + g] = make_uint2((uint32_t)(h1 - h0), 0u);
    }
}

__global__ void k_ix_probe_records(const uint32_t *fval, uint64_t n, const uint32_t *a, const uint32_t *b, const uint64_t *head,
                                   const uint64_t *head_off, const uint64_t *ghead, const uint64_t *ff, const uint64_t *ff_off,
                                   const uint64_t *words_off, uint2 *pos, uint2 *pos_all)
{
    const uint64_t q = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const uint64_t g = head_off[q] + head[q] - 1;
    const uint32_t e = fval[q], x = a[e], y = b[e];
    if (ff[q]) pos[words_off[g] + 1 + (ff_off[q] - ff_off[ghead[g]])] = make_uint2(x, y);
    if (pos_all) pos_all[q + g + 1] = make_uint2(x, y);
}

// ---------------------------------------------------------------- host side
bool ix_acgtn(char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N'; }

// every index the kernels follow is checked here, before anything is launched
int ix_validate(vga_ctx *ctx, const vga_index_desc *d)
{
    if (d->kmer_length == 0 || d->kmer_length > 15)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED,
                             "kmer_length %u: the k-mer walk on the GPU supports 1..15; the host builder handles k-mers of up to %d bases "
                             "(vgh_index_build, `vgaligner index` without --device)",
                             d->kmer_length, VGA_MAX_KMER_LENGTH);
    if (d->seq_length >= (1ull << 31) || d->n_nodes >= (1ull << 30) || d->n_edges >= (1ull << 31))
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "graph too large for 32-bit device coordinates");
    if (!d->seq_fwd || !d->node_seq_idx || !d->node_edge_idx || !d->node_edges_to || (!d->edges && d->n_edges) || d->n_nodes == 0)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: null array or no node in vga_index_desc");
    for (uint64_t i = 0; i < d->seq_length; i++)
        if (!ix_acgtn(d->seq_fwd[i]))
            return vga_set_error(ctx, VGA_ERR_UNSUPPORTED,
                                 "base %llu of the graph (0x%02x) is outside upper-case A/C/G/T/N; the 2-bit key cannot order it",
                                 (unsigned long long)i, (unsigned)(unsigned char)d->seq_fwd[i]);
    const uint64_t n = d->n_nodes;
    if (d->node_seq_idx[0] != 0 || d->node_seq_idx[n] != d->seq_length || d->node_edge_idx[0] != 0 || d->node_edge_idx[n] != d->n_edges)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: NodeRef bounds do not match seq_length / n_edges");
    for (uint64_t i = 0; i < n; i++) {
        if (d->node_seq_idx[i + 1] <= d->node_seq_idx[i])
            return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "node %llu has an empty sequence", (unsigned long long)(i + 1));
        if (d->node_edge_idx[i + 1] < d->node_edge_idx[i] || d->node_edges_to[i] > d->node_edge_idx[i + 1] - d->node_edge_idx[i])
            return vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: edge ranges of node %llu are not monotone", (unsigned long long)(i + 1));
    }
    for (uint64_t e = 0; e < d->n_edges; e++)
        if ((d->edges[e] >> 1) < 1 || (d->edges[e] >> 1) > n)
            return vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: edge %llu names a missing node", (unsigned long long)e);
    return VGA_OK;
}

int ix_build_impl(vga_ctx *ctx, vga_index_desc *d, uint64_t max_furc, uint64_t max_deg)
{
    if (int rc = ix_validate(ctx, d)) return rc;
    vga_index_release(ctx->index);
    vga_timers_reset(ctx);
    if (int rc = vga_index_load_graph(ctx, d)) return rc;
    vga_dev_index &ix = ctx->index;
    ix.k = d->kmer_length;
    ix_build B{ctx, {}, ctx->stream};
    hipStream_t st = ctx->stream;
    const uint32_t k = d->kmer_length;
    ix_graph g{ix.d_seq_fwd, ix.d_node_start, ix.d_edge_idx, ix.d_edges_to, ix.d_edges, (uint32_t)d->n_nodes,
               (uint32_t)d->seq_length, k, max_furc, max_deg};
    const uint64_t n_items = 2 * d->seq_length;

    // 1. count, mask the discarded handle-orientations, scan
    uint64_t *counts = B.mem.get<uint64_t>(n_items), *off = B.mem.get<uint64_t>(n_items + 1);
    uint8_t *disc = B.mem.get<uint8_t>(2 * d->n_nodes);
    ix_flags *flags = B.mem.get<ix_flags>(1);
    if (!counts || !off || !disc || !flags) return B.nomem("the work items", n_items);
    VGA_HIP_CHECK(ctx, hipMemsetAsync(disc, 0, 2 * d->n_nodes, st));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(flags, 0, sizeof(ix_flags), st));
    int t_all = vga_timer_begin(ctx, "index_build_total", 0);
    int t = vga_timer_begin(ctx, "k_ix_count", 0);
    hipLaunchKernelGGL(k_ix_count, dim3(ix_grid(n_items, IX_NT)), dim3(IX_NT), 0, st, g, n_items, counts, disc, flags);
    hipLaunchKernelGGL(k_ix_mask, dim3(ix_grid(n_items, 256)), dim3(256), 0, st, g, n_items, counts, (const uint8_t *)disc);
    if (int rc = B.scan(counts, n_items, off)) return rc;
    vga_timer_end(ctx, t);
    ix_flags hf;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(&hf, flags, sizeof hf, hipMemcpyDeviceToHost, st));
    const uint64_t R = B.read_u64(off + n_items);
    VGA_HIP_CHECK(ctx, hipGetLastError());
    if (hf.blown)
        return vga_set_error(ctx, VGA_ERR_NOMEM,
                             "vga_index_build_kmers: the DFS from work item %u takes more than %u steps (the graph's k-mer paths "
                             "blow up; lower max_furcations / max_degree)",
                             hf.blown_item, IX_VISIT_CAP);
    if (R == UINT64_MAX) return vga_set_error(ctx, VGA_ERR_HIP, "vga_index_build_kmers: reading the record count failed");
    if (R >= 0xFFFFFFFFull) return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_index_build_kmers: %llu k-mer records", (unsigned long long)R);
    if (R == 0) return vga_set_error(ctx, VGA_ERR_ARG, "the graph has no k-mer of this length");  // kmer.rs:828 unwrap()

    // 2. emit every record at its emission index
    ix_emit_out o;
    o.off = off;
    o.key = B.mem.get<uint64_t>(R);
    o.val = B.mem.get<uint32_t>(R);
    o.a = B.mem.get<uint32_t>(R);
    o.b = B.mem.get<uint32_t>(R);
    o.forks = B.mem.get<uint8_t>(R);
    if (!o.key || !o.val || !o.a || !o.b || !o.forks) return B.nomem("the k-mer records", R);
    t = vga_timer_begin(ctx, "k_ix_emit", 21 * R);
    hipLaunchKernelGGL(k_ix_emit, dim3(ix_grid(n_items, IX_NT)), dim3(IX_NT), 0, st, g, n_items, disc, flags, o);
    vga_timer_end(ctx, t);

    // 3. stable sort by k-mer, dedup
    uint64_t *skey = o.key;
    uint32_t *sval = o.val;
    t = vga_timer_begin(ctx, "k_ix_sort_kmer", 24 * R * ((2 * k + 7) / 8));
    if (int rc = B.radix(skey, sval, R, 2 * k)) return rc;
    vga_timer_end(ctx, t);
    uint64_t *keep = B.mem.get<uint64_t>(R), *keep_off = B.mem.get<uint64_t>(R + 1);
    if (!keep || !keep_off) return B.nomem("dedup", R);
    t = vga_timer_begin(ctx, "k_ix_dedup", 0);
    hipLaunchKernelGGL(k_ix_dedup, dim3(ix_grid(R, 256)), dim3(256), 0, st, (const uint64_t *)skey, (const uint32_t *)sval, R,
                       (const uint32_t *)o.a, (const uint32_t *)o.b, (const uint8_t *)o.forks, keep);
    if (int rc = B.scan(keep, R, keep_off)) return rc;
    vga_timer_end(ctx, t);
    const uint64_t S = B.read_u64(keep_off + R);
    if (S == UINT64_MAX) return vga_set_error(ctx, VGA_ERR_HIP, "vga_index_build_kmers: reading the survivor count failed");

    // 4. total order (k-mer, start_orient, start, end_orient, end): LSD, positions first, then the k-mer
    uint32_t pb = 1;
    while (pb < 31 && (1ull << pb) <= d->seq_length) pb++;
    uint64_t *pkey = B.mem.get<uint64_t>(S), *fkey = B.mem.get<uint64_t>(S);
    uint32_t *pval = B.mem.get<uint32_t>(S);
    if (!pkey || !fkey || !pval) return B.nomem("the position sort", S);
    t = vga_timer_begin(ctx, "k_ix_sort_pos", 24 * S * ((2 * pb + 2 + 7) / 8 + (2 * k + 7) / 8));
    hipLaunchKernelGGL(k_ix_compact, dim3(ix_grid(R, 256)), dim3(256), 0, st, (const uint32_t *)sval, R, (const uint64_t *)keep_off,
                       (const uint32_t *)o.a, (const uint32_t *)o.b, pb, pkey, pval);
    if (int rc = B.radix(pkey, pval, S, 2 * pb + 2)) return rc;
    hipLaunchKernelGGL(k_ix_gather_key, dim3(ix_grid(S, 256)), dim3(256), 0, st, (const uint32_t *)pval, S, (const uint64_t *)o.key, fkey);
    if (int rc = B.radix(fkey, pval, S, 2 * k)) return rc;
    vga_timer_end(ctx, t);

    // 5. groups, the position table, the probe tables
    uint64_t *head = B.mem.get<uint64_t>(S), *head_off = B.mem.get<uint64_t>(S + 1), *ff = B.mem.get<uint64_t>(S),
             *ff_off = B.mem.get<uint64_t>(S + 1);
    if (!head || !head_off || !ff || !ff_off) return B.nomem("the groups", S);
    t = vga_timer_begin(ctx, "k_ix_groups", 0);
    hipLaunchKernelGGL(k_ix_heads, dim3(ix_grid(S, 256)), dim3(256), 0, st, (const uint64_t *)fkey, (const uint32_t *)pval, S,
                       (const uint32_t *)o.a, (const uint32_t *)o.b, head, ff);
    if (int rc = B.scan(head, S, head_off)) return rc;
    if (int rc = B.scan(ff, S, ff_off)) return rc;
    const uint64_t G = B.read_u64(head_off + S);
    if (G == UINT64_MAX) return vga_set_error(ctx, VGA_ERR_HIP, "vga_index_build_kmers: reading the k-mer count failed");
    const uint64_t NP = S + G;
    uint64_t *table3 = B.mem.get<uint64_t>(3 * NP), *starts = B.mem.get<uint64_t>(G), *ghead = B.mem.get<uint64_t>(G),
             *gend = B.mem.get<uint64_t>(G);
    char *keys = B.mem.get<char>(G * k);
    if (!table3 || !starts || !ghead || !gend || !keys) return B.nomem("the position table", NP);
    hipLaunchKernelGGL(k_ix_groups, dim3(ix_grid(S, 256)), dim3(256), 0, st, (const uint64_t *)fkey, (const uint32_t *)pval, S, k,
                       (const uint32_t *)o.a, (const uint32_t *)o.b, (const uint64_t *)head, (const uint64_t *)head_off, table3, starts,
                       keys, ghead, gend);
    vga_timer_end(ctx, t);

    t = vga_timer_begin(ctx, "k_ix_probe", 0);
    uint64_t *words = B.mem.get<uint64_t>(G), *words_off = B.mem.get<uint64_t>(G + 1);
    if (!words || !words_off) return B.nomem("the probe table", G);
    hipLaunchKernelGGL(k_ix_probe_count, dim3(ix_grid(G, 256)), dim3(256), 0, st, (const uint64_t *)ghead, (const uint64_t *)gend, G,
                       (const uint64_t *)ff_off, words);
    if (int rc = B.scan(words, G, words_off)) return rc;
    uint64_t n_words = B.read_u64(words_off + G);
    if (n_words == UINT64_MAX) return vga_set_error(ctx, VGA_ERR_HIP, "vga_index_build_kmers: reading the probe table size failed");
    if (n_words >= 0xFFFFFFFFull || (k <= 13 && NP >= 0xFFFFFFFFull))
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "position table too large");
    const uint64_t entries = 1ull << (2 * k);
    if (n_words == 0) n_words = 1;  // (as the host loop: one {0, 0} word when no k-mer has a forward/forward record)
    if (hipMalloc((void **)&ix.d_table, entries * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&ix.d_pos, n_words * sizeof(uint2)) != hipSuccess ||
        (k <= 13 && (hipMalloc((void **)&ix.d_table_all, entries * sizeof(uint32_t)) != hipSuccess ||
                     hipMalloc((void **)&ix.d_pos_all, NP * sizeof(uint2)) != hipSuccess))) {
        (void)hipGetLastError();
        return B.nomem("the probe tables", entries);
    }
    ix.table_entries = entries;
    ix.n_pos_words = n_words;
    ix.all_view = ix.d_table_all != nullptr;
    ix.probe_table_bytes = (ix.d_table_all ? 2 : 1) * entries * sizeof(uint32_t);
    ix.probe_pos_bytes = (n_words + (ix.d_pos_all ? NP : 0)) * sizeof(uint2);
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ix.d_table, 0xFF, entries * sizeof(uint32_t), st));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(ix.d_pos, 0, n_words * sizeof(uint2), st));
    if (ix.d_table_all) VGA_HIP_CHECK(ctx, hipMemsetAsync(ix.d_table_all, 0xFF, entries * sizeof(uint32_t), st));
    hipLaunchKernelGGL(k_ix_probe_headers, dim3(ix_grid(G, 256)), dim3(256), 0, st, (const uint64_t *)fkey, (const uint64_t *)ghead,
                       (const uint64_t *)gend, G, (const uint64_t *)ff_off, (const uint64_t *)words_off, ix.d_table, ix.d_pos,
                       ix.d_table_all, ix.d_pos_all);
    hipLaunchKernelGGL(k_ix_probe_records, dim3(ix_grid(S, 256)), dim3(256), 0, st, (const uint32_t *)pval, S, (const uint32_t *)o.a,
                       (const uint32_t *)o.b, (const uint64_t *)head, (const uint64_t *)head_off, (const uint64_t *)ghead,
                       (const uint64_t *)ff, (const uint64_t *)ff_off, (const uint64_t *)words_off, ix.d_pos, ix.d_pos_all);
    vga_timer_end(ctx, t);
    vga_timer_end(ctx, t_all);
    VGA_HIP_CHECK(ctx, hipGetLastError());

    // 6. the k-mer half of *desc, in host memory the caller releases with vga_index_kmers_free
    static_assert(sizeof(vga_kmerpos) == 24, "vga_kmerpos is three u64 words");
    char *h_keys = (char *)malloc(std::max<uint64_t>(G * k, 1));
    uint64_t *h_starts = (uint64_t *)malloc(std::max<uint64_t>(G, 1) * sizeof(uint64_t));
    vga_kmerpos *h_tab = (vga_kmerpos *)malloc(std::max<uint64_t>(NP, 1) * sizeof(vga_kmerpos));
    if (!h_keys || !h_starts || !h_tab) {
        free(h_keys); free(h_starts); free(h_tab);
        return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_index_build_kmers: out of host memory for %llu records", (unsigned long long)NP);
    }
    hipError_t e = hipMemcpyAsync(h_keys, keys, G * k, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_starts, starts, G * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_tab, table3, NP * sizeof(vga_kmerpos), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        free(h_keys); free(h_starts); free(h_tab);
        return vga_set_error(ctx, VGA_ERR_HIP, "vga_index_build_kmers: %s", hipGetErrorString(e));
    }
    vga_timers_collect(ctx);
    d->n_kmers = G;
    d->kmer_keys = h_keys;
    d->kmer_starts = h_starts;
    d->n_kmer_pos = NP;
    d->kmer_pos_table = h_tab;
    ix.loaded = true;
    return VGA_OK;
}

}  // namespace

extern "C" int vga_index_build_kmers(vga_ctx *ctx, vga_index_desc *desc, uint64_t max_furcations, uint64_t max_degree)
{
    if (!ctx) {
        int n = 0;
        return (hipGetDeviceCount(&n) != hipSuccess || n <= 0) ? VGA_ERR_NO_DEVICE : VGA_ERR_ARG;
    }
    if (!desc) return vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: null desc");
    (void)hipSetDevice(ctx->device);
    int rc;
    try {
        rc = ix_build_impl(ctx, desc, max_furcations, max_degree);
    } catch (const std::bad_alloc &) {
        rc = vga_set_error(ctx, VGA_ERR_NOMEM, "vga_index_build_kmers: out of host memory");
    } catch (const std::exception &e) {
        rc = vga_set_error(ctx, VGA_ERR_ARG, "vga_index_build_kmers: %s", e.what());
    }
    if (rc != VGA_OK) {
        (void)hipStreamSynchronize(ctx->stream);
        vga_index_release(ctx->index);  // on failure the context holds no index, as after a failed vga_index_upload
    }
    return rc;
}

extern "C" void vga_index_kmers_free(vga_index_desc *desc)
{
    if (!desc) return;
    free((void *)desc->kmer_keys);
    free((void *)desc->kmer_starts);
    free((void *)desc->kmer_pos_table);
    desc->n_kmers = 0;
    desc->kmer_keys = nullptr;
    desc->kmer_starts = nullptr;
    desc->n_kmer_pos = 0;
    desc->kmer_pos_table = nullptr;
}
