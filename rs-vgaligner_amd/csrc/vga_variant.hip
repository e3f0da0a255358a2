// vga_variant.hip -- the diploid call at every graph base from the pileup counters: k_vc_count, k_vc_scan, k_vc_emit and the two
// C entry points vga_variant_call / vga_variant_call_table.  See vga_variant.hpp for the shape.
//
// Meaning (include/vga_hip.h): a base whose own letter is A C G T and whose depth reaches min_depth is tested; among the 15
// unordered pairs of the alleles A C G T D the cheapest is its genotype (an observation the pair holds costs 0 under a homozygous
// pair and 256 under a heterozygous one, any other E; the reference genotype wins every tie), among none / het / hom the cheapest
// is its insertion state, and it is reported when either differs from the graph by at least min_qual.  Everything is an integer,
// so the result does not depend on the device, and the reported bases leave in base order: a count per workgroup, one scan of the
// counts, and an emit pass that places each call at  offset of its workgroup + rank inside it  -- no atomic decides a place.
#include "vga_variant.hpp"

#include "vga_pileup.hpp"

#include <algorithm>

namespace {

// column of a letter: a c g t in either case, anything else N (vga_pileup.hip's pu_col)
__device__ __forceinline__ uint32_t vc_col(char c)
{
    const char l = (char)(c | 0x20);
    return l == 'a' ? 0u : l == 'c' ? 1u : l == 'g' ? 2u : l == 't' ? 3u : PU_COL_N;
}

struct vc_params {
    uint32_t E;
    uint64_t min_depth, min_qual;
};

struct vc_site {
    uint64_t row[PU_COLS];
    uint64_t ins_qual, depth;
    uint32_t gt;    // VC_GT(x, y) | state << 6
    uint32_t qual;
    bool tested, reported, big;
};

// One base: 15 + 3 costs in registers.  The loops are unrolled, so n[] is never indexed by a value only known at run time, and the
// order of the definition -- (r, r), the pairs that hold r by their other allele, the rest by (x, y) -- is a key compared on ties.
template <typename T>
__device__ __forceinline__ vc_site vc_eval(const T *__restrict__ counts, const char *__restrict__ letters, uint32_t i, const vc_params &P)
{
    vc_site s;
    s.big = false;
#pragma unroll
    for (uint32_t c = 0; c < PU_COLS; c++) {
        s.row[c] = (uint64_t)counts[(size_t)i * PU_COLS + c];
        s.big = s.big || s.row[c] >= VC_MAX_COUNT;
    }
    const uint64_t n[5] = {s.row[0], s.row[1], s.row[2], s.row[3], s.row[PU_COL_DEL]};
    const uint64_t ins = s.row[PU_COL_INS];
    const uint32_t r = vc_col(letters[i]);
    const uint64_t S = n[0] + n[1] + n[2] + n[3] + n[4], E = P.E;
    s.depth = S + s.row[PU_COL_N];
    s.tested = !s.big && r < 4u && s.depth >= P.min_depth;
    uint64_t best = ~0ull, second = ~0ull;
    uint32_t bkey = 0xFFFFFFFFu, bgt = 0;
#pragma unroll
    for (uint32_t x = 0; x < 5; x++) {
#pragma unroll
        for (uint32_t y = x; y < 5; y++) {
            const uint64_t cost = x == y ? E * (S - n[x]) : 256ull * (n[x] + n[y]) + E * (S - n[x] - n[y]);
            const uint32_t key = (x == r && y == r) ? 0u : x == r ? 1u + y - (y > r ? 1u : 0u) : y == r ? 1u + x - (x > r ? 1u : 0u) : 5u + x * 5u + y;
            if (cost < best || (cost == best && key < bkey)) {
                second = best;  // (best <= second: the pair that loses its place is the cheapest of the others)
                best = cost;
                bkey = key;
                bgt = VC_GT(x, y);
            } else if (cost < second)
                second = cost;
        }
    }
    const uint64_t q = second - best;
    s.qual = q > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)q;
    // the insertion behind the base: none, het, hom -- the first minimum in that order
    const uint64_t k = ins < s.depth ? ins : s.depth;
    const uint64_t c0 = ins * E, c1 = 256ull * s.depth, c2 = (s.depth - k) * E;
    uint32_t state = 0;
    uint64_t ib = c0;
    if (c1 < ib) { ib = c1; state = 1u; }
    if (c2 < ib) { ib = c2; state = 2u; }
    const uint64_t lo01 = c0 < c1 ? c0 : c1, hi01 = c0 < c1 ? c1 : c0, mid = lo01 > (hi01 < c2 ? hi01 : c2) ? lo01 : (hi01 < c2 ? hi01 : c2);
    s.ins_qual = mid - ib;
    s.gt = bgt | (state << 6);
    s.reported = s.tested && ((bgt != VC_GT(r, r) && (uint64_t)s.qual >= P.min_qual) || (state != 0u && s.ins_qual >= P.min_qual));
    return s;
}

// One base per thread.  wg_calls[b] / wg_tested[b]: the reported / tested bases of workgroup b (a ballot and a popcount per wave,
// the four waves added through LDS).  flags bit 0: some counter has VC_MAX_COUNT or more (an OR: no order in it).
template <typename T>
__global__ __launch_bounds__(VC_BLOCK) void k_vc_count(const T *__restrict__ counts, const char *__restrict__ letters, uint32_t n, vc_params P,
                                                       uint32_t *__restrict__ wg_calls, uint32_t *__restrict__ wg_tested, uint32_t *__restrict__ flags)
{
    __shared__ uint32_t s_calls[VC_BLOCK / 64], s_tested[VC_BLOCK / 64];
    const uint32_t tid = threadIdx.x, i = blockIdx.x * VC_BLOCK + tid;
    bool rep = false, tst = false, big = false;
    if (i < n) {
        const vc_site s = vc_eval<T>(counts, letters, i, P);
        rep = s.reported; tst = s.tested; big = s.big;
    }
    const uint64_t rmask = __builtin_amdgcn_ballot_w64(rep), tmask = __builtin_amdgcn_ballot_w64(tst), bmask = __builtin_amdgcn_ballot_w64(big);
    if ((tid & 63u) == 0u) {
        s_calls[tid >> 6] = (uint32_t)__builtin_popcountll(rmask);
        s_tested[tid >> 6] = (uint32_t)__builtin_popcountll(tmask);
        if (bmask) atomicOr(flags, 1u);
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t c = 0, t = 0;
        for (uint32_t w = 0; w < VC_BLOCK / 64; w++) { c += s_calls[w]; t += s_tested[w]; }
        wg_calls[blockIdx.x] = c;
        wg_tested[blockIdx.x] = t;
    }
}

// wg_off[b] = wg_calls[0] + ... + wg_calls[b - 1] for b = 0 .. n_wg, totals = {tested, calls}: one workgroup, a contiguous piece per
// thread, the pieces' sums scanned in LDS (k_pu_finish's shape).
__global__ __launch_bounds__(VC_SCAN_BLOCK) void k_vc_scan(const uint32_t *__restrict__ wg_calls, const uint32_t *__restrict__ wg_tested, uint32_t n_wg,
                                                           uint32_t *__restrict__ wg_off, unsigned long long *__restrict__ totals)
{
    __shared__ uint32_t part[VC_SCAN_BLOCK], tpart[VC_SCAN_BLOCK];
    const uint32_t tid = threadIdx.x;
    const uint32_t piece = (n_wg + VC_SCAN_BLOCK - 1u) / VC_SCAN_BLOCK;
    const uint64_t a64 = (uint64_t)tid * piece, b64 = a64 + piece;
    const uint32_t a = a64 < n_wg ? (uint32_t)a64 : n_wg, b = b64 < n_wg ? (uint32_t)b64 : n_wg;
    uint32_t s = 0, t = 0;
    for (uint32_t i = a; i < b; i++) { s += wg_calls[i]; t += wg_tested[i]; }
    part[tid] = s;
    tpart[tid] = t;
    __syncthreads();
    for (uint32_t d = 1; d < VC_SCAN_BLOCK; d <<= 1) {
        const uint32_t u = tid >= d ? part[tid - d] : 0u, v = tid >= d ? tpart[tid - d] : 0u;
        __syncthreads();
        part[tid] += u;
        tpart[tid] += v;
        __syncthreads();
    }
    uint32_t run = tid ? part[tid - 1] : 0u;
    for (uint32_t i = a; i < b; i++) {
        wg_off[i] = run;
        run += wg_calls[i];
    }
    if (tid == VC_SCAN_BLOCK - 1u) {
        wg_off[n_wg] = part[tid];
        totals[0] = tpart[tid];
        totals[1] = part[tid];
    }
}

// The workgroups that reported something evaluate their bases once more and write each call at  wg_off[b] + its rank among the
// reported lanes of the workgroup  (mbcnt over the wave's ballot, the waves below through LDS), as long as that place is below cap.
template <typename T>
__global__ __launch_bounds__(VC_BLOCK) void k_vc_emit(const T *__restrict__ counts, const char *__restrict__ letters, uint32_t n, vc_params P,
                                                      const uint32_t *__restrict__ wg_off, uint32_t cap, uint32_t *__restrict__ pos,
                                                      uint8_t *__restrict__ gt, uint32_t *__restrict__ qual, unsigned long long *__restrict__ ins_qual,
                                                      unsigned long long *__restrict__ depth, unsigned long long *__restrict__ rows)
{
    __shared__ uint32_t s_calls[VC_BLOCK / 64];
    const uint32_t off = wg_off[blockIdx.x];
    if (wg_off[blockIdx.x + 1] == off || off >= cap) return;  // (the same for every thread of the workgroup)
    const uint32_t tid = threadIdx.x, i = blockIdx.x * VC_BLOCK + tid;
    vc_site s;
    s.reported = false;
    if (i < n) s = vc_eval<T>(counts, letters, i, P);
    const uint64_t rmask = __builtin_amdgcn_ballot_w64(s.reported);
    if ((tid & 63u) == 0u) s_calls[tid >> 6] = (uint32_t)__builtin_popcountll(rmask);
    __syncthreads();
    if (!s.reported) return;
    uint32_t at = off + __builtin_amdgcn_mbcnt_hi((uint32_t)(rmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)rmask, 0u));
    for (uint32_t w = 0; w < (tid >> 6); w++) at += s_calls[w];
    if (at >= cap) return;
    pos[at] = i;
    gt[at] = (uint8_t)s.gt;
    qual[at] = s.qual;
    ins_qual[at] = s.ins_qual;
    depth[at] = s.depth;
#pragma unroll
    for (uint32_t c = 0; c < PU_COLS; c++) rows[(size_t)at * PU_COLS + c] = s.row[c];
}

struct vc_out {
    uint64_t cap;
    uint32_t *pos;
    uint8_t *gt;
    uint32_t *qual;
    uint64_t *ins_qual, *depth, *rows, *n_tested, *n_calls;
};

// the three kernels over a table that is on the device, and the first min(n_calls, cap) calls back to the host
template <typename T>
int vc_run(vga_ctx *ctx, const char *who, const T *d_counts, const char *d_letters, uint32_t n, const vc_params &P, const vc_out &o)
{
    hipStream_t st = ctx->stream;
    unsigned long long totals[2] = {0ull, 0ull};
    vga_timers_reset(ctx);
    if (n) {
        const uint32_t n_wg = (n + VC_BLOCK - 1u) / VC_BLOCK;
        vga_dbuf<uint32_t> d_wg;  // wg_calls, wg_tested (n_wg each), wg_off (n_wg + 1), flags (1)
        vga_dbuf<unsigned long long> d_totals;
        VGA_HIP_CHECK_OOM(ctx, d_wg.reserve((size_t)3 * n_wg + 2));
        VGA_HIP_CHECK_OOM(ctx, d_totals.reserve(2));
        uint32_t *wg_calls = d_wg.p, *wg_tested = d_wg.p + n_wg, *wg_off = d_wg.p + 2 * (size_t)n_wg, *flags = d_wg.p + 3 * (size_t)n_wg + 1;
        VGA_HIP_CHECK(ctx, hipMemsetAsync(flags, 0, 4, st));
        int rc = vga_launch(ctx, "k_vc_count", (uint64_t)n * (PU_COLS * sizeof(T) + 1), k_vc_count<T>, dim3(n_wg), dim3(VC_BLOCK), d_counts, d_letters, n, P, wg_calls, wg_tested, flags);
        if (rc == VGA_OK) rc = vga_launch(ctx, "k_vc_scan", (uint64_t)n_wg * 12, k_vc_scan, dim3(1), dim3(VC_SCAN_BLOCK), wg_calls, wg_tested, n_wg, wg_off, d_totals.p);
        if (rc != VGA_OK) return rc;
        uint32_t h_flags = 0;
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(totals, d_totals.p, sizeof totals, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(&h_flags, flags, 4, hipMemcpyDeviceToHost, st));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        if (h_flags & 1u) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, OPLIST_ERR_WIDE, who);
        const uint64_t m = std::min<uint64_t>(totals[1], o.cap);
        if (m) {
            vga_dbuf<uint32_t> d_pos, d_qual;
            vga_dbuf<uint8_t> d_gt;
            vga_dbuf<unsigned long long> d_wide;  // ins_qual, depth (m each), rows (7 m)
            VGA_HIP_CHECK_OOM(ctx, d_pos.reserve(m));
            VGA_HIP_CHECK_OOM(ctx, d_qual.reserve(m));
            VGA_HIP_CHECK_OOM(ctx, d_gt.reserve(m));
            VGA_HIP_CHECK_OOM(ctx, d_wide.reserve((size_t)m * (2 + PU_COLS)));
            unsigned long long *d_insq = d_wide.p, *d_depth = d_wide.p + m, *d_rows = d_wide.p + 2 * m;
            rc = vga_launch(ctx, "k_vc_emit", m * (13 + 8 * (2 + PU_COLS)), k_vc_emit<T>, dim3(n_wg), dim3(VC_BLOCK), d_counts, d_letters, n, P, wg_off, (uint32_t)m, d_pos.p, d_gt.p,
                            d_qual.p, d_insq, d_depth, d_rows);
            if (rc != VGA_OK) return rc;
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.pos, d_pos.p, m * 4, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.gt, d_gt.p, m, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.qual, d_qual.p, m * 4, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.ins_qual, d_insq, m * 8, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.depth, d_depth, m * 8, hipMemcpyDeviceToHost, st));
            if (o.rows) VGA_HIP_CHECK(ctx, hipMemcpyAsync(o.rows, d_rows, m * PU_COLS * 8, hipMemcpyDeviceToHost, st));
            VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        }
        vga_timers_collect(ctx);
    }
    if (o.n_tested) *o.n_tested = totals[0];
    if (o.n_calls) *o.n_calls = totals[1];
    return VGA_OK;
}

int vc_check(vga_ctx *ctx, const char *who, uint32_t E, uint64_t min_depth, const vc_out &o)
{
    if (E < VC_MIN_ERROR || E > VC_MAX_ERROR) return vga_set_error(ctx, VGA_ERR_ARG, "%s: error cost %u, %u to %u are served", who, E, VC_MIN_ERROR, VC_MAX_ERROR);
    if (min_depth < 1) return vga_set_error(ctx, VGA_ERR_ARG, "%s: min_depth is at least 1", who);
    if (o.cap && (!o.pos || !o.gt || !o.qual || !o.ins_qual || !o.depth)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with cap %llu", who, (unsigned long long)o.cap);
    return VGA_OK;
}

}  // namespace

extern "C" int vga_variant_call(vga_ctx *ctx, uint32_t E, uint64_t min_depth, uint64_t min_qual, uint64_t cap, uint32_t *pos, uint8_t *gt, uint32_t *qual,
                                uint64_t *ins_qual, uint64_t *depth, uint64_t *counts, uint64_t *n_tested, uint64_t *n_calls)
{
    if (!ctx) return VGA_ERR_ARG;
    const vc_out o = {cap, pos, gt, qual, ins_qual, depth, counts, n_tested, n_calls};
    int rc = vc_check(ctx, __func__, E, min_depth, o);
    if (rc != VGA_OK) return rc;
    if (!oplist_on(ctx, pu_maker(), __func__)) return VGA_ERR_ARG;
    pu_state *pu = pu_active(ctx);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    const uint32_t *table = nullptr;
    uint32_t n = 0;
    if ((rc = pu_finish_device(ctx, pu, __func__, &table, &n)) != VGA_OK) return rc;
    const vc_params P = {E, min_depth, min_qual};
    return vc_run<uint32_t>(ctx, __func__, table, ctx->index.d_seq_fwd, n, P, o);
}

extern "C" int vga_variant_call_table(vga_ctx *ctx, uint64_t n, const uint64_t *counts_in, const char *letters, uint32_t E, uint64_t min_depth, uint64_t min_qual,
                                      uint64_t cap, uint32_t *pos, uint8_t *gt, uint32_t *qual, uint64_t *ins_qual, uint64_t *depth, uint64_t *counts,
                                      uint64_t *n_tested, uint64_t *n_calls)
{
    if (!ctx) return VGA_ERR_ARG;
    const vc_out o = {cap, pos, gt, qual, ins_qual, depth, counts, n_tested, n_calls};
    int rc = vc_check(ctx, __func__, E, min_depth, o);
    if (rc != VGA_OK) return rc;
    if (n && (!counts_in || !letters)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null table", __func__);
    if (n >= VC_MAX_BASES) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu bases, positions are 31-bit", __func__, (unsigned long long)n);
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vga_dbuf<unsigned long long> d_counts;
    vga_dbuf<char> d_letters;
    if ((rc = table_upload(ctx, d_counts, counts_in, (size_t)n * PU_COLS)) != VGA_OK) return rc;
    if ((rc = table_upload(ctx, d_letters, letters, (size_t)n)) != VGA_OK) return rc;
    const vc_params P = {E, min_depth, min_qual};
    return vc_run<unsigned long long>(ctx, __func__, d_counts.p, d_letters.p, (uint32_t)n, P, o);
}
