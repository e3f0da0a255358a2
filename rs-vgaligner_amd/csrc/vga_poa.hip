// vga_poa.hip -- banded partial-order alignment on gfx950: the replacement for the reference's only
// native component, abPOA behind  AbpoaAligner::create_align_safe(nodes, edges, query, Global)
// (src/align.rs:173-203; result fields consumed at src/align.rs:1107,1152-1165).
//
//   K4  k_poa_dp_lds<NT,4>  one workgroup per (read, subgraph) problem.  Rows = graph bases in topological
//                        order, processed one after the other because the adaptive band of a row depends on
//                        where its predecessors' maxima fell (that dependency is also why an anti-diagonal
//                        wavefront cannot be used: a row's band is unknown until the rows above are complete).
//                        Lanes run across the band's columns, four adjacent columns per lane.
//   K4b k_poa_traceback  one lane per problem walking the 1-byte direction codes.
//
// HBM layout per problem (all carved from one persistent pool by a device-side bump allocator, 1 MiB chunks;
// every row is stored from the 4-aligned column  bal = beg & ~3  with a width rounded up to 4):
//   direction row  : 1 byte per cell (+3 predecessor-choice bytes per cell on the rare rows with more than one
//                    predecessor) -- the only per-cell data kept for the traceback;
//   value row      : int32 H + two 1-byte clamped gap deltas per cell, kept only for the LAST base of every graph
//                    node (the only rows a later, non-adjacent row can depend on) and the source row;
//   row arrays     : 40 B per row (beg, end, direction offset, value offset, leftmost/rightmost max column,
//                    predecessor row or predecessor-list slice).
// The deltas: a successor only ever needs max(H - (O+E), Ek - E); storing d = min(H - Ek, O) keeps exactly that
// quantity (H - E - d) and the open/extend decision (d == O) in one byte.
//
// Host -> device description of a problem is per NODE (16 B each) plus the node sequences; rows are generated
// on the device.  Numerics are 32-bit integer and bit-exact against oracle/og_poa.c (see its header for the
// specification: recurrences, tie order, band rule).
//
// This file holds every POA kernel and one typed launcher per kernel group (vga_poa_launch.hpp): k_poa_dp_lds and the traceback in
// vga_poa_kernels.hpp, k_poa_dp_t4 ... _t7 in vga_poa_t4.hpp ... vga_poa_t7.hpp, and in vga_poa_row.hpp the instruction helpers
// they share and the row that k_poa_dp_t6 and k_poa_dp_t7 have in common.  The host side lives apart and
// includes no kernel header: vga_poa_run.hip (poa_run -- plan, pool, launch, collect -- and vga_poa_batch), vga_poa_pool.hip (the
// traceback pool), vga_poa_shape.hpp (environment switches, kernel family, launch shape).
#include "vga_common.hpp"
#include "vga_poa_launch.hpp"

#include <algorithm>
#include <cstddef>
#include <map>
#include <mutex>
#include <type_traits>

#include "vga_poa_kernels.hpp"
#include "vga_poa_t4.hpp"
#include "vga_poa_t5.hpp"
#include "vga_poa_t6.hpp"
#include "vga_poa_t7.hpp"
#include "vga_poa_text.hpp"

// The dynamic LDS a kernel may ask for is an attribute of the function for the whole process (per device), and contexts on other
// host threads launch the same kernels with other sizes: the limit only ever goes up, under a lock, so that no launch meets a
// limit that another thread has just set lower than what it asks for
static hipError_t poa_allow_lds(int device, const void *fn, size_t bytes)
{
    static std::mutex mu;
    static std::map<std::pair<int, const void *>, size_t> cur;
    std::lock_guard<std::mutex> g(mu);
    size_t &c = cur[std::make_pair(device, fn)];
    if (bytes <= c) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) c = bytes;
    return e;
}

// One workgroup per staged problem: copies its node table, predecessor rows, sink rows, bases and query from the device
// store of vga_subgraph.hip (and the batch's reads) to where this sub-batch's poa_prob says they are.
// ids: per staged problem its index in the store and its number of predecessor entries.  The store has two parts
// (problems below / from `split`); a re-run launch may hold problems of both.
__global__ __launch_bounds__(256) void k_sg_gather(const uint32_t *__restrict__ ids, const poa_prob *__restrict__ probs, const sg_off *__restrict__ offs,
                                                   uint32_t split, sg_gather_src s0, sg_gather_src s1, const char *__restrict__ reads,
                                                   uint4 *ntab, uint32_t *preds, uint32_t *sinks, char *seq, char *q)
{
    const uint32_t p = ids[2 * blockIdx.x], n_preds = ids[2 * blockIdx.x + 1];
    const poa_prob pb = probs[blockIdx.x];
    const sg_off of = offs[p];
    const sg_gather_src S = p >= split ? s1 : s0;
    const int tid = threadIdx.x;
    const uint4 *a = S.ntab + of.node0 + (p - S.p0);  // (a part's node tables carry one source entry per problem of the part)
    for (uint32_t i = (uint32_t)tid; i < pb.n_nodes; i += 256) ntab[pb.node0 + i] = a[i];
    for (uint32_t i = (uint32_t)tid; i < n_preds; i += 256) preds[pb.pred0 + i] = S.preds[of.pred0 + i];
    for (uint32_t i = (uint32_t)tid; i < pb.n_sink; i += 256) sinks[pb.sink0 + i] = S.sinks[of.sink0 + i];
    const uint32_t *sw = (const uint32_t *)(S.seq + of.seq0);  // (seq0 is a multiple of 4 on both sides)
    uint32_t *dw = (uint32_t *)(seq + pb.seq0);
    for (uint32_t i = (uint32_t)tid; i < (pb.N + 3) / 4; i += 256) dw[i] = sw[i];
    for (uint32_t i = (uint32_t)tid; i < pb.qlen; i += 256) q[pb.q0 + i] = reads[of.q_src + i];
}

// ======================================================================================== launchers
// k_poa_dp_t5 / t6 / t7 share one signature: one switch yields the function, one launch follows
using poa_dp_fn = void (*)(const poa_prob *, const char *, const uint4 *, const uint32_t *, const uint32_t *, poa_t5_args);
using poa_t4_fn = void (*)(const poa_prob *, const char *, const uint4 *, const uint32_t *, const uint32_t *, poa_dev_params, poa_row *, uint8_t *,
                           unsigned long long *, uint64_t, poa_out *, uint32_t, uint32_t, uint32_t, uint8_t *, uint32_t *, uint32_t, uint64_t,
                           unsigned long long *, uint32_t *);
using poa_lds_fn = void (*)(const poa_prob *, const char *, const uint4 *, const uint32_t *, const uint32_t *, const uint32_t *, poa_dev_params,
                            poa_row *, uint8_t *, unsigned long long *, uint64_t, poa_out *, uint32_t, unsigned long long *);

template <int NT>
static poa_dp_fn t5_fn(bool def) { return def ? k_poa_dp_t5<NT, true> : k_poa_dp_t5<NT, false>; }
template <int NT>
static poa_dp_fn t7_fn(bool def) { return def ? k_poa_dp_t7<NT, true> : k_poa_dp_t7<NT, false>; }
template <int NT>
static poa_t4_fn t4_fn(bool def) { return def ? k_poa_dp_t4<NT, true> : k_poa_dp_t4<NT, false>; }

// the instantiated (kernel, workgroup size, default penalties) combinations; null for any other
static poa_dp_fn poa_dp_fn_of(poa_kernel k, int nt, bool def)
{
    if (k == POA_K_T6) return nt != 64 ? nullptr : (def ? k_poa_dp_t6<8, true> : k_poa_dp_t6<8, false>);
    if (k == POA_K_T7) {
        switch (nt) {
        case 128: return t7_fn<128>(def);
        case 256: return t7_fn<256>(def);
        case 512: return t7_fn<512>(def);
        case 1024: return t7_fn<1024>(def);
        }
        return nullptr;
    }
    switch (nt) {
    case 128: return t5_fn<128>(def);
    case 192: return t5_fn<192>(def);
    case 256: return t5_fn<256>(def);
    case 320: return t5_fn<320>(def);
    case 384: return t5_fn<384>(def);
    case 448: return t5_fn<448>(def);
    case 512: return t5_fn<512>(def);
    case 768: return t5_fn<768>(def);
    case 1024: return t5_fn<1024>(def);
    }
    return nullptr;
}

static poa_t4_fn poa_t4_fn_of(int nt, bool def)
{
    switch (nt) {
    case 128: return t4_fn<128>(def);
    case 192: return t4_fn<192>(def);
    case 256: return t4_fn<256>(def);
    case 320: return t4_fn<320>(def);
    case 384: return t4_fn<384>(def);
    case 448: return t4_fn<448>(def);
    case 512: return t4_fn<512>(def);
    case 768: return t4_fn<768>(def);
    case 1024: return t4_fn<1024>(def);
    }
    return nullptr;
}

hipError_t poa_launch_dp(int device, hipStream_t st, const poa_shape &sh, uint32_t nb, const poa_t5_args &a, const uint32_t *sink)
{
    (void)hipGetLastError();  // a launch failure below must be this launch's, not an older ignored status
    hipError_t e;
    if (sh.kernel == POA_K_LDS) {
        // (128, 256 and anything else as 512: the shape only ever halves from 512)
        const poa_lds_fn fn = sh.nt == 128 ? k_poa_dp_lds<128, 4> : (sh.nt == 256 ? k_poa_dp_lds<256, 4> : k_poa_dp_lds<512, 4>);
        const int nt = sh.nt == 128 || sh.nt == 256 ? sh.nt : 512;
        e = poa_allow_lds(device, (const void *)fn, sh.lds);
        hipLaunchKernelGGL(fn, dim3(nb), dim3(nt), sh.lds, st, a.probs, a.queries, a.node_tab, a.seq32, a.preds, sink, a.P, a.rows, a.pool, a.pool_next,
                           a.pool_size, a.outs, a.lds_cols, (unsigned long long *)nullptr);
    } else if (sh.kernel == POA_K_T4) {
        const poa_t4_fn fn = poa_t4_fn_of(sh.nt, sh.def_pen);
        if (!fn) return hipErrorInvalidValue;
        e = poa_allow_lds(device, (const void *)fn, sh.lds);
        hipLaunchKernelGGL(fn, dim3(nb), dim3(sh.nt), sh.lds, st, a.probs, a.queries, a.node_tab, a.seq32, a.preds, a.P, a.rows, a.pool, a.pool_next,
                           a.pool_size, a.outs, a.lds_cols, a.hg_cols, a.win_mask, a.tb_ops, a.tb_orow, 0u, (uint64_t)0, (unsigned long long *)nullptr,
                           (uint32_t *)nullptr);
    } else {
        const poa_dp_fn fn = poa_dp_fn_of(sh.kernel, sh.nt, sh.def_pen);
        if (!fn) return hipErrorInvalidValue;
        e = poa_allow_lds(device, (const void *)fn, sh.lds);
        hipLaunchKernelGGL(fn, dim3(nb), dim3(sh.nt), sh.lds, st, a.probs, a.queries, a.node_tab, a.seq32, a.preds, a);
    }
    const hipError_t le = hipGetLastError();
    return e != hipSuccess ? e : le;
}

template <int ENC>
static void traceback_wave(hipStream_t st, uint32_t nb, const poa_launch_bufs &b, const uint8_t *pool)
{
    hipLaunchKernelGGL(k_poa_traceback_wave<ENC>, dim3(nb), dim3(64), 0, st, nb, b.probs, b.rows, b.preds, pool, b.outs, b.ops, b.orow, 0);
}

void poa_launch_traceback(hipStream_t st, poa_kernel dp, uint32_t nb, const poa_launch_bufs &b, const uint8_t *pool)
{
    // the direction codes: bytes of k_poa_dp_lds, k_poa_dp_t4's own byte encoding, dwords of k_poa_dp_t5
    if (dp == POA_K_LDS) traceback_wave<0>(st, nb, b, pool);
    else if (dp == POA_K_T4) traceback_wave<1>(st, nb, b, pool);
    else traceback_wave<2>(st, nb, b, pool);
}

hipError_t poa_launch_gather(hipStream_t st, uint32_t nb, const uint32_t *ids, const poa_prob *probs, const sg_off *offs, uint32_t split,
                             const sg_gather_src &s0, const sg_gather_src &s1, const char *reads, uint4 *ntab, uint32_t *preds, uint32_t *sinks,
                             char *seq, char *q)
{
    hipLaunchKernelGGL(k_sg_gather, dim3(nb), dim3(256), 0, st, ids, probs, offs, split, s0, s1, reads, ntab, preds, sinks, seq, q);
    return hipGetLastError();
}

hipError_t poa_launch_text(hipStream_t st, uint32_t nb, const poa_launch_bufs &b, char *arena, uint32_t arena_bytes, unsigned long long *cursor,
                           poa_text_out *touts)
{
    hipLaunchKernelGGL(k_poa_text, dim3(nb), dim3(64), 0, st, nb, b.probs, b.outs, b.ops, b.orow, b.rows, b.ntab, (const char *)b.seq32, b.q, arena,
                       arena_bytes, cursor, touts);
    return hipGetLastError();
}

hipError_t poa_launch_text_to_host(hipStream_t st, const uint4 *src, uint4 *dst, uint64_t n16)
{
    hipLaunchKernelGGL(k_poa_text_to_host, dim3((unsigned)std::min<uint64_t>(256, (n16 + 255) / 256)), dim3(256), 0, st, src, dst, n16);
    return hipGetLastError();
}

void poa_launch_chunks_add(hipStream_t st, const poa_chunk_pool &cp, uint32_t first, uint32_t count)
{
    hipLaunchKernelGGL(k_poa_chunks_add, dim3(1), dim3(64), 0, st, cp, first, count);
}
