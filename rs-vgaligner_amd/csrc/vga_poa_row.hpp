// vga_poa_row.hpp -- the row of k_poa_dp_t6 and k_poa_dp_t7, once: what the two kernels have in common of a problem's set-up, a
// row's topology, band, allocation and record, the staging of a virtual predecessor row, the cell recurrences and the epilogue.
// Everything here is a __device__ __forceinline__ function or a plain struct of scalars; what differs between one wave and a
// workgroup (broadcasts, waits and barriers, where the row above lives, the row maximum, the sink pick-up) stays in the kernels.
// The first part holds the instruction helpers that k_poa_dp_t4 and k_poa_dp_t5 share with them, under their old names.
#pragma once

#include "vga_poa_launch.hpp"
#include "vga_poa_kernels.hpp"

#define T4_NEG (4 * POA_NEG)

template <int B>
__device__ __forceinline__ int t4_sub_byte(int a, int g)  // a - byte B of g
{
    int r;
    if constexpr (B == 0) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "=v"(r) : "v"(a), "v"(g));
    if constexpr (B == 1) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "=v"(r) : "v"(a), "v"(g));
    if constexpr (B == 2) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "=v"(r) : "v"(a), "v"(g));
    if constexpr (B == 3) asm("v_sub_u32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "=v"(r) : "v"(a), "v"(g));
    return r;
}
// byte B of dst = min(t, c) (unsigned; c <= 255), and  acc = 2 acc + (t >= c)
template <int B>
__device__ __forceinline__ void t4_gap_byte(int &dst, int &acc, int t, int c)
{
    if constexpr (B == 0) asm("v_min_u32_sdwa %0, %2, %3 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\tv_cmp_le_u32 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc" : "+v"(dst), "+v"(acc) : "v"(t), "s"(c) : "vcc");
    if constexpr (B == 1) asm("v_min_u32_sdwa %0, %2, %3 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\tv_cmp_le_u32 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc" : "+v"(dst), "+v"(acc) : "v"(t), "s"(c) : "vcc");
    if constexpr (B == 2) asm("v_min_u32_sdwa %0, %2, %3 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\tv_cmp_le_u32 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc" : "+v"(dst), "+v"(acc) : "v"(t), "s"(c) : "vcc");
    if constexpr (B == 3) asm("v_min_u32_sdwa %0, %2, %3 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD\n\tv_cmp_le_u32 vcc, %3, %2\n\tv_addc_co_u32 %1, vcc, %1, %1, vcc" : "+v"(dst), "+v"(acc) : "v"(t), "s"(c) : "vcc");
}
__device__ __forceinline__ void t4_flag_ne(int &acc, int a, int b)  // acc = 2 acc + (a != b)
{
    asm("v_cmp_ne_u32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, %0, %0, vcc" : "+v"(acc) : "v"(a), "v"(b) : "vcc");
}
// byte B of dst = low byte of (2 acc + (a != b))
template <int B>
__device__ __forceinline__ void t4_flag_ne_dep(int &dst, int acc, int a, int b)
{
    if constexpr (B == 0) asm("v_cmp_ne_u32 vcc, %2, %3\n\tv_addc_co_u32_sdwa %0, vcc, %1, %1, vcc dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(acc), "v"(a), "v"(b) : "vcc");
    if constexpr (B == 1) asm("v_cmp_ne_u32 vcc, %2, %3\n\tv_addc_co_u32_sdwa %0, vcc, %1, %1, vcc dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(acc), "v"(a), "v"(b) : "vcc");
    if constexpr (B == 2) asm("v_cmp_ne_u32 vcc, %2, %3\n\tv_addc_co_u32_sdwa %0, vcc, %1, %1, vcc dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(acc), "v"(a), "v"(b) : "vcc");
    if constexpr (B == 3) asm("v_cmp_ne_u32 vcc, %2, %3\n\tv_addc_co_u32_sdwa %0, vcc, %1, %1, vcc dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(acc), "v"(a), "v"(b) : "vcc");
}
__device__ __forceinline__ int t4_max3(int a, int b, int c)
{
    int r;
    asm("v_max3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// lanes 1..63: max(v of the lane below, pre); lane 0: pre   (wave_shr:1, bound_ctrl off: lane 0 keeps the old value)
__device__ __forceinline__ int t4_shr1_max(int v, int pre)
{
    int r = pre;
    asm("s_nop 1\n\tv_max_i32_dpp %0, %1, %2 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(v), "v"(pre));  // (s_nop: the compiler does not see that %1 is read through DPP)
    return r;
}
__device__ __forceinline__ int t4_shr1_mov(int v, int first)  // lanes 1..63: v of the lane below; lane 0: first
{
    int r = first;
    asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(v));
    return r;
}

// byte B of dst = min(t, c)   (unsigned; c <= 255)
template <int B>
__device__ __forceinline__ void t5_min_byte(int &dst, int t, int c)
{
    if constexpr (B == 0) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:BYTE_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(t), "s"(c));
    if constexpr (B == 1) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(t), "s"(c));
    if constexpr (B == 2) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:BYTE_2 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(t), "s"(c));
    if constexpr (B == 3) asm("v_min_u32_sdwa %0, %1, %2 dst_sel:BYTE_3 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:DWORD" : "+v"(dst) : "v"(t), "s"(c));
}

// a scalar of its own: cuts a uniform value loose from the (wide) load that produced it
__device__ __forceinline__ int t5_own(int v)
{
    asm volatile("" : "+v"(v));  // (through a vector register: the prologue can afford it, and nothing can be folded away)
    return __builtin_amdgcn_readfirstlane(v);
}
__device__ __forceinline__ uint32_t t5_own(uint32_t v) { return (uint32_t)t5_own((int)v); }
__device__ __forceinline__ uint64_t t5_own(uint64_t v) { return ((uint64_t)t5_own((uint32_t)(v >> 32)) << 32) | t5_own((uint32_t)v); }
template <typename T>
__device__ __forceinline__ T *t5_own(T *p) { return (T *)t5_own((uint64_t)p); }

// ================================================================================================================================
// The shared row of k_poa_dp_t6 / k_poa_dp_t7.  Recurrences, direction dwords, value rows, row records, chunk pool and fused
// traceback are k_poa_dp_t5's (bit-exact against oracle/og_poa.c).

// ---- the problem, in scalars of the wave's own
struct poa_row_view {
    int qlen;
    const char *query;
    const uint4 *ntab;
    const uint32_t *plist, *seqw;
    poa_row *R;
    uint32_t n_nodes, ring_rows;
    int bw, banded, p_match, p_mismatch;
};
__device__ __forceinline__ poa_row_view poa_row_view_of(const poa_prob &pb, const char *queries, const uint4 *node_tab, const uint32_t *seq32,
                                                        const uint32_t *preds, const poa_t5_args &A)
{
    poa_row_view V;
    V.qlen = t5_own((int)pb.qlen);
    V.query = queries + pb.q0;
    V.ntab = node_tab + t5_own(pb.node0);
    V.plist = preds + t5_own(pb.pred0);
    V.seqw = seq32 + t5_own(pb.seq0 >> 2);
    V.R = A.rows + t5_own(pb.row0);
    V.n_nodes = t5_own(pb.n_nodes);
    V.ring_rows = t5_own(pb.ring_rows);
    V.bw = t5_own((int)pb.w);
    V.banded = t5_own(A.P.banded);
    V.p_match = t5_own(A.P.match);
    V.p_mismatch = t5_own(A.P.mismatch);
    return V;
}
// gap penalties (compile-time constants under DEF) and what the gap-byte arithmetic of k_poa_dp_t5 derives from them
struct poa_row_pen {
    int o1, e1, o2, e2, D1, D2;
    uint32_t g_bias, e_probe;
};
template <bool DEF>
__device__ __forceinline__ poa_row_pen poa_row_pen_of(const poa_dev_params &P)
{
    poa_row_pen K;
    K.o1 = DEF ? 4 : t5_own(P.o1); K.e1 = DEF ? 2 : t5_own(P.e1); K.o2 = DEF ? 24 : t5_own(P.o2); K.e2 = DEF ? 1 : t5_own(P.e2);
    K.D1 = 4 * K.o1; K.D2 = 4 * K.o2 + 1;
    K.g_bias = (uint32_t)(4 * K.e1 | (4 * K.e2) << 8) * 0x00010001u;
    K.e_probe = (uint32_t)((128 - K.D1) | (128 - K.D2) << 8) * 0x00010001u;
    return K;
}

// ---- the state region (ring of value rows) of slot `got`; no slot: the problem's first thread writes the result (the pool is
// full, or the launch is not in chunk-pool mode and the problem goes back) and the kernel returns
__device__ __forceinline__ bool poa_row_state(const poa_t5_args &A, int got, bool first_thread, uint64_t &state_lo)
{
    if (got < 0) {
        if (first_thread) {
            poa_out &O = A.outs[blockIdx.x];
            O.t_end = O.t_begin; O.cells = 0; O.vcells = 0; O.maxw = 0; O.nops = 0;
            O.score = POA_NEG; O.row = 0; O.status = A.cp.n_slots ? POA_ST_POOL : POA_ST_RETRY;
        }
        return false;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    state_lo = (uint64_t)A.cp.state_base + (uint64_t)(uint32_t)got * A.cp.state_size;
    return true;
}

// ---- direction rows (and the value rows that outlive the ring) out of 1 MiB chunks: the problem's list of chunks and the cursor
// in the newest one.  One thread pops (poa_chunks_pop), everybody hears of it the kernel's way and books it (poa_chunks_took)
struct poa_chunks {
    uint32_t own_head, own_tail, own_chunks;
    uint64_t dcur;
    uint32_t drem;
};
__device__ __forceinline__ uint32_t poa_chunks_pop(const poa_chunk_pool &cp, const poa_chunks &C)
{
    const uint32_t idx = poa_chunk_pop(cp, blockIdx.x);
    if (idx != POA_NIL) __hip_atomic_store(cp.next + idx, C.own_head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return idx;
}
__device__ __forceinline__ void poa_chunks_took(poa_chunks &C, uint32_t idx, uint64_t addr)
{
    C.own_head = idx;
    if (C.own_tail == POA_NIL) C.own_tail = idx;
    C.own_chunks++;
    C.dcur = addr;
    C.drem = (uint32_t)POA_CHUNK;
}
__device__ __forceinline__ uint64_t poa_chunks_bump(poa_chunks &C, uint32_t bytes)
{
    const uint64_t r = C.dcur;
    C.dcur += bytes;
    C.drem -= bytes;
    return r;
}

// ---- column codes (one-hot nibbles, four columns per halfword): column j stands for query[j - 1].  Returns whether the thread
// met a character other than A / C / G / T
__device__ __forceinline__ int poa_row_codes(uint16_t *Qn, const char *query, int qlen, int n_hw, int tid, int nt)
{
    int non_acgt = 0;
    for (int t = tid; t < n_hw; t += nt) {
        uint32_t hw = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int j = 4 * t + k;
            uint32_t code = 0;
            if (j >= 1 && j <= qlen) {
                const char ch = query[j - 1];
                code = (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') ? 1u << (((uint32_t)ch >> 1) & 3u) : 0u;
                non_acgt |= code == 0;
            }
            hw |= code << (4 * k);
        }
        Qn[t] = (uint16_t)hw;
    }
    return non_acgt;
}

// ---- row `tn` of node `v` (table entry nt): where it sits in the graph
struct poa_row_topo {
    uint32_t r;      // the row
    bool last;       // last base of its node (its value row is kept)
    bool is_sink;
    uint32_t ps;     // predecessor row, or first entry of the predecessor list
    uint32_t gb;     // the row's base
    bool simple;     // the only predecessor is the row above
    bool first;      // first base of a node
    int np;          // predecessors
    int remain;      // graph bases after this row on the longest path to the sink
};
__device__ __forceinline__ poa_row_topo poa_row_topo_of(const uint4 nt, uint32_t v, uint32_t tn, const uint32_t *seqw, uint32_t &seq_word,
                                                        uint32_t &seq_word_idx)
{
    const uint32_t nlen = nt.y & 0xFFFFFFu;
    const int np_node = (int)(nt.y >> 24);
    poa_row_topo T;
    T.r = nt.x + tn;
    T.last = tn + 1 == nlen;
    T.is_sink = T.last && (nt.z >> 31) != 0;
    T.ps = nt.w;
    T.gb = 0;
    if (v > 0) {
        const uint32_t bi = T.r - 1;
        if ((bi & 3u) == 0 || (bi >> 2) != seq_word_idx) { seq_word_idx = bi >> 2; seq_word = seqw[seq_word_idx]; }
        T.gb = (seq_word >> (8u * (bi & 3u))) & 0xffu;
    }
    T.simple = T.r > 0 && (tn > 0 || (np_node == 1 && T.ps == T.r - 1));
    T.first = tn == 0 && v > 0;
    T.np = v == 0 ? 0 : (tn == 0 ? np_node : 1);
    T.remain = (int)(nt.z & 0x3fffffffu) + (int)(nlen - 1 - tn);
    return T;
}

// ---- band.  The span of the maxima of a row's predecessors when they are not just the row above: a far predecessor's columns
// come out of its row record (the caller has waited for it to land)
__device__ __forceinline__ void poa_row_far_span(const poa_row_view &V, const poa_row_topo &T, int prev_lmax, int prev_rmax, int &mpl, int &mpr)
{
    mpl = INT32_MAX; mpr = 0;
    for (int t = 0; t < T.np; t++) {
        const uint32_t p = T.np == 1 ? T.ps : V.plist[T.ps + t];
        int lm, rm;
        if (p == T.r - 1) { lm = prev_lmax + 1; rm = prev_rmax + 1; }
        else {
            lm = __builtin_amdgcn_readfirstlane(V.R[p].lmax) + 1;
            rm = __builtin_amdgcn_readfirstlane(V.R[p].rmax) + 1;
        }
        mpl = lm < mpl ? lm : mpl;
        mpr = rm > mpr ? rm : mpr;
    }
}
// the band of a row whose predecessors' maxima span [mpl, mpr]: widened to the diagonal and by the band width; bal / W: the first
// column and the width of the row's storage
__device__ __forceinline__ void poa_row_band(const poa_row_view &V, const poa_row_topo &T, int mpl, int mpr, int &beg, int &end, int &bal, int &W)
{
    if (!V.banded) { beg = 0; end = V.qlen; }
    else {
        const int diag = V.qlen - T.remain;
        const int lo = mpl < diag ? mpl : diag;
        const int hi = mpr > diag ? mpr : diag;
        beg = lo - V.bw; if (beg < 0) beg = 0;
        end = hi + V.bw; if (end > V.qlen) end = V.qlen;
    }
    bal = beg & ~3;
    W = (end - bal + 1 + 3) & ~3;
}

// ---- row allocation and record
__device__ __forceinline__ uint32_t poa_row_dir_bytes(int W, int np) { return (uint32_t)W * (np > 1 ? 4u : 1u); }
// a kept value row lives in a chunk if it outlives the ring (and the source row's does): else in the next ring slot
__device__ __forceinline__ bool poa_row_value_in_chunk(const poa_row_topo &T, const uint4 nt) { return T.r == 0 || (nt.z & 0x40000000u); }
__device__ __forceinline__ uint64_t poa_row_ring_slot(uint64_t ring_base, uint32_t ring_size, uint32_t ring_rows, uint32_t &ring_head)
{
    const uint64_t voff = ring_base + (uint64_t)ring_head * ring_size;
    ring_head = ring_head + 1 == ring_rows ? 0 : ring_head + 1;
    return voff;
}
struct poa_row_counts {
    uint64_t cells, vcells;
    int maxw;
};
__device__ __forceinline__ void poa_row_record(poa_row *R, const poa_row_topo &T, bool first_thread, int beg, int end, int W, uint64_t doff,
                                               uint64_t voff, poa_row_counts &N)
{
    if (T.r > 0) N.cells += (uint64_t)(end - beg + 1);
    if (T.last) N.vcells += (uint64_t)(end - beg + 1);
    N.maxw = W > N.maxw ? W : N.maxw;
    if (first_thread) {
        // what the traceback reads of every row: band, direction row, predecessor (a row inside a node: npred 0 = the row above)
        *(int4 *)&R[T.r].beg = make_int4(beg, end, (int)(uint32_t)doff, (int)(uint32_t)(doff >> 32));
        *(uint2 *)&R[T.r].pred = make_uint2(T.ps, T.first ? (uint32_t)T.np : 0u);
        if (T.last) R[T.r].voff = voff;
    }
}

// ---- the row's base: which column-code bit matches it, and the substitution scores as tagged words
struct poa_row_base {
    int gsh, ne4t, mm4;
};
__device__ __forceinline__ poa_row_base poa_row_base_of(uint32_t gb, int p_match, int p_mismatch)
{
    const uint32_t gd = gb - (uint32_t)'A';
    const bool acgt = gd < 20u && ((0x80045u >> gd) & 1u);
    const int sc_eq = acgt ? p_match : 0, sc_ne = acgt ? -p_mismatch : 0;
    poa_row_base B;
    B.gsh = (int)((gb >> 1) & 3u);
    B.ne4t = 4 * sc_ne + 1;
    B.mm4 = 4 * (sc_eq - sc_ne);
    return B;
}

// ---- STAGING (k_poa_dp_t5's): the virtual predecessor row of the predecessors' value rows
// a predecessor's value row and band  (no value row -- vga_poa_t5.hpp, staging: Vq null, Wq 0, the problem is given up)
struct poa_pred_row {
    const uint8_t *Vq;
    int bp, balq, Wq;
    unsigned pspan;
};
__device__ __forceinline__ poa_pred_row poa_pred_row_of(const poa_row *R, uint32_t p)
{
    poa_pred_row P;
    P.bp = __builtin_amdgcn_readfirstlane(R[p].beg);
    const int ep = __builtin_amdgcn_readfirstlane(R[p].end);
    const uint64_t vq_off = poa_uniform_u64(R[p].voff);
    P.Vq = (const uint8_t *)vq_off;
    P.balq = P.bp & ~3;
    P.Wq = vq_off != 0 ? (ep - P.balq + 1 + 3) & ~3 : 0;
    P.pspan = (unsigned)(ep - P.bp);
    return P;
}
// the quad at column j0 as the value row holds it (`fill` where the row has no storage)
__device__ __forceinline__ void poa_pred_quad(const poa_pred_row &P, int j0, int fill, int4 &hv, uint2 &gg)
{
    const int idx = j0 - P.balq;
    hv = make_int4(fill, fill, fill, fill);
    gg = make_uint2(0u, 0u);
    if (idx >= 0 && idx < P.Wq) {
        hv = *(const int4 *)((const int32_t *)P.Vq + idx);
        gg = *(const uint2 *)(P.Vq + 4ll * P.Wq + 2ll * idx);
    }
}
__device__ __forceinline__ int poa_pred_word(const poa_pred_row &P, int j, int fill)
{
    const int idx = j - P.balq;
    return (idx >= 0 && idx < P.Wq) ? ((const int32_t *)P.Vq)[idx] : fill;
}
// one predecessor: its quad at j0, masked by its band
__device__ __forceinline__ void poa_stage_quad(const poa_pred_row &P, int j0, int4 &hv, uint2 &gg)
{
    poa_pred_quad(P, j0, T4_NEG + 1, hv, gg);
    const unsigned pspan = P.pspan;
    const bool in0 = (unsigned)(j0 - P.bp) <= pspan, in1 = (unsigned)(j0 + 1 - P.bp) <= pspan, in2 = (unsigned)(j0 + 2 - P.bp) <= pspan,
               in3 = (unsigned)(j0 + 3 - P.bp) <= pspan;
    hv.x = in0 ? hv.x : T4_NEG + 1; hv.y = in1 ? hv.y : T4_NEG + 1; hv.z = in2 ? hv.z : T4_NEG + 1; hv.w = in3 ? hv.w : T4_NEG + 1;
    gg.x = (in0 ? gg.x & 0xffffu : 0u) | (in1 ? gg.x & 0xffff0000u : 0u);
    gg.y = (in2 ? gg.y & 0xffffu : 0u) | (in3 ? gg.y & 0xffff0000u : 0u);
}
// ... and its word at column j (the column left of a lane's first)
__device__ __forceinline__ int poa_stage_word(const poa_pred_row &P, int j)
{
    const int wl = poa_pred_word(P, j, T4_NEG + 1);
    return (unsigned)(j - P.bp) <= P.pspan ? wl : T4_NEG + 1;
}
// several predecessors: the running maximum of the lane's Q quads from column jl over the T.np predecessors, per cell for H and
// for H - G1, H - G2; which predecessor won goes into the row's predecessor-choice planes (drow + W, + 2 W, + 3 W).  h: the merged
// words, ga / gb: their gap bytes, hl: the merged word left of jl, no_row: a predecessor had no value row.  (Returned by value:
// written through references into the caller's arrays, the same code costs k_poa_dp_t7 six vector registers)
template <int Q>
struct poa_merged {
    int h[Q][4];
    uint32_t ga[Q], gb[Q];
    int hl;
    bool no_row;
};
template <int Q>
__device__ __forceinline__ poa_merged<Q> poa_stage_merge(const poa_row_view &V, const poa_row_topo &T, int jl, int bal, int W, uint8_t *drow)
{
    poa_merged<Q> M;
    int x1[Q][4], x2[Q][4];
    uint32_t ah[Q], a1[Q], a2[Q];  // which predecessor won: a byte per cell (planes of the direction row)
    uint32_t ahl = 0;
    M.no_row = false;
    M.hl = T4_NEG;
#pragma unroll
    for (int q = 0; q < Q; q++) {
        ah[q] = 0; a1[q] = 0; a2[q] = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { M.h[q][k] = T4_NEG; x1[q][k] = T4_NEG; x2[q][k] = T4_NEG; }
    }
    for (int t = 0; t < T.np; t++) {
        const poa_pred_row P = poa_pred_row_of(V.R, V.plist[T.ps + t]);
        if (__builtin_expect(P.Vq == nullptr, 0)) M.no_row = true;
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int j0 = jl + 4 * q;
            int4 hv;
            uint2 gg;
            poa_pred_quad(P, j0, 0, hv, gg);
            const int hj[4] = {hv.x, hv.y, hv.z, hv.w};
            const uint32_t g16[4] = {gg.x & 0xffffu, gg.x >> 16, gg.y & 0xffffu, gg.y >> 16};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if ((unsigned)(j0 + k - P.bp) <= P.pspan) {
                    const int h = hj[k], c1 = h - (int)(g16[k] & 255u), c2 = h - (int)(g16[k] >> 8);
                    if (h > M.h[q][k]) { M.h[q][k] = h; ah[q] = (ah[q] & ~(255u << (8 * k))) | ((uint32_t)t << (8 * k)); }
                    if (c1 > x1[q][k]) { x1[q][k] = c1; a1[q] = (a1[q] & ~(255u << (8 * k))) | ((uint32_t)t << (8 * k)); }
                    if (c2 > x2[q][k]) { x2[q][k] = c2; a2[q] = (a2[q] & ~(255u << (8 * k))) | ((uint32_t)t << (8 * k)); }
                }
            }
        }
        {
            const int wl = poa_pred_word(P, jl - 1, 0);
            if (jl >= 1 && (unsigned)(jl - 1 - P.bp) <= P.pspan && wl > M.hl) { M.hl = wl; ahl = (uint32_t)t; }
        }
    }
#pragma unroll
    for (int q = 0; q < Q; q++) {
        uint32_t gv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) gv[k] = (uint32_t)(M.h[q][k] - x1[q][k]) | ((uint32_t)(M.h[q][k] - x2[q][k]) << 8);
        M.ga[q] = gv[0] | (gv[1] << 16);
        M.gb[q] = gv[2] | (gv[3] << 16);
        // predecessor-choice planes: M of column j looks at column j - 1 of the predecessors
        const int c = jl + 4 * q - bal;
        if (c >= 0 && c < W) {
            const uint32_t left = q == 0 ? ahl : (ah[q > 0 ? q - 1 : 0] >> 24);
            *(uint32_t *)(drow + (uint32_t)(W + c)) = left | (ah[q] << 8);
            *(uint32_t *)(drow + (uint32_t)(2 * W + c)) = a1[q];
            *(uint32_t *)(drow + (uint32_t)(3 * W + c)) = a2[q];
        }
    }
    return M;
}

// ---- CELLS.  Phase 1, one quad: M / E1 / E2 from the row above (H words, gap bytes ga | gb, hp the word left of the quad; q4 the
// quad's column codes), Ht' (tagged).  hp leaves as the quad's last word.
// (a query character other than A / C / G / T scores 0 against anything: its column code is 0, and the !PLAIN form for such
// queries adds the mismatch term only where the code is not)
template <bool PLAIN>
__device__ __forceinline__ void poa_cells_p1(const poa_row_base &B, uint32_t q4, const int (&H)[4], uint32_t ga, uint32_t gb, int &hp,
                                             int (&htt)[4], int (&e1t)[4], int (&e2t)[4])
{
    const uint32_t eqb = q4 >> B.gsh;
    const uint32_t anyb = PLAIN ? 0u : (q4 | (q4 >> 1) | (q4 >> 2) | (q4 >> 3));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int g = (int)(k < 2 ? ga : gb);
        const int ev1 = (k & 1) ? t4_sub_byte<2>(H[k], g) : t4_sub_byte<0>(H[k], g);
        const int ev2 = (k & 1) ? t4_sub_byte<3>(H[k], g) : t4_sub_byte<1>(H[k], g);
        int m;
        if constexpr (PLAIN) m = (int)__umul24(__builtin_amdgcn_ubfe(eqb, 4u * k, 1u), (uint32_t)B.mm4) + (hp + B.ne4t);
        else
            m = (int)__umul24(__builtin_amdgcn_ubfe(eqb, 4u * k, 1u), (uint32_t)B.mm4) +
                (int)__builtin_amdgcn_ubfe(anyb, 4u * k, 1u) * (B.ne4t - 1) + (hp + 1);
        htt[k] = t4_max3(m, ev1, ev2);
        e1t[k] = ev1;
        e2t[k] = ev2;
        hp = H[k];
    }
}
// the source row, the quad from column j: H(0, 0) = 0, everything else comes out of the insertion scan
__device__ __forceinline__ void poa_cells_source(int j, int (&htt)[4], int (&e1t)[4], int (&e2t)[4])
{
#pragma unroll
    for (int k = 0; k < 4; k++) {
        htt[k] = (j + k == 0 ? 0 : T4_NEG) + 2;
        e1t[k] = T4_NEG + 1;
        e2t[k] = T4_NEG;
    }
}
// the lane's part of the max-plus scan over its 4 Q cells: ht4 (Ht' without tags), the lane's aggregates and its last cell's term,
// in the a-space that base1 / base2 place the lane's first column in.  first_lane: the lane that holds `beg` -- its sb cells left
// of it stay out of the scan (never its last cell; their tags do not matter)
template <int Q>
__device__ __forceinline__ void poa_cells_scan(const poa_row_pen &K, const int (&htt)[Q][4], int (&ht4)[Q][4], bool first_lane, int sb, int base1,
                                               int base2, int &agg1, int &agg2, int &alast1, int &alast2)
{
    int a1 = POA_IDENT, a2 = POA_IDENT;
#pragma unroll
    for (int q = 0; q < Q; q++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = 4 * q + k;
            int h4 = htt[q][k] & ~3;
            if (c < 4 * Q - 1) h4 = (first_lane && c < sb) ? POA_IDENT : h4;
            ht4[q][k] = h4;
            const int r1 = h4 + 4 * K.e1 * c, r2 = h4 + 4 * K.e2 * c;
            a1 = r1 > a1 ? r1 : a1;
            a2 = r2 > a2 ? r2 : a2;
            if (c == 4 * Q - 1) { alast1 = r1 + base1; alast2 = r2 + base2; }
        }
    agg1 = a1 + base1;
    agg2 = a2 + base2;
}
// Phase 2, quad q of the lane: H'' = max3(Ht, F1, F2) -> the cell words h, the gap bytes ga / gb and the direction dword.  R1 / R2:
// the running insertion terms, L1 / L2: those of the cell to the left; both move on to the next quad
__device__ __forceinline__ void poa_cells_p2(const poa_row_pen &K, int q, const int (&ht4)[4], const int (&htt)[4], const int (&e1t)[4],
                                             const int (&e2t)[4], int &R1, int &R2, int &L1, int &L2, int (&h_out)[4], uint32_t &ga_out,
                                             uint32_t &gb_out, uint32_t &dir_out)
{
    int dirq = 0, ga = 0, gbb = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = 4 * q + k;
        const int h4 = ht4[k];
        const int f1 = R1 - (4 * (K.o1 + K.e1 * c) - 1), f2 = R2 - 4 * (K.o2 + K.e2 * c);
        const int hh = t4_max3(h4 | 3, f1, f2);
        const int h = (hh & ~3) | 1;
        int acc = (hh << 2) | (htt[k] & 3);
        const int u1 = h - e1t[k], u2 = h - e2t[k];
        if (k == 0) { t5_min_byte<0>(ga, u1, K.D1); t5_min_byte<1>(ga, u2, K.D2); }
        if (k == 1) { t5_min_byte<2>(ga, u1, K.D1); t5_min_byte<3>(ga, u2, K.D2); }
        if (k == 2) { t5_min_byte<0>(gbb, u1, K.D1); t5_min_byte<1>(gbb, u2, K.D2); }
        if (k == 3) { t5_min_byte<2>(gbb, u1, K.D1); t5_min_byte<3>(gbb, u2, K.D2); }
        t4_flag_ne(acc, R1, L1);
        if (k == 0) t4_flag_ne_dep<0>(dirq, acc, R2, L2);
        if (k == 1) t4_flag_ne_dep<1>(dirq, acc, R2, L2);
        if (k == 2) t4_flag_ne_dep<2>(dirq, acc, R2, L2);
        if (k == 3) t4_flag_ne_dep<3>(dirq, acc, R2, L2);
        L1 = h4 + 4 * K.e1 * c; L2 = h4 + 4 * K.e2 * c;
        R1 = L1 > R1 ? L1 : R1;
        R2 = L2 > R2 ? L2 : R2;
        h_out[k] = h;
    }
    const uint32_t ya = (uint32_t)ga + K.e_probe, yb = ((uint32_t)gbb + K.e_probe) >> 1;
    const uint32_t e8 = (ya & 0x80808080u) | (yb & ~0x80808080u);
    dir_out = (e8 & 0xC0C0C0C0u) | ((uint32_t)dirq & ~0xC0C0C0C0u);
    ga_out = (uint32_t)ga + K.g_bias;
    gb_out = (uint32_t)gbb + K.g_bias;
}

// ---- epilogue, one wave: the result, the traceback (k_poa_dp_t5's, out of the same records and direction rows), the pool.
// sink_val / sink_row1: the best sink row's value and row + 1 (0: none); ring_bytes: what the problem held of its state region
__device__ __forceinline__ void poa_row_finish(const poa_t5_args &A, const poa_prob &pb, const uint32_t *preds, tb_lds &tb, int tid, bool failed,
                                               int status, int sink_val, uint32_t sink_row1, const poa_row_counts &N, const poa_chunks &C,
                                               uint64_t ring_bytes, uint32_t state_slot)
{
    poa_out &O = A.outs[blockIdx.x];
    uint32_t start_row = 0;
    if (failed) { if (status == POA_ST_OK) status = POA_ST_POOL; }
    else {
        start_row = sink_row1 ? sink_row1 - 1 : 0u;
        status = (sink_row1 != 0 && sink_val > POA_NEG / 2) ? POA_ST_OK : POA_ST_NOALN;
    }
    if (tid == 0) {
        O.cells = failed ? 0 : N.cells; O.vcells = failed ? 0 : N.vcells; O.maxw = failed ? 0u : (uint32_t)N.maxw;
        O.score = failed ? POA_NEG : sink_val;
        O.row = start_row;
        O.status = status;
    }
    if (A.tb_ops) poa_traceback_wave<2>(tb, tid, pb, A.rows, preds, nullptr, O, A.tb_ops, A.tb_orow, 0, status, start_row);
    if (tid == 0) {
        O.t_end = __builtin_amdgcn_s_memrealtime();
        if (C.own_head != POA_NIL) poa_chunk_push(A.cp, blockIdx.x, C.own_head, C.own_tail);
        (void)atomicAdd(A.pool_next, (unsigned long long)C.own_chunks * POA_CHUNK + ring_bytes);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        (void)atomicExch(&A.cp.slot_flag[state_slot], 0u);
    }
}
