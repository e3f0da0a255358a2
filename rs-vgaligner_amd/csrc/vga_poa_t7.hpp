// vga_poa_t7.hpp -- K4 "t7": k_poa_dp_t6's row (eight columns per lane, a row loop whose scalar state fits the scalar registers,
// row maximum resolved once per row) for bands that do not fit a wave: NT / 64 waves per problem, the row above in LDS by absolute
// column (k_poa_dp_t5's window, 6 bytes per column), one workgroup barrier per step for the cross-wave part of the max-plus scan and
// one at the end of a row.  Same recurrences, direction dwords, value rows, row records, chunk pool and fused traceback as
// k_poa_dp_t5 / k_poa_dp_t6 (bit-exact against oracle/og_poa.c), so the kernels are interchangeable problem by problem.
//   * A lane owns 8 consecutive columns of a step (two quads), a wave 512, a step NT * 8.  Per cell that halves what a step pays for
//     the wave scan, the cross-wave exchange, the addresses of its loads and stores and the loop around it.
//   * The row above is read before a step's barrier and written back after it (in place, as t5); the first lane of a later step
//     takes the column left of it from a word the last lane parked.
//   * Band edges: a wave whose 512 columns lie inside the predecessor's band reads it as it is; the (at most two) others mask the
//     cells outside it.  Cells right of `end` are written back far below every real score, so the row maximum needs no band test.
//   * Row maximum: a lane keeps its best word and the first / last step it saw it in; the columns are found once per row from the
//     lane's own cells in LDS, the wave's triple goes to LDS, every wave combines the NW triples at the top of the next row (t5).
// Handed back with POA_ST_RETRY (and re-run by k_poa_dp_t5 at once): a row wider than the LDS window, classic pool mode.
#pragma once

#include <type_traits>

#include "vga_poa_row.hpp"

template <int NT, bool DEF>
__global__ __launch_bounds__(NT) void k_poa_dp_t7(const poa_prob *__restrict__ probs, const char *__restrict__ queries,
                                                  const uint4 *__restrict__ node_tab, const uint32_t *__restrict__ seq32,
                                                  const uint32_t *__restrict__ preds, const poa_t5_args A)
{
    constexpr int NW = NT / 64;
    constexpr int CPL = 8, Q = 2;
    constexpr int STEP = NT * CPL;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    int4 *sX = (int4 *)smem;                  // [2][NW] {scan1, scan2, last1, last2} per wave
    int4 *sRed = sX + 2 * NW;                 // [NW] {row max, leftmost, rightmost, 0} per wave
    int32_t *edgeW = (int32_t *)(sRed + NW);  // [2] (+2 pad) the word left of a later step's first column
    int32_t *sSink = edgeW + 4;               // [0] H of the sink column, [1] state slot hand-over, [2] best sink value, [3] its row + 1
    uint64_t *sChunk = (uint64_t *)(sSink + 4);  // [4] a new chunk's index
    constexpr int HDR = (3 * NW + 1 + 1 + 2) * 16;
    const uint32_t lds_cols = t5_own(A.lds_cols), hg_cols = t5_own(A.hg_cols);
    const int wmask = (int)(hg_cols - 1u);  // (a power of two: the host sees to it)
    int32_t *Hs = (int32_t *)(smem + HDR);                                // [hg_cols] 4 H + 1
    uint16_t *Gs = (uint16_t *)(smem + HDR + 4ull * hg_cols);             // [hg_cols] G1 | G2 << 8
    uint16_t *Qn = (uint16_t *)(smem + HDR + 6ull * hg_cols);             // [lds_cols / 4] four one-hot column codes per halfword

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (tid == 0) A.outs[blockIdx.x].t_begin = __builtin_amdgcn_s_memrealtime();
    if (A.prio) __builtin_amdgcn_s_setprio(3);
    const poa_prob pb = probs[blockIdx.x];
    const poa_row_view V = poa_row_view_of(pb, queries, node_tab, seq32, preds, A);
    const poa_row_pen K = poa_row_pen_of<DEF>(A.P);
    const int e1 = K.e1, e2 = K.e2;

    // ---- a state region (ring of value rows) and chunks for the direction rows: as k_poa_dp_t5 in chunk-pool mode
    int status = POA_ST_OK;
    int got = -1;
    if (A.cp.n_slots != 0 && !(pb.flags & 1u)) {
        if (tid == 0) sSink[1] = poa_slot_acquire(A.cp.slot_flag, A.cp.n_slots, blockIdx.x);
        __syncthreads();
        got = __builtin_amdgcn_readfirstlane(sSink[1]);
    }
    uint64_t state_lo;
    if (!poa_row_state(A, got, tid == 0, state_lo)) return;
    const uint32_t state_slot = (uint32_t)got;
    poa_chunks C = {POA_NIL, POA_NIL, 0, 0, 0};
    bool failed = false;
    // one thread pops, the workgroup hears of it through LDS -- every wave reaches this branch in the same row (its condition is
    // replicated state)
    auto alloc = [&](uint32_t bytes_asked) -> uint64_t {
        const uint32_t bytes = (bytes_asked + 15u) & ~15u;
        if (__builtin_expect(bytes > C.drem, 0)) {
            if (bytes > POA_CHUNK) { failed = true; return C.dcur; }
            if (tid == 0) {
                const uint32_t idx = poa_chunks_pop(A.cp, C);
                sChunk[0] = idx == POA_NIL ? 0ull : poa_chunk_addr(A.cp, idx);
                sChunk[1] = idx;
            }
            __syncthreads();
            const uint32_t idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sChunk[1]);
            const uint64_t a = poa_uniform_u64(sChunk[0]);
            __syncthreads();
            if (idx == POA_NIL) { failed = true; return C.dcur; }
            poa_chunks_took(C, idx, a);
        }
        return poa_chunks_bump(C, bytes);
    };

    const int non_acgt = poa_row_codes(Qn, V.query, V.qlen, (int)(lds_cols / 4), tid, NT);
    if (tid == 0) { sSink[2] = POA_NEG; sSink[3] = 0; }
    const bool q_plain = __builtin_amdgcn_readfirstlane(__syncthreads_or(non_acgt)) == 0;
    // a row of this kernel is never wider than the window, nor than the query
    const uint32_t ring_size = (6u * ((hg_cols < (uint32_t)V.qlen + 8u ? hg_cols : (uint32_t)V.qlen + 8u) + 8u) + 15u) & ~15u;
    const uint64_t ring_base = state_lo;
    if ((uint64_t)ring_size * V.ring_rows > A.cp.state_size) { failed = true; status = POA_ST_RETRY; }
    uint32_t ring_head = 0;

    int prev_beg = 0, prev_end = -1;
    uint32_t seq_word = 0, seq_word_idx = 0xFFFFFFFFu;
    poa_row_counts N = {0, 0, 0};

    for (uint32_t v = 0; v < V.n_nodes && !failed; v++) {
    const uint4 nt = V.ntab[v];
    const uint32_t nlen = nt.y & 0xFFFFFFu;
    for (uint32_t tn = 0; tn < nlen && !failed; tn++) {
        POA_MARK("t7_row");
        const poa_row_topo T = poa_row_topo_of(nt, v, tn, V.seqw, seq_word, seq_word_idx);
        const uint32_t r = T.r;
        const bool last = T.last, is_sink = T.is_sink, simple = T.simple;
        const int np = T.np;
        // ---- the previous row's maximum: every wave combines the waves' triples (k_poa_dp_t5)
        int prev_lmax = 0, prev_rmax = 0;
        if (r > 0) {
            int4 rw = make_int4(INT32_MIN, INT32_MAX, INT32_MIN, 0);
            if (lane < NW) rw = sRed[lane];
            int b = rw.x, t;
            t = poa_dpp<0x111, 0xf>(INT32_MIN, b); b = t > b ? t : b;
            if (NW > 2) { t = poa_dpp<0x112, 0xf>(INT32_MIN, b); b = t > b ? t : b; }
            if (NW > 4) { t = poa_dpp<0x114, 0xf>(INT32_MIN, b); b = t > b ? t : b; }
            if (NW > 8) { t = poa_dpp<0x118, 0xf>(INT32_MIN, b); b = t > b ? t : b; }
            const int rbest = __builtin_amdgcn_readlane(b, NW - 1);
            const uint64_t tie = __builtin_amdgcn_ballot_w64(rw.x == rbest);
            if (__builtin_expect(__builtin_popcountll(tie) == 1, 1)) {
                const int w1 = __builtin_ctzll(tie);
                prev_lmax = __builtin_amdgcn_readlane(rw.y, w1);
                prev_rmax = __builtin_amdgcn_readlane(rw.z, w1);
            } else {
                int lm = rw.x == rbest ? rw.y : INT32_MAX, rm = rw.x == rbest ? rw.z : INT32_MIN;
                t = poa_dpp<0x111, 0xf>(INT32_MAX, lm); lm = t < lm ? t : lm;
                t = poa_dpp<0x111, 0xf>(INT32_MIN, rm); rm = t > rm ? t : rm;
                if (NW > 2) {
                    t = poa_dpp<0x112, 0xf>(INT32_MAX, lm); lm = t < lm ? t : lm;
                    t = poa_dpp<0x112, 0xf>(INT32_MIN, rm); rm = t > rm ? t : rm;
                }
                if (NW > 4) {
                    t = poa_dpp<0x114, 0xf>(INT32_MAX, lm); lm = t < lm ? t : lm;
                    t = poa_dpp<0x114, 0xf>(INT32_MIN, rm); rm = t > rm ? t : rm;
                }
                if (NW > 8) {
                    t = poa_dpp<0x118, 0xf>(INT32_MAX, lm); lm = t < lm ? t : lm;
                    t = poa_dpp<0x118, 0xf>(INT32_MIN, rm); rm = t > rm ? t : rm;
                }
                prev_lmax = __builtin_amdgcn_readlane(lm, NW - 1);
                prev_rmax = __builtin_amdgcn_readlane(rm, NW - 1);
            }
            // (rows a later row can name as a far predecessor: node ends -- their record keeps the columns)
            if (tn == 0 && tid == 0) { V.R[r - 1].lmax = prev_lmax; V.R[r - 1].rmax = prev_rmax; }
        }
        // ---- band
        int mpl, mpr;
        if (r == 0) { mpl = 0; mpr = 0; }
        else if (simple) { mpl = prev_lmax + 1; mpr = prev_rmax + 1; }
        else {
            __syncthreads();  // vmcnt(0) + barrier: value rows and row records of far predecessors have landed
            poa_row_far_span(V, T, prev_lmax, prev_rmax, mpl, mpr);
        }
        int beg, end, bal, W;
        poa_row_band(V, T, mpl, mpr, beg, end, bal, W);
        const int nbase = beg & ~7;  // the first lane's first column
        if ((uint32_t)(end - nbase + 1 + 8) > hg_cols) { failed = true; status = POA_ST_RETRY; break; }  // (wider than the LDS window)
        const uint64_t doff = alloc(poa_row_dir_bytes(W, np));
        uint64_t voff = 0;
        if (last && !failed)
            voff = poa_row_value_in_chunk(T, nt) ? alloc(6u * (uint32_t)W) : poa_row_ring_slot(ring_base, ring_size, V.ring_rows, ring_head);
        if (__builtin_expect(failed, 0)) break;
        poa_row_record(V.R, T, tid == 0, beg, end, W, doff, voff, N);
        uint8_t *drow = (uint8_t *)doff;
        uint8_t *Vrow = (uint8_t *)voff;
        const poa_row_base B = poa_row_base_of(T.gb, V.p_match, V.p_mismatch);

        int pbeg = prev_beg, pend = prev_end;  // where the row above is defined
        if (!simple && r > 0) {
            POA_MARK("t7_stage");
            // ---- STAGING (k_poa_dp_t5's): the virtual predecessor row of the predecessors' value rows, into LDS
            // (a predecessor without a value row -- vga_poa_t5.hpp, staging: the problem is given up, by every wave alike)
            for (int t = 0; t < np; t++) failed |= poa_uniform_u64(V.R[np == 1 ? T.ps : V.plist[T.ps + t]].voff) == 0;
            if (__builtin_expect(failed, 0)) break;
            for (int c0 = 0; nbase + c0 <= end; c0 += STEP) {
                const int jl = nbase + c0 + CPL * tid;
                if (jl > end) continue;
                if (np == 1) {
                    const poa_pred_row P = poa_pred_row_of(V.R, T.ps);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        const int j0 = jl + 4 * q;
                        int4 hv;
                        uint2 gg;
                        poa_stage_quad(P, j0, hv, gg);
                        *(int4 *)(Hs + (j0 & wmask)) = hv;
                        *(uint2 *)(Gs + (j0 & wmask)) = gg;
                    }
                    if (c0 == 0 && tid == 0 && nbase > 0) Hs[(nbase - 1) & wmask] = poa_stage_word(P, jl - 1);
                } else {
                    const poa_merged<Q> M = poa_stage_merge<Q>(V, T, jl, bal, W, drow);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        const int j0 = jl + 4 * q;
                        *(int4 *)(Hs + (j0 & wmask)) = make_int4(M.h[q][0], M.h[q][1], M.h[q][2], M.h[q][3]);
                        *(uint2 *)(Gs + (j0 & wmask)) = make_uint2(M.ga[q], M.gb[q]);
                    }
                    if (c0 == 0 && tid == 0 && nbase > 0) Hs[(nbase - 1) & wmask] = M.hl;
                }
            }
            POA_LDS_BARRIER();
            // the virtual row is defined on every column the row can look at
            pbeg = nbase > 0 ? nbase - 1 : 0;
            pend = INT32_MAX / 2;
        }

        // ---- steps of NT * 8 columns
        int best = INT32_MIN, bfirst = 0, blast = 0;
        int carry1 = POA_IDENT, carry2 = POA_IDENT, left1 = POA_IDENT, left2 = POA_IDENT;
        int buf = 0;
        for (int c0 = 0; nbase + c0 <= end; c0 += STEP, buf ^= 1) {
            const int jw0 = nbase + c0 + 64 * CPL * wv;  // the wave's first column
            const int j0 = jw0 + CPL * lane;
            const bool wave_act = jw0 <= end;
            const bool more = nbase + c0 + STEP <= end;  // another step follows (then every wave is active in this one)
            const int base1 = 4 * e1 * j0, base2 = 4 * e2 * j0;  // (the scan runs in absolute "a-space" across waves and steps)
            int H[Q][4];
            uint32_t Ga[Q], Gb[Q];
            int htt[Q][4], ht4[Q][4], e1t[Q][4], e2t[Q][4];
            int agg1 = POA_IDENT, agg2 = POA_IDENT, alast1 = POA_IDENT, alast2 = POA_IDENT;
            POA_MARK("t7_p1");
            if (wave_act) {
                if (__builtin_expect(r > 0, 1)) {
                    // the row above: eight words, eight gap-byte pairs, the codes of the eight columns
                    {
                        const int4 h0 = *(const int4 *)(Hs + (j0 & wmask)), h1 = *(const int4 *)(Hs + ((j0 + 4) & wmask));
                        const uint4 g = *(const uint4 *)(Gs + (j0 & wmask));
                        H[0][0] = h0.x; H[0][1] = h0.y; H[0][2] = h0.z; H[0][3] = h0.w;
                        H[1][0] = h1.x; H[1][1] = h1.y; H[1][2] = h1.z; H[1][3] = h1.w;
                        Ga[0] = g.x; Gb[0] = g.y; Ga[1] = g.z; Gb[1] = g.w;
                    }
                    const uint32_t qq = *(const uint32_t *)(Qn + (j0 >> 2));
                    // the word left of the wave: the last word of the wave before (same step: not written yet), or -- first wave of
                    // a later step -- what the last lane parked
                    int left0;
                    if (wv == 0 && c0 > 0) left0 = edgeW[buf ^ 1];
                    else left0 = Hs[(jw0 > 0 ? jw0 - 1 : 0) & wmask];
                    if (more && tid == NT - 1) edgeW[buf] = H[1][3];
                    // band edges of the row above (uniform per wave)
                    if (__builtin_expect(jw0 <= pbeg || jw0 + 64 * CPL - 1 > pend, 0)) {
#pragma unroll
                        for (int q = 0; q < Q; q++)
#pragma unroll
                            for (int k = 0; k < 4; k++) {
                                const int j = j0 + 4 * q + k;
                                H[q][k] = (j < pbeg || j > pend) ? T4_NEG + 1 : H[q][k];
                            }
                        left0 = (jw0 - 1 < pbeg || jw0 - 1 > pend || jw0 == 0) ? T4_NEG + 1 : left0;
                    }
                    int hp = t4_shr1_mov(H[1][3], left0);
                    auto cells = [&](auto plain_c) {
#pragma unroll
                        for (int q = 0; q < Q; q++)
                            poa_cells_p1<decltype(plain_c)::value>(B, q == 0 ? qq & 0xffffu : qq >> 16, H[q], Ga[q], Gb[q], hp, htt[q], e1t[q], e2t[q]);
                    };
                    if (__builtin_expect(q_plain, 1)) cells(std::true_type{});
                    else cells(std::false_type{});
                } else {
#pragma unroll
                    for (int q = 0; q < Q; q++) poa_cells_source(j0 + 4 * q, htt[q], e1t[q], e2t[q]);
                }
                POA_MARK("t7_scan");
                // (cells of the very first lane left of beg stay out of the scan)
                poa_cells_scan<Q>(K, htt, ht4, tid == 0 && c0 == 0, beg - nbase, base1, base2, agg1, agg2, alast1, alast2);
            }
            int i1 = POA_IDENT, i2 = POA_IDENT;
            if (wave_act) { i1 = poa_wave_scan_max(agg1); i2 = poa_wave_scan_max(agg2); }
            if (lane == 63) sX[buf * NW + wv] = make_int4(i1, i2, alast1, alast2);
            POA_LDS_BARRIER();
            POA_MARK("t7_exchange");
            int pre1 = carry1, pre2 = carry2, pl1 = left1, pl2 = left2;
            if ((wave_act && wv > 0) || more) {
                int4 x = make_int4(POA_IDENT, POA_IDENT, POA_IDENT, POA_IDENT);
                if (lane < NW) x = sX[buf * NW + lane];
                int s1 = x.x, s2 = x.y, t;
                t = poa_dpp<0x111, 0xf>(INT32_MIN, s1); s1 = t > s1 ? t : s1;
                t = poa_dpp<0x111, 0xf>(INT32_MIN, s2); s2 = t > s2 ? t : s2;
                if (NW > 2) {
                    t = poa_dpp<0x112, 0xf>(INT32_MIN, s1); s1 = t > s1 ? t : s1;
                    t = poa_dpp<0x112, 0xf>(INT32_MIN, s2); s2 = t > s2 ? t : s2;
                }
                if (NW > 4) {
                    t = poa_dpp<0x114, 0xf>(INT32_MIN, s1); s1 = t > s1 ? t : s1;
                    t = poa_dpp<0x114, 0xf>(INT32_MIN, s2); s2 = t > s2 ? t : s2;
                }
                if (NW > 8) {
                    t = poa_dpp<0x118, 0xf>(INT32_MIN, s1); s1 = t > s1 ? t : s1;
                    t = poa_dpp<0x118, 0xf>(INT32_MIN, s2); s2 = t > s2 ? t : s2;
                }
                if (wv > 0) {
                    const int a = __builtin_amdgcn_readlane(s1, wv - 1), b = __builtin_amdgcn_readlane(s2, wv - 1);
                    pre1 = a > pre1 ? a : pre1;
                    pre2 = b > pre2 ? b : pre2;
                    pl1 = __builtin_amdgcn_readlane(x.z, wv - 1);
                    pl2 = __builtin_amdgcn_readlane(x.w, wv - 1);
                }
                if (more) {
                    const int a = __builtin_amdgcn_readlane(s1, NW - 1), b = __builtin_amdgcn_readlane(s2, NW - 1);
                    carry1 = a > carry1 ? a : carry1;
                    carry2 = b > carry2 ? b : carry2;
                    left1 = __builtin_amdgcn_readlane(x.z, NW - 1);
                    left2 = __builtin_amdgcn_readlane(x.w, NW - 1);
                }
            }
            if (wave_act) {
                POA_MARK("t7_p2");
                const int run1_ = t4_shr1_max(i1, pre1), run2_ = t4_shr1_max(i2, pre2);
                const int la1_ = t4_shr1_mov(alast1, pl1), la2_ = t4_shr1_mov(alast2, pl2);
                int R1 = run1_ - base1, R2 = run2_ - base2, L1 = la1_ - base1, L2 = la2_ - base2;
                uint32_t dirs[Q];
                const bool edge_out = jw0 + 64 * CPL - 1 > end;  // the wave that holds `end`: what lies right of it is written back clean
#pragma unroll
                for (int q = 0; q < Q; q++) poa_cells_p2(K, q, ht4[q], htt[q], e1t[q], e2t[q], R1, R2, L1, L2, H[q], Ga[q], Gb[q], dirs[q]);
                if (__builtin_expect(edge_out, 0)) {
#pragma unroll
                    for (int q = 0; q < Q; q++)
#pragma unroll
                        for (int k = 0; k < 4; k++) H[q][k] = j0 + 4 * q + k > end ? T4_NEG + 1 : H[q][k];
                }
                if (__builtin_expect(is_sink, 0)) {
                    const int kq = V.qlen - j0;
#pragma unroll
                    for (int q = 0; q < Q; q++)
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (kq == 4 * q + k) sSink[0] = H[q][k];
                }
                // the lane's best word and the first / last step it was seen in
                {
                    const int m3 = t4_max3(H[0][0], H[0][1], H[0][2]), n3 = t4_max3(H[1][0], H[1][1], H[1][2]);
                    const int m4 = t4_max3(m3, n3, H[0][3]);
                    const int m8 = m4 > H[1][3] ? m4 : H[1][3];
                    const bool gt = m8 > best;
                    best = gt ? m8 : best;
                    bfirst = gt ? c0 : bfirst;
                    blast = m8 >= best ? c0 : blast;
                }
                POA_MARK("t7_stores");
                if (j0 <= end) {
                    *(int4 *)(Hs + (j0 & wmask)) = make_int4(H[0][0], H[0][1], H[0][2], H[0][3]);
                    *(int4 *)(Hs + ((j0 + 4) & wmask)) = make_int4(H[1][0], H[1][1], H[1][2], H[1][3]);
                    *(uint4 *)(Gs + (j0 & wmask)) = make_uint4(Ga[0], Gb[0], Ga[1], Gb[1]);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        const int c = j0 + 4 * q - bal;
                        if (c >= 0 && c < W) {
                            *(uint32_t *)(drow + (uint32_t)c) = dirs[q];
                            if (last) {
                                *(int4 *)(Vrow + 4u * (uint32_t)c) = make_int4(H[q][0], H[q][1], H[q][2], H[q][3]);
                                *(uint2 *)(Vrow + (uint32_t)(4 * W + 2 * c)) = make_uint2(Ga[q], Gb[q]);
                            }
                        }
                    }
                }
            }
        }
        POA_MARK("t7_rowmax");
        // ---- the wave's (maximum, leftmost, rightmost column): from the lane's own cells of the steps it saw its best word in
        {
            const int wb = __builtin_amdgcn_readlane(poa_wave_scan_max(best), 63);
            int lcol = INT32_MAX, rcol = INT32_MIN;
            if (best == wb && wb != INT32_MIN) {
                const int jf = nbase + bfirst + 64 * CPL * wv + CPL * lane, jl2 = nbase + blast + 64 * CPL * wv + CPL * lane;
                const int4 f0 = *(const int4 *)(Hs + (jf & wmask)), f1 = *(const int4 *)(Hs + ((jf + 4) & wmask));
                const int4 l0 = *(const int4 *)(Hs + (jl2 & wmask)), l1 = *(const int4 *)(Hs + ((jl2 + 4) & wmask));
                const int hf[8] = {f0.x, f0.y, f0.z, f0.w, f1.x, f1.y, f1.z, f1.w};
                const int hl[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
                int cf = 0, cl = 0;
#pragma unroll
                for (int c = 7; c >= 0; c--) cf = hf[c] == wb ? c : cf;
#pragma unroll
                for (int c = 0; c < 8; c++) cl = hl[c] == wb ? c : cl;
                lcol = jf + cf;
                rcol = jl2 + cl;
            }
            lcol = poa_wave_scan_min(lcol);
            rcol = poa_wave_scan_max(rcol);
            if (lane == 63) sRed[wv] = make_int4(wb, lcol, rcol, 0);
        }
        POA_LDS_BARRIER();
        if (__builtin_expect(is_sink, 0) && tid == 0) {  // (the next sink row's phase 2 is at least one barrier away)
            const int val = (V.qlen >= beg && V.qlen <= end) ? sSink[0] >> 2 : POA_NEG;
            if (sSink[3] == 0 || val > sSink[2]) { sSink[2] = val; sSink[3] = (int)r + 1; }
        }
        prev_beg = beg; prev_end = end;
    }
    }
    __syncthreads();
    // (the last row of the problem: its maximum's columns go into its record like every node end's -- nothing reads them)
    if (tid >= 64) return;
    // ---- epilogue, first wave
    int sink_best = POA_NEG, sr = 0;
    if (!failed) {
        sink_best = __builtin_amdgcn_readfirstlane(sSink[2]);
        sr = __builtin_amdgcn_readfirstlane(sSink[3]);
    }
    poa_row_finish(A, pb, preds, *(tb_lds *)(smem + HDR), tid, failed, status, sink_best, (uint32_t)sr, N, C, (uint64_t)ring_size * V.ring_rows, state_slot);
}
