// vga_poa_t6.hpp -- K4 "t6": ONE WAVE PER PROBLEM for narrow bands (config 5: mean band 340 columns, widest rows 350-700).
// Same recurrences, direction dwords, value rows, row records and fused traceback as k_poa_dp_t5 (bit-exact against
// oracle/og_poa.c), but the row state never leaves the registers and nothing is exchanged between waves:
//   * a lane owns CPL consecutive columns (CPL = 8: two quads), the wave a WINDOW of 64 CPL columns anchored at a multiple of
//     CPL at or below the band's first column; H words and G bytes of the row above live in 3 CPL / 2 vector registers.  When
//     the anchor moves (every CPL rows while the band slides along the diagonal) the state moves across lanes: one DPP
//     wave_shl per register for the common step of one lane, ds_bpermute for anything else;
//   * a row wider than the window (config 5: one problem in eight has a stretch of them) runs a SECOND STEP of the same code on
//     a second register set that continues the window (128 virtual lanes); the scan totals of the first step are its carry;
//   * no barriers, no LDS row, no cross-wave scan: the max-plus scan of a row is the lane's serial scan, one DPP wave scan and
//     one wave_shr; the row maximum is a DPP reduction and two ballots;
//   * every row is written CLEAN: cells outside [beg, end] leave the row far below every real score, so no row ever masks what
//     it reads -- the per-cell band tests of k_poa_dp_t5's edge wave-steps (every wave-step is one when a row is a single
//     step) shrink to one select per cell on the way out and one on the way into the scan;
//   * rows whose predecessors are not the row above (first row of a node behind a bubble, several predecessors) build the
//     virtual predecessor row of k_poa_dp_t5's staging pass straight into the registers from the predecessors' value rows;
//   * the row loop's scalar state is small enough to stay in scalar registers (k_poa_dp_t5 keeps ~200 scalars alive and
//     pays ~45 v_readlane / v_writelane per wave and row for the ones that spill).
// What it does not do is handed back with POA_ST_RETRY and runs in k_poa_dp_t5: a row whose band does not fit two windows,
// a query with characters other than A / C / G / T, anything outside chunk-pool mode.
#pragma once

#include <type_traits>

#include "vga_poa_row.hpp"

// lanes 0..62: v of the lane above; lane 63: fill   (wave_shl:1, bound_ctrl off: the last lane keeps the old value)
__device__ __forceinline__ int t6_shl1(int v, int fill)
{
    int r = fill;
    asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shl:1 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(v));
    return r;
}
// any lane distance d (new[l] = old[l + d], `fill` where l + d leaves the wave)
__device__ __forceinline__ int t6_shift(int v, int fill, int src_lane_bytes, bool in_range)
{
    const int t = __builtin_amdgcn_ds_bpermute(src_lane_bytes, v);
    return in_range ? t : fill;
}

template <int CPL, bool DEF>
__global__ __launch_bounds__(64) void k_poa_dp_t6(const poa_prob *__restrict__ probs, const char *__restrict__ queries,
                                                  const uint4 *__restrict__ node_tab, const uint32_t *__restrict__ seq32,
                                                  const uint32_t *__restrict__ preds, const poa_t5_args A)
{
    static_assert(CPL == 8 || CPL == 12 || CPL == 16, "two to four quads per lane");
    constexpr int Q = CPL / 4;
    constexpr int WIN = 64 * CPL;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t *Qn = (uint16_t *)smem;  // [lds_cols / 4] four one-hot column codes per halfword (as k_poa_dp_t5); the traceback's staging area later

    const int lane = threadIdx.x;
    if (lane == 0) A.outs[blockIdx.x].t_begin = __builtin_amdgcn_s_memrealtime();
    const poa_prob pb = probs[blockIdx.x];
    const poa_row_view V = poa_row_view_of(pb, queries, node_tab, seq32, preds, A);
    const uint32_t lds_cols = t5_own(A.lds_cols);
    const poa_row_pen K = poa_row_pen_of<DEF>(A.P);
    const int e1 = K.e1, e2 = K.e2;

    // ---- a state region (ring of value rows) and, for the direction rows, chunks from the pool: as k_poa_dp_t5 in chunk-pool mode
    int status = POA_ST_OK;
    int got = -1;
    if (A.cp.n_slots != 0 && !(pb.flags & 1u)) {
        if (lane == 0) got = poa_slot_acquire(A.cp.slot_flag, A.cp.n_slots, blockIdx.x);
        got = __builtin_amdgcn_readfirstlane(got);
    }
    uint64_t state_lo;
    if (!poa_row_state(A, got, lane == 0, state_lo)) return;
    const uint32_t state_slot = (uint32_t)got;
    poa_chunks C = {POA_NIL, POA_NIL, 0, 0, 0};
    bool failed = false;
    // lane 0 pops, the wave hears of it by readfirstlane
    auto alloc = [&](uint32_t bytes_asked) -> uint64_t {
        const uint32_t bytes = (bytes_asked + 15u) & ~15u;
        if (__builtin_expect(bytes > C.drem, 0)) {
            uint32_t idx = POA_NIL;
            if (bytes <= POA_CHUNK) {
                if (lane == 0) idx = poa_chunks_pop(A.cp, C);
                idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            }
            if (idx == POA_NIL) { failed = true; return C.dcur; }
            uint64_t a = 0;
            if (lane == 0) a = poa_chunk_addr(A.cp, idx);
            poa_chunks_took(C, idx, poa_uniform_u64(a));
        }
        return poa_chunks_bump(C, bytes);
    };

    const int non_acgt = poa_row_codes(Qn, V.query, V.qlen, (int)(lds_cols / 4), lane, 64);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const bool q_plain = __builtin_amdgcn_ballot_w64(non_acgt != 0) == 0;
    // a row of this kernel never has more than 2 WIN + 4 storage columns: the ring's slots are sized for that
    const uint32_t ring_size = (6u * (uint32_t)(2 * WIN + 8) + 15u) & ~15u;
    const uint64_t ring_base = state_lo;
    if ((uint64_t)ring_size * V.ring_rows > A.cp.state_size || !q_plain) { failed = true; status = POA_ST_RETRY; }
    uint32_t ring_head = 0;

    // ---- the row above, in registers: lane l of set s holds columns wbase + CPL (64 s + l) .. + CPL - 1.  Set 0 is the window
    // every row runs in; set 1 continues it for the rows that are wider (a second step of the same code): it only holds anything
    // while b_live
    int H[2][Q][4];             // cell words 4 H + 1
    uint32_t Ga[2][Q], Gb[2][Q];  // G1 | G2 << 8 of cells 0, 1 / 2, 3 of each quad
    uint32_t qn[2][Q];          // the column codes of the lane's quads (they only change when the window moves)
#pragma unroll
    for (int s = 0; s < 2; s++)
#pragma unroll
        for (int q = 0; q < Q; q++) {
            qn[s][q] = 0; Ga[s][q] = 0; Gb[s][q] = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) H[s][q][k] = T4_NEG + 1;
        }
    bool b_live = false;
    int wbase = 0;  // first column of the window the registers hold (a multiple of CPL)
    bool have_codes = false;
    const int lane_e1 = 4 * e1 * CPL * lane, lane_e2 = 4 * e2 * CPL * lane;  // a-space offset of the lane's first column in its window

    int prev_lmax = 0, prev_rmax = 0;
    uint32_t seq_word = 0, seq_word_idx = 0xFFFFFFFFu;
    int sink_val = POA_NEG;
    uint32_t sink_row1 = 0;  // best sink row + 1 (0: none yet)
    poa_row_counts N = {0, 0, 0};

    for (uint32_t v = 0; v < V.n_nodes && !failed; v++) {
    const uint4 nt = V.ntab[v];
    const uint32_t nlen = nt.y & 0xFFFFFFu;
    for (uint32_t tn = 0; tn < nlen && !failed; tn++) {
        POA_MARK("t6_row");
        const poa_row_topo T = poa_row_topo_of(nt, v, tn, V.seqw, seq_word, seq_word_idx);
        const uint32_t r = T.r;
        const bool last = T.last, simple = T.simple;
        const int np = T.np;
        // ---- band
        int mpl, mpr;
        if (r == 0) { mpl = 0; mpr = 0; }
        else if (simple) { mpl = prev_lmax + 1; mpr = prev_rmax + 1; }
        else {
            // value rows and row records of far predecessors were stored by this wave: they have landed once its stores have
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            poa_row_far_span(V, T, prev_lmax, prev_rmax, mpl, mpr);
        }
        int beg, end, bal, W;
        poa_row_band(V, T, mpl, mpr, beg, end, bal, W);
        const int nbase = (int)((uint32_t)beg / (uint32_t)CPL) * CPL;  // the window this row needs
        if (end - nbase >= 2 * WIN) { failed = true; status = POA_ST_RETRY; break; }
        const bool two = end - nbase >= WIN;  // a second step
        const uint64_t doff = alloc(poa_row_dir_bytes(W, np));
        uint64_t voff = 0;
        if (last && !failed)
            voff = poa_row_value_in_chunk(T, nt) ? alloc(6u * (uint32_t)W) : poa_row_ring_slot(ring_base, ring_size, V.ring_rows, ring_head);
        if (__builtin_expect(failed, 0)) break;
        poa_row_record(V.R, T, lane == 0, beg, end, W, doff, voff, N);
        uint8_t *drow = (uint8_t *)doff;
        uint8_t *Vrow = (uint8_t *)voff;
        const poa_row_base B = poa_row_base_of(T.gb, V.p_match, V.p_mismatch);

        POA_MARK("t6_state");
        int hp0[2];  // the predecessor's word at the column left of the lane's first, per set
        hp0[1] = T4_NEG + 1;
        if (two && !b_live) {
            // the second set comes into use: nothing of the row above lies there
#pragma unroll
            for (int q = 0; q < Q; q++) {
                Ga[1][q] = 0; Gb[1][q] = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) H[1][q][k] = T4_NEG + 1;
            }
            b_live = true;
        }
        if (__builtin_expect(simple, 1)) {
            // ---- the row above is in the registers: move it if the window moves
            hp0[0] = t4_shr1_mov(H[0][Q - 1][3], T4_NEG + 1);
            if (b_live) hp0[1] = t4_shr1_mov(H[1][Q - 1][3], __builtin_amdgcn_readlane(H[0][Q - 1][3], 63));
            const int dl = (nbase - wbase) / CPL;
            if (dl != 0) {
                if (dl == 1 && !b_live) {
                    hp0[0] = t6_shl1(hp0[0], T4_NEG + 1);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) H[0][q][k] = t6_shl1(H[0][q][k], T4_NEG + 1);
                        Ga[0][q] = (uint32_t)t6_shl1((int)Ga[0][q], 0);
                        Gb[0][q] = (uint32_t)t6_shl1((int)Gb[0][q], 0);
                    }
                } else if (dl == 1) {
                    // lane 63 of the first set takes over lane 0 of the second
                    hp0[0] = t6_shl1(hp0[0], __builtin_amdgcn_readlane(hp0[1], 0));
                    hp0[1] = t6_shl1(hp0[1], T4_NEG + 1);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            H[0][q][k] = t6_shl1(H[0][q][k], __builtin_amdgcn_readlane(H[1][q][k], 0));
                            H[1][q][k] = t6_shl1(H[1][q][k], T4_NEG + 1);
                        }
                        Ga[0][q] = (uint32_t)t6_shl1((int)Ga[0][q], __builtin_amdgcn_readlane((int)Ga[1][q], 0));
                        Gb[0][q] = (uint32_t)t6_shl1((int)Gb[0][q], __builtin_amdgcn_readlane((int)Gb[1][q], 0));
                        Ga[1][q] = (uint32_t)t6_shl1((int)Ga[1][q], 0);
                        Gb[1][q] = (uint32_t)t6_shl1((int)Gb[1][q], 0);
                    }
                } else {
                    // any distance: lane l of set s takes what virtual lane 64 s + l + dl held (of 128, the second set only if live)
                    const int s0 = lane + dl, s1 = lane + 64 + dl;
                    const int sb0 = (s0 & 63) << 2, sb1 = (s1 & 63) << 2;
                    const int w0 = s0 >> 6, w1 = s1 >> 6;  // 0: first set, 1: second set, anything else: outside
                    const bool live = b_live;
                    auto move = [&](int &a, int &b, int fill) {
                        const int a0 = __builtin_amdgcn_ds_bpermute(sb0, a), a1 = __builtin_amdgcn_ds_bpermute(sb1, a);
                        int b0 = fill, b1 = fill;
                        if (live) { b0 = __builtin_amdgcn_ds_bpermute(sb0, b); b1 = __builtin_amdgcn_ds_bpermute(sb1, b); }
                        a = w0 == 0 ? a0 : (w0 == 1 ? b0 : fill);
                        b = w1 == 0 ? a1 : (w1 == 1 ? b1 : fill);
                    };
                    move(hp0[0], hp0[1], T4_NEG + 1);
#pragma unroll
                    for (int q = 0; q < Q; q++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) move(H[0][q][k], H[1][q][k], T4_NEG + 1);
                        int x, y;
                        x = (int)Ga[0][q]; y = (int)Ga[1][q]; move(x, y, 0); Ga[0][q] = (uint32_t)x; Ga[1][q] = (uint32_t)y;
                        x = (int)Gb[0][q]; y = (int)Gb[1][q]; move(x, y, 0); Gb[0][q] = (uint32_t)x; Gb[1][q] = (uint32_t)y;
                    }
                }
                have_codes = false;
            }
        } else if (r > 0) {
            // ---- STAGING (k_poa_dp_t5's, into registers): the virtual predecessor row of the predecessors' value rows
            have_codes = false;
            auto stage = [&](auto sc) {
                constexpr int s = decltype(sc)::value;
                const int jl = nbase + CPL * (lane + 64 * s);
                if (np == 1) {
                    const poa_pred_row P = poa_pred_row_of(V.R, T.ps);
                    if (__builtin_expect(P.Vq == nullptr, 0)) failed = true;  // (a predecessor without a value row: vga_poa_t5.hpp, staging)
#pragma unroll
                    for (int q = 0; q < Q; q++) {
                        int4 hv;
                        uint2 gg;
                        poa_stage_quad(P, jl + 4 * q, hv, gg);
                        H[s][q][0] = hv.x; H[s][q][1] = hv.y; H[s][q][2] = hv.z; H[s][q][3] = hv.w;
                        Ga[s][q] = gg.x;
                        Gb[s][q] = gg.y;
                    }
                    hp0[s] = poa_stage_word(P, jl - 1);
                } else {
                    const poa_merged<Q> M = poa_stage_merge<Q>(V, T, jl, bal, W, drow);
                    if (M.no_row) failed = true;
#pragma unroll
                    for (int q = 0; q < Q; q++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) H[s][q][k] = M.h[q][k];
                        Ga[s][q] = M.ga[q];
                        Gb[s][q] = M.gb[q];
                    }
                    hp0[s] = M.hl;
                }
            };
            stage(std::integral_constant<int, 0>{});
            if (two) stage(std::integral_constant<int, 1>{});
        }
        wbase = nbase;
        if (!have_codes) {
            // (a lane's first column is a multiple of 4: the quads' halfwords are adjacent)
#pragma unroll
            for (int s = 0; s < 2; s++)
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const int t = ((nbase + CPL * (lane + 64 * s)) >> 2) + q;
                    qn[s][q] = t < (int)(lds_cols / 4) ? (uint32_t)Qn[t] : 0u;
                }
            have_codes = true;
        }

        // right of `end` the row is cleaned on the way out: virtual lanes above le, and in lane le the cells above se
        const int le = (end - nbase) / CPL, se = (end - nbase) - le * CPL;
        const int sb = beg - nbase;  // 0 .. CPL - 1: cells of the first lane left of beg stay out of the scan
        int bestv[2] = {INT32_MIN, INT32_MIN};
        int tot1 = POA_IDENT, tot2 = POA_IDENT, lst1 = POA_IDENT, lst2 = POA_IDENT;  // what a step hands to the next one
        auto step = [&](auto sc) {
            constexpr int s = decltype(sc)::value;
            const int jl = nbase + CPL * (lane + 64 * s);
            const int le1 = lane_e1 + 4 * e1 * WIN * s, le2 = lane_e2 + 4 * e2 * WIN * s;
            int htt[Q][4], ht4[Q][4], e1t[Q][4], e2t[Q][4];
            POA_MARK("t6_p1");
            // ---- phase 1: M / E1 / E2 from the row above, Ht' (tagged); the lane's part of the max-plus scan
            if (__builtin_expect(r > 0, 1)) {
                int hp = hp0[s];
#pragma unroll
                for (int q = 0; q < Q; q++) poa_cells_p1<true>(B, qn[s][q], H[s][q], Ga[s][q], Gb[s][q], hp, htt[q], e1t[q], e2t[q]);
            } else {
#pragma unroll
                for (int q = 0; q < Q; q++) poa_cells_source(jl + 4 * q, htt[q], e1t[q], e2t[q]);
            }
            POA_MARK("t6_scan");
            int agg1, agg2, alast1 = POA_IDENT, alast2 = POA_IDENT;
            poa_cells_scan<Q>(K, htt, ht4, s == 0 && lane == 0, sb, le1, le2, agg1, agg2, alast1, alast2);
            const int i1 = poa_wave_scan_max(agg1), i2 = poa_wave_scan_max(agg2);
            const int run1_ = t4_shr1_max(i1, tot1), run2_ = t4_shr1_max(i2, tot2);
            const int la1_ = t4_shr1_mov(alast1, lst1), la2_ = t4_shr1_mov(alast2, lst2);
            if (s == 0 && two) {
                const int a = __builtin_amdgcn_readlane(i1, 63), b = __builtin_amdgcn_readlane(i2, 63);
                tot1 = a; tot2 = b;
                lst1 = __builtin_amdgcn_readlane(alast1, 63);
                lst2 = __builtin_amdgcn_readlane(alast2, 63);
            }
            POA_MARK("t6_p2");
            // ---- phase 2: H'' = max3(Ht, F1, F2), the cell words, gap bytes and direction dwords; the row maximum
            int R1 = run1_ - le1, R2 = run2_ - le2, L1 = la1_ - le1, L2 = la2_ - le2;
            int best = INT32_MIN;
            uint32_t dirs[Q];
            const int lg = lane + 64 * s;
#pragma unroll
            for (int q = 0; q < Q; q++) {
                poa_cells_p2(K, q, ht4[q], htt[q], e1t[q], e2t[q], R1, R2, L1, L2, H[s][q], Ga[s][q], Gb[s][q], dirs[q]);
                // clean on the way out
#pragma unroll
                for (int k = 0; k < 4; k++) H[s][q][k] = (lg > le || (lg == le && 4 * q + k > se)) ? T4_NEG + 1 : H[s][q][k];
                const int m3 = t4_max3(H[s][q][0], H[s][q][1], H[s][q][2]);
                const int m4 = m3 > H[s][q][3] ? m3 : H[s][q][3];
                best = m4 > best ? m4 : best;
            }
            bestv[s] = best;
            POA_MARK("t6_stores");
            // ---- stores: direction dwords, and the value row of a node's last base (what a far successor reads)
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const int c = jl + 4 * q - bal;
                if (c >= 0 && c < W) {
                    *(uint32_t *)(drow + (uint32_t)c) = dirs[q];
                    if (last) {
                        *(int4 *)(Vrow + 4u * (uint32_t)c) = make_int4(H[s][q][0], H[s][q][1], H[s][q][2], H[s][q][3]);
                        *(uint2 *)(Vrow + (uint32_t)(4 * W + 2 * c)) = make_uint2(Ga[s][q], Gb[s][q]);
                    }
                }
            }
        };
        step(std::integral_constant<int, 0>{});
        if (__builtin_expect(two, 0)) step(std::integral_constant<int, 1>{});
        b_live = two;
        POA_MARK("t6_rowmax");
        // ---- the row maximum and its leftmost / rightmost column (cells outside the band are far below it)
        {
            const int wb0 = __builtin_amdgcn_readlane(poa_wave_scan_max(bestv[0]), 63);
            int wb = wb0, wb1 = INT32_MIN;
            if (two) { wb1 = __builtin_amdgcn_readlane(poa_wave_scan_max(bestv[1]), 63); wb = wb1 > wb ? wb1 : wb; }
            // one compare per slot gives the holders of the maximum as a lane mask per slot: the first / last holding lane of any slot,
            // then the first / last slot of that lane, are scalar bit tests
            auto first_of = [&](auto sc) {
                constexpr int s = decltype(sc)::value;
                uint64_t m[CPL], any = 0;
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int k = 0; k < 4; k++) { m[4 * q + k] = __builtin_amdgcn_ballot_w64(H[s][q][k] == wb); any |= m[4 * q + k]; }
                const int lf = __builtin_ctzll(any);
                int cf = 0;
#pragma unroll
                for (int c = CPL - 1; c >= 0; c--)
                    if ((m[c] >> lf) & 1ull) cf = c;
                return nbase + CPL * (lf + 64 * s) + cf;
            };
            auto last_of = [&](auto sc) {
                constexpr int s = decltype(sc)::value;
                uint64_t m[CPL], any = 0;
#pragma unroll
                for (int q = 0; q < Q; q++)
#pragma unroll
                    for (int k = 0; k < 4; k++) { m[4 * q + k] = __builtin_amdgcn_ballot_w64(H[s][q][k] == wb); any |= m[4 * q + k]; }
                const int lr = 63 - __builtin_clzll(any);
                int cr = 0;
#pragma unroll
                for (int c = 0; c < CPL; c++)
                    if ((m[c] >> lr) & 1ull) cr = c;
                return nbase + CPL * (lr + 64 * s) + cr;
            };
            if (__builtin_expect(!two, 1)) {
                prev_lmax = first_of(std::integral_constant<int, 0>{});
                prev_rmax = last_of(std::integral_constant<int, 0>{});
            } else {
                prev_lmax = wb0 == wb ? first_of(std::integral_constant<int, 0>{}) : first_of(std::integral_constant<int, 1>{});
                prev_rmax = wb1 == wb ? last_of(std::integral_constant<int, 1>{}) : last_of(std::integral_constant<int, 0>{});
            }
            if (last && lane == 0) { V.R[r].lmax = prev_lmax; V.R[r].rmax = prev_rmax; }
        }
        POA_MARK("t6_sink");
        if (__builtin_expect(T.is_sink, 0)) {
            int val = POA_NEG;
            if (V.qlen >= beg && V.qlen <= end) {
                const int lq = (V.qlen - nbase) / CPL, cs = (V.qlen - nbase) - lq * CPL;
                int w = 0;
#pragma unroll
                for (int s = 0; s < 2; s++)
#pragma unroll
                    for (int q = 0; q < Q; q++)
#pragma unroll
                        for (int k = 0; k < 4; k++)
                            if (cs == 4 * q + k && (lq >> 6) == s) w = __builtin_amdgcn_readlane(H[s][q][k], lq & 63);
                val = w >> 2;
            }
            if (sink_row1 == 0 || val > sink_val) { sink_val = val; sink_row1 = r + 1; }
        }
    }
    }
    // ---- epilogue
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    poa_row_finish(A, pb, preds, *(tb_lds *)smem, lane, failed, status, sink_val, sink_row1, N, C, (uint64_t)ring_size * V.ring_rows, state_slot);
}
