// vga_poa_shape.hpp -- what a POA launch looks like, decided without touching the GPU: the environment switches of the POA host
// (read once per call), the DP kernel family a call's penalties allow, and the launch shape (kernel, workgroup size, LDS column
// window, LDS bytes) of one sub-batch.  Plain C++: no HIP type or call, so that a host compiler builds it alone
// (tests/test_poa_shape_cpu.py pins the selection rules below).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/vga_hip.h"

// ---------------------------------------------------------------------------------------------------------------- LDS sizes
#define POA_LDS_LIMIT ((size_t)(160 * 1024 - 256))  // what a workgroup may ask for on gfx950

#define TB_WIN 32
struct tb_lds {  // 6 912 B: what one wave of the traceback stages per stretch (vga_poa_kernels.hpp: poa_traceback_wave)
    int beg[64], end[64], ws[64];
    uint64_t doff[64];
    uint32_t pred[64], np[64];
    uint32_t dir[64][TB_WIN / 4], pl1[64][TB_WIN / 4], pr4[64][4];
};

static inline uint32_t poa_lds_cols(uint32_t max_q) { return ((max_q + 1 + 15u) & ~15u) + 16u; }

static inline size_t poa_lds_bytes(uint32_t lds_cols, int nt)
{
    const int nw = nt / 64;
    return 7ull * lds_cols + (size_t)(8 * nw + 3 * nw + 2) * 4 + 16;
}

static inline size_t poa_t4_lds_bytes(uint32_t hg_cols, uint32_t lds_cols, int nt)
{
    const int nw = nt / 64;
    return std::max<size_t>(6ull * hg_cols + ((lds_cols / 2 + 15u) & ~15u), sizeof(tb_lds)) + (size_t)(3 * nw + 1 + 4 + 6 + 1) * 16 + 16;
}

static inline size_t poa_t5_lds_bytes(uint32_t hg_cols, uint32_t lds_cols, int nt)
{
    const int nw = nt / 64;
    return std::max<size_t>(6ull * hg_cols + ((lds_cols / 2 + 15u) & ~15u), sizeof(tb_lds)) + (size_t)(3 * nw + 1 + 1 + 2) * 16 + 16;
}

template <int CPL>
static inline size_t poa_t6_lds_bytes(uint32_t lds_cols)
{
    return std::max<size_t>(((size_t)lds_cols / 2 + 15u) & ~(size_t)15u, sizeof(tb_lds)) + 64;
}

// ----------------------------------------------------------------------------------------------------------------- switches
// Every VGA_POA_* / VGA_POOL_* environment switch (testing and diagnostics; DESIGN.md has the table).  Read once at the start of
// a call -- per call, not per process: the GPU tests change them between calls on one context.
struct poa_switches {
    // VGA_POA_KERNEL: a comma list, matched by substring
    bool k_unpacked = false;  // k_poa_dp_lds whatever the penalties
    bool k_t4 = false;        // k_poa_dp_t4 instead of k_poa_dp_t5
    bool k_t5 = false;        // no k_poa_dp_t6 / k_poa_dp_t7 launch
    bool k_t6 = false;        // k_poa_dp_t6 on every launch that can take it, whatever its width estimate
    bool k_t7 = false;        // k_poa_dp_t7 on every launch that can take it
    bool k_full = false;      // every column in LDS
    bool k_generic = false;   // run-time penalties (no default-penalty specialisation)
    int k_nt = 0;             // "128" / "256" / "512": the workgroup size (0: not pinned)
    bool has_nt = false, has_window = false, has_t7_nt = false, has_t7_window = false;
    int nt = 0, t7_nt = 0;            // VGA_POA_NT, VGA_POA_T7_NT
    uint32_t window = 0, t7_window = 0;  // VGA_POA_WINDOW (a power of two; 0: every column), VGA_POA_T7_WINDOW
    bool tb_fused = true;     // VGA_POA_TB: fused unless set without "fused" (then a traceback kernel of its own after the DP)
    bool arenas_off = false;  // VGA_POA_ARENAS=0: classic mode for the whole call
    bool has_arenas = false;  // ... another number caps the state regions
    uint64_t arenas = 0;
    bool has_slots = false, has_sub = false;
    int slots = 0;            // VGA_POA_SLOTS: launches in flight
    uint64_t sub = 0;         // VGA_POA_SUB: problems per sub-batch
    bool giant_prio = true;   // VGA_POA_GIANT_PRIO=0: the launch of a call's longest problems runs at ordinary issue priority
    bool text_host = false;   // VGA_POA_TEXT=host: cs / CIGAR / node path from host threads
    bool text_memcpy = false; // VGA_POA_TEXT_MEMCPY: the device text comes back by hipMemcpy, not by the copy kernel
    bool has_text_arena = false;
    uint64_t text_arena = 0;  // VGA_POA_TEXT_ARENA: caps the text arena (the overflow path)
    bool has_cov_words = false, has_pileup_words = false, has_ins_words = false, has_del_words = false;
    uint64_t cov_words = 0;     // VGA_COV_LIST_WORDS: caps the buffer of run lists (the no-room route; 0: every problem takes it)
    uint64_t pileup_words = 0;  // VGA_PILEUP_LIST_WORDS: the same for the pileup lists
    uint64_t ins_words = 0;     // VGA_INS_LIST_WORDS: the same for the insertion lists
    uint64_t del_words = 0;     // VGA_DEL_LIST_WORDS: the same for the deletion lists
    bool has_dump_rows = false;
    std::string dump_rows;    // VGA_POA_DUMP_ROWS: file for the row records of every launch's first problem
    bool has_pool_fraction = false, has_pool_bytes = false, has_pool_seg = false;
    double pool_fraction = 0; // VGA_POOL_FRACTION: overrides vga_ctx_set_pool_fraction
    uint64_t pool_bytes = 0;  // VGA_POOL_BYTES: caps what the pool may take
    uint64_t pool_seg = 0;    // VGA_POOL_SEG: segment size
    double pool_fill = 0.7;   // VGA_POOL_FILL: fraction of the resident problems' estimate the chunk pool starts with
    bool pool_check = false;  // VGA_POOL_CHECK: chunk ownership is tracked and checked (poa_chunk_pool::owner)
};

static inline poa_switches poa_read_switches()
{
    poa_switches s;
    auto u64 = [](const char *name, bool &has, uint64_t &v) {
        const char *e = getenv(name);
        has = e != nullptr;
        if (e) v = strtoull(e, nullptr, 10);
    };
    if (const char *k = getenv("VGA_POA_KERNEL")) {
        s.k_unpacked = strstr(k, "unpacked") != nullptr;
        s.k_t4 = strstr(k, "t4") != nullptr;
        s.k_t5 = strstr(k, "t5") != nullptr;
        s.k_t6 = strstr(k, "t6") != nullptr;
        s.k_t7 = strstr(k, "t7") != nullptr;
        s.k_full = strstr(k, "full") != nullptr;
        s.k_generic = strstr(k, "generic") != nullptr;
        s.k_nt = strstr(k, "128") ? 128 : (strstr(k, "256") ? 256 : (strstr(k, "512") ? 512 : 0));
    }
    if (const char *e = getenv("VGA_POA_NT")) { s.has_nt = true; s.nt = atoi(e); }
    if (const char *e = getenv("VGA_POA_T7_NT")) { s.has_t7_nt = true; s.t7_nt = atoi(e); }
    if (const char *e = getenv("VGA_POA_WINDOW")) { s.has_window = true; s.window = (uint32_t)strtoul(e, nullptr, 10); }
    if (const char *e = getenv("VGA_POA_T7_WINDOW")) { s.has_t7_window = true; s.t7_window = (uint32_t)strtoul(e, nullptr, 10); }
    if (const char *e = getenv("VGA_POA_TB")) s.tb_fused = strstr(e, "fused") != nullptr;
    if (const char *e = getenv("VGA_POA_ARENAS")) { s.arenas_off = atoi(e) == 0; s.has_arenas = true; s.arenas = strtoull(e, nullptr, 10); }
    if (const char *e = getenv("VGA_POA_SLOTS")) { s.has_slots = true; s.slots = atoi(e); }
    u64("VGA_POA_SUB", s.has_sub, s.sub);
    if (const char *e = getenv("VGA_POA_GIANT_PRIO")) s.giant_prio = atoi(e) != 0;
    if (const char *e = getenv("VGA_POA_TEXT")) s.text_host = strstr(e, "host") != nullptr;
    s.text_memcpy = getenv("VGA_POA_TEXT_MEMCPY") != nullptr;
    u64("VGA_POA_TEXT_ARENA", s.has_text_arena, s.text_arena);
    if (const char *e = getenv("VGA_COV_LIST_WORDS")) { s.has_cov_words = true; s.cov_words = (uint64_t)std::max(0ll, atoll(e)); }
    u64("VGA_PILEUP_LIST_WORDS", s.has_pileup_words, s.pileup_words);
    u64("VGA_INS_LIST_WORDS", s.has_ins_words, s.ins_words);
    u64("VGA_DEL_LIST_WORDS", s.has_del_words, s.del_words);
    if (const char *e = getenv("VGA_POA_DUMP_ROWS")) { s.has_dump_rows = true; s.dump_rows = e; }
    if (const char *e = getenv("VGA_POOL_FRACTION")) { s.has_pool_fraction = true; s.pool_fraction = atof(e); }
    u64("VGA_POOL_BYTES", s.has_pool_bytes, s.pool_bytes);
    u64("VGA_POOL_SEG", s.has_pool_seg, s.pool_seg);
    if (const char *e = getenv("VGA_POOL_FILL")) s.pool_fill = atof(e);
    if (const char *e = getenv("VGA_POOL_CHECK")) s.pool_check = atoi(e) != 0;
    return s;
}

// ------------------------------------------------------------------------------------------------------------------- family
// The DP kernel family of a call: the one decision the LDS admission check, chunk-pool eligibility and every launch go by.
enum poa_family { POA_FAM_LDS, POA_FAM_T4, POA_FAM_T5 };

static inline poa_family poa_choose_family(const vga_poa_params &p, const poa_switches &sw)
{
    const int g1 = p.gap_open1 + p.gap_ext1, g2 = p.gap_open2 + p.gap_ext2;
    // k_poa_dp_t4 (vga_poa_t4.hpp): scores scaled by 4 with argmax tags, G bytes 4 g - 1 / 4 g.  Everything else -- and
    // VGA_POA_KERNEL=unpacked -- is k_poa_dp_lds (any gap penalties that fit a byte per gap state)
    if (sw.k_unpacked || 4 * g1 - 1 > 255 || 4 * g2 > 255 || p.gap_ext1 < 1 || p.match + p.mismatch < 0 || p.match + p.mismatch >= (1 << 20))
        return POA_FAM_LDS;
    // k_poa_dp_t5 (vga_poa_t5.hpp), the default: the same rows under a leaderless row loop; its packed gap-byte arithmetic
    // needs 4 o_k + 1 <= 128, 4 (o1 + e1) <= 255 and 4 (o2 + e2) + 1 <= 255.  VGA_POA_KERNEL=t4 selects k_poa_dp_t4
    if (sw.k_t4 || p.gap_open1 > 31 || p.gap_open2 > 31 || 4 * g2 + 1 > 255 || 4 * g1 > 255) return POA_FAM_T4;
    return POA_FAM_T5;
}

// LDS bytes of the smallest launch the family has for a query of lds_cols column codes: what decides whether a call is admitted.
// k_poa_dp_t4 / k_poa_dp_t5 can shrink their window of the row state down to 512 columns (one figure for both: k_poa_dp_t5's
// header is 112 B smaller); k_poa_dp_lds keeps every column
static inline size_t poa_min_lds_bytes(poa_family family, uint32_t lds_cols)
{
    return family == POA_FAM_LDS ? poa_lds_bytes(lds_cols, 128) : poa_t4_lds_bytes(std::min<uint32_t>(lds_cols, 512), lds_cols, 128);
}

// -------------------------------------------------------------------------------------------------------------------- shape
enum poa_kernel { POA_K_LDS, POA_K_T4, POA_K_T5, POA_K_T6, POA_K_T7 };

static inline const char *poa_kernel_name(poa_kernel k)
{
    static const char *const names[] = {"k_poa_dp_lds", "k_poa_dp_t4", "k_poa_dp_t5", "k_poa_dp_t6", "k_poa_dp_t7"};
    return names[k];
}

struct poa_shape_in {
    uint32_t max_q = 0;            // longest query of the sub-batch
    double mean_w = 0, max_w = 0;  // mean and maximum of its problems' width estimates
    uint64_t left = 0;             // problems of the call from this launch on ...
    uint64_t in_flight = 0;        // ... and those of the launches in flight (they share the GPU with this one)
    uint32_t n_cu = 256;
    bool giant = false;            // the launch of a call's very long problems (poa_feed::klass)
    bool general = false;          // a re-run of what a specialised kernel handed back (POA_ST_RETRY)
    bool arena = false;            // chunk-pool mode
    bool fused = false;            // the DP kernel walks the alignments back itself
    bool default_penalties = false;  // gap penalties 4, 2, 24, 1
    poa_family family = POA_FAM_T5;
};

struct poa_shape {
    poa_kernel kernel = POA_K_T5;
    bool def_pen = false;   // the default-penalty specialisation
    int nt = 0;             // threads per workgroup
    uint32_t lds_cols = 0;  // column codes of the longest query
    uint32_t hg_cols = 0, win_mask = 0xFFFFFFFFu;  // LDS column window (mask 0xFFFFFFFF: every column)
    size_t lds = 0;         // dynamic LDS bytes
    // the shape of the family's own kernel, which a k_poa_dp_t6 / k_poa_dp_t7 launch starts from (else equal to the above): the
    // trace's launch line reports it, and k_poa_dp_t6 is handed its window
    int fam_nt = 0;
    uint32_t fam_cols = 0;
    size_t fam_lds = 0;
};

static inline poa_shape poa_choose_shape(const poa_shape_in &in, const poa_switches &sw)
{
    const bool t4 = in.family != POA_FAM_LDS, t5 = in.family == POA_FAM_T5;
    const uint32_t lds_cols = poa_lds_cols(in.max_q);
    // LDS column window (k_poa_dp_t4 / t5): 4096 columns keep almost every row of a 10 kbp read resident (its widest
    // rows, a few per cent, take the HBM detour described in the kernel) and let five workgroups share a CU.
    // Queries that fit a smaller array anyway keep every column.
    uint32_t hg_cols = lds_cols, win_mask = 0xFFFFFFFFu;
    auto set_window = [&](uint32_t want) {
        hg_cols = lds_cols; win_mask = 0xFFFFFFFFu;
        if (want >= 16 && (want & (want - 1)) == 0 && want < lds_cols) { hg_cols = want; win_mask = want - 1; }
    };
    if (t4 && !sw.k_full) {
        uint32_t want = 4096;
        // narrow bands: a window that just covers the launch's widest estimated row (rows that turn out wider take
        // the HBM detour) leaves room for more two-wave workgroups per CU -- such launches are bound by the latency
        // of the per-row chain, not by instruction issue (config 5: +20 %)
        if (in.mean_w <= 800.0) {
            uint32_t w2 = 512;
            while (w2 < 4096 && (double)w2 < in.max_w * 1.25 + 16.0) w2 <<= 1;
            want = w2;
        }
        // the longest problems of a call have a CU almost to themselves (16 waves, 55-66 KB of LDS) and are often as wide as the
        // query: every column in LDS (62 % of the cells of config 4's 107 000-row problem lie in rows wider than 8 192 columns,
        // 100 % of those of its 34 000-row problems: 24-27 us per row through the HBM detour against 7.6).  A query too long for
        // that falls back to the largest window that fits (below)
        if (in.giant) want = 0;
        if (sw.has_window) want = sw.window;
        set_window(want);
    }
    // workgroup size
    int nt = in.max_q >= 3072 ? 512 : (in.max_q >= 768 ? 256 : 128);
    auto lds_of = [&](int t) { return t5 ? poa_t5_lds_bytes(hg_cols, lds_cols, t) : (t4 ? poa_t4_lds_bytes(hg_cols, lds_cols, t) : poa_lds_bytes(lds_cols, t)); };
    if (t4) {
        // the one that keeps the most waves resident (LDS and 16 wave slots per CU at this kernel's register count
        // bound the workgroups per CU; the problems still to be run -- this sub-batch and the ones that will overlap
        // it -- bound how many there are); ties go to the smaller workgroup, whose barriers are cheaper
        size_t best_waves = 0;
        for (int t = 128; t <= 512; t += 64) {
            const size_t by_lds = std::max<size_t>(1, (160 * 1024) / (lds_of(t) + 256));
            const size_t per_cu = std::min<size_t>(by_lds, (size_t)(16 / (t / 64)));
            const size_t waves = std::min<size_t>(in.left + in.in_flight, per_cu * (size_t)in.n_cu) * (size_t)(t / 64);
            if (waves > best_waves) { best_waves = waves; nt = t; }
        }
        // narrow bands (one step of a 128-thread workgroup covers a typical row): the per-row set-up and the
        // barriers dominate, and they are per wave -- config 5 (mean width 340): +6 % with 128 threads
        if (in.mean_w <= 800.0) nt = 128;  // (the estimate is of a problem's widest rows: about twice its mean band)
        if (in.giant) nt = 1024;           // (config 4: +5 % over 512, same-box)
        if (sw.has_nt) nt = sw.nt;
        if (nt < 128 || (nt > 512 && nt != 768 && nt != 1024) || nt % 64) nt = 512;
    }
    if (sw.k_nt) nt = sw.k_nt;
    if (t4) {
        // a query whose column codes leave no room for the chosen window: every column becomes the largest power of two below,
        // a window is halved (down to 512 columns), then the workgroup steps down through the instantiated sizes
        if (lds_of(nt) > POA_LDS_LIMIT && win_mask == 0xFFFFFFFFu && lds_cols > 512) {
            uint32_t w2 = 1u << 30;
            while (w2 >= lds_cols) w2 >>= 1;
            set_window(w2);
        }
        while (lds_of(nt) > POA_LDS_LIMIT && win_mask != 0xFFFFFFFFu && hg_cols > 512) set_window(hg_cols / 2);
        while (nt > 128 && lds_of(nt) > POA_LDS_LIMIT) nt = nt > 768 ? 768 : (nt > 512 ? 512 : nt - 64);
    } else
        while (nt > 128 && lds_of(nt) > POA_LDS_LIMIT) nt /= 2;
    poa_shape s;
    s.kernel = t5 ? POA_K_T5 : (t4 ? POA_K_T4 : POA_K_LDS);
    s.def_pen = t4 && in.default_penalties && !sw.k_generic;
    s.lds_cols = lds_cols;
    s.nt = s.fam_nt = nt;
    s.hg_cols = s.fam_cols = hg_cols;
    s.win_mask = win_mask;
    s.lds = s.fam_lds = lds_of(nt);
    // k_poa_dp_t6 (vga_poa_t6.hpp): one wave per problem, the row in registers -- launches of narrow bands in chunk-pool
    // mode with the fused traceback; what does not fit its window comes back with POA_ST_RETRY and runs in k_poa_dp_t5.
    // VGA_POA_KERNEL=t5 keeps both specialised kernels out
    const bool special = t5 && in.arena && in.fused && !in.general;
    const bool t6 = special && !in.giant && !sw.k_t5 && (sw.k_t6 || (in.mean_w <= 800.0 && in.max_w <= 1000.0));
    // k_poa_dp_t7 (vga_poa_t7.hpp): t6's eight-columns-per-lane row for bands that need several waves.  The launch of a call's
    // longest problems runs it (1 024 threads: 8 192 columns per step, every column in LDS): their rows are a serial chain
    // on a CU of their own, and a t7 row takes 4.9-5.9 us where a t5 row of the same 6 000-column band takes 7.6 (config 4:
    // 10 900 -> 13 600-13 850 reads/s).  On ordinary launches it issues as many instructions per cell as t5 and loses to the
    // problems that leave its window (config 3: 7 700 against 9 450 reads/s), so there it is opt-in (VGA_POA_KERNEL=t7)
    const bool t7 = special && !t6 && (sw.k_t7 || (in.giant && !sw.k_t5));
    if (t7) {
        int nt7 = in.giant ? 1024 : 256;
        if (sw.has_t7_nt) nt7 = sw.t7_nt;
        uint32_t w7 = 4096;
        while (w7 < lds_cols && (in.giant || (double)w7 < in.max_w * 1.6 + 64.0)) w7 <<= 1;  // (a power of two that holds the launch's widest expected row)
        if (sw.has_t7_window) w7 = sw.t7_window;
        while (poa_t5_lds_bytes(w7, lds_cols, nt7) > POA_LDS_LIMIT && w7 > 1024) w7 >>= 1;
        s.kernel = POA_K_T7;
        s.nt = nt7;
        s.hg_cols = w7; s.win_mask = w7 - 1;
        s.lds = poa_t5_lds_bytes(w7, lds_cols, nt7);
    } else if (t6) {
        s.kernel = POA_K_T6;
        s.nt = 64;
        s.lds = poa_t6_lds_bytes<8>(lds_cols);
    }
    return s;
}
