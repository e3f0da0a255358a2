// vga_align_plan.hpp -- the launch plan of one vga_align_batch call, decided without touching the GPU: the environment switches
// of the call (read once), which (read, chain) pairs become POA problems, what the subgraph kernels are told about each, the
// footprint proxy that fixes the launch order, in how many parts the subgraph store is built and which problems count as very
// long.  Plain C++: no HIP type or call, so that a host compiler builds it alone (tests/test_align_plan_cpu.py pins the rules).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/vga_hip.h"
#include "vga_sg_records.hpp"

// ----------------------------------------------------------------------------------------------------------------- switches
// The environment switches of vga_align_batch (diagnostics and tests).  Read once at the start of a call -- per call, not per
// process: the GPU tests change them between calls on one context.
struct align_switches {
    bool sg_host = false;  // VGA_SUBGRAPH=host: the host-thread walk (vga_subgraph_host.hip) instead of k_sg_mark / k_sg_emit
    // a problem is very long from this many rows -- config 3's longest problems have 21 000-22 000 rows and stay in the ordinary
    // launches; config 4's bubble-rich problems of 24 000-38 000 rows, whose band is as wide as the query on every row, do not
    uint32_t giant_rows = 24000u;  // VGA_GIANT_ROWS
    // ... and so do problems with fewer rows whose band will be as wide as the query (a subgraph several times longer than the
    // read: the band spans what separates the path from the diagonal `qlen - remain`): in an ordinary launch every row of
    // theirs is wider than the LDS window and takes the HBM detour -- 24-27 us per row, 0.83-0.99 s for 34 000-37 000 rows on
    // config 4, as long as the 107 000-row problem takes in the launch of the long ones.  The product rows x expected width
    // (poa_run's estimate: from the longest source-sink path) decides.
    double giant_cells = 1.5e8;  // VGA_GIANT_CELLS
    bool has_sg_split = false;   // VGA_SG_SPLIT: the number of problems in the store's first part (0 or less: one part)
    long sg_split = 0;
    bool trace = false;          // VGA_TRACE set and not 0: the line about the parts of the store
};

static inline align_switches align_read_switches()
{
    align_switches s;
    if (const char *e = getenv("VGA_SUBGRAPH")) s.sg_host = strstr(e, "host") != nullptr;
    if (const char *e = getenv("VGA_GIANT_ROWS")) s.giant_rows = (uint32_t)atol(e);
    if (const char *e = getenv("VGA_GIANT_CELLS")) s.giant_cells = atof(e);
    if (const char *e = getenv("VGA_SG_SPLIT")) { s.has_sg_split = true; s.sg_split = atol(e); }
    if (const char *e = getenv("VGA_TRACE")) s.trace = atoi(e) != 0;
    return s;
}

// ------------------------------------------------------------------------------------------------------- problem selection
// Which (read, chain) pairs become POA problems: per read the first min(best_n, len) chains (align.rs:43-50), placeholders
// skipped.  The problems of read r are read_prob0[r] .. read_prob0[r + 1] of the list.
static inline void align_select(const vga_map_result *m, uint32_t best_n, std::vector<uint64_t> &prob_read, std::vector<uint64_t> &prob_chain,
                                std::vector<uint64_t> &read_prob0)
{
    const uint64_t R = m->n_reads;
    prob_read.clear();
    prob_chain.clear();
    read_prob0.assign(R + 1, 0);
    for (uint64_t r = 0; r < R; r++) {
        read_prob0[r] = prob_read.size();
        const uint64_t c0 = m->chain_off[r], c1 = m->chain_off[r + 1];
        const uint64_t take = std::min<uint64_t>(best_n, c1 - c0);
        for (uint64_t c = c0; c < c0 + take; c++)
            if (!m->chain_placeholder[c]) { prob_read.push_back(r); prob_chain.push_back(c); }
    }
    read_prob0[R] = prob_read.size();
}

// ------------------------------------------------------------------------------------------------------------- per problem
struct align_prob {
    sg_desc desc;     // what k_sg_mark is told about the chain
    uint32_t lo, hi;  // smallest target_begin / largest target_end over the chain's anchors
    float west;       // the band-width term of the proxy (its floor, 650: a graph about as long as the read)
    double proxy;     // footprint ~ rows x mean band width: larger = launched earlier
    bool reverse;     // an anchor carries bit 31 in its begin or end (vga_map_params.only_forward = 0)
};

// One pass over the anchors of chain c of read r (qlen bases, k-mers of k).
static inline align_prob align_plan_problem(const vga_map_result *m, uint64_t r, uint64_t c, uint32_t qlen, uint32_t k, const align_switches &sw)
{
    align_prob o = {};
    const uint64_t a0 = m->anchor_off[r];
    const uint64_t c0 = m->chain_anchor_off[c], c1 = m->chain_anchor_off[c + 1];
    uint32_t lo = 0xFFFFFFFFu, hi = 0, pmin = 0xFFFFFFFFu, pmax = 0;
    for (uint64_t t = c0; t < c1; t++) {
        const uint64_t ai = a0 + m->chain_anchor_idx[t];
        lo = std::min(lo, m->target_begin[ai]);
        hi = std::max(hi, m->target_end[ai]);
        if ((m->target_begin[ai] | m->target_end[ai]) >> 31) o.reverse = true;
        // smallest / largest position over the anchors' begins and inclusive ends (align.rs:286-308; chain.rs:65-70)
        const uint32_t s = m->target_begin[ai], e = m->target_end[ai] - 1;
        pmin = std::min(pmin, std::min(s, e));
        pmax = std::max(pmax, std::max(s, e));
    }
    o.lo = lo;
    o.hi = hi;
    // footprint ~ rows x mean band width.  Rows: the chain's span on the linearised graph plus what the extension
    // adds for the part of the read the chain does not cover (it walks every allele, ~1.6 graph bases per read
    // base on DRB1-3123); the longest path is ~0.85 of the rows (width estimate).
    const double q_first = c1 > c0 ? (double)m->query_begin[a0 + m->chain_anchor_idx[c0]] : 0.0;
    const double q_last = c1 > c0 ? (double)m->query_begin[a0 + m->chain_anchor_idx[c1 - 1]] + (double)k : (double)qlen;
    const double uncovered = q_first + std::max(0.0, (double)qlen - q_last);
    const double rows = (double)(hi > lo ? hi - lo : 0) + 1.6 * uncovered;
    o.west = (float)(650.0 + 0.3 * std::max(0.0, 0.85 * rows - (double)qlen));
    o.proxy = rows * (double)o.west;
    // a chain whose span alone makes it a long problem goes to the front of the order whatever its width term: it must be in the
    // first part of the store, where its actual rows are known before the launch of the long problems starts -- config 4: 21
    // problems of 24 000-37 000 rows sat behind position 2 048, were launched as a second group of long problems 80 ms into
    // the call and, 1 024-thread workgroups that need a CU's 16 wave slots at once, only got their CUs when the bulk launch
    // beside them had nothing left to dispatch: they ended last, 512 ms after their launch
    if (rows >= 0.85 * (double)sw.giant_rows) o.proxy += 1e13;
    if (c1 > c0) {
        const uint64_t fa = a0 + m->chain_anchor_idx[c0], la = a0 + m->chain_anchor_idx[c1 - 1];
        o.desc = {pmin, pmax, m->query_begin[fa], m->target_begin[fa], m->query_begin[la], m->target_end[la], qlen, 0u};
    }
    return o;
}

// ------------------------------------------------------------------------------------------------------------ launch order
// Largest footprint first, ties in list order: ord[i] = the list index of the problem at launch position i.
static inline std::vector<uint32_t> align_launch_order(const std::vector<double> &proxy)
{
    std::vector<uint32_t> ord(proxy.size());
    std::iota(ord.begin(), ord.end(), 0u);
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t x, uint32_t y) { return proxy[x] > proxy[y]; });
    return ord;
}

// ... and its inverse: slot_of[q] = the launch position of list index q
static inline std::vector<uint32_t> align_slot_of(const std::vector<uint32_t> &ord)
{
    std::vector<uint32_t> slot_of(ord.size());
    for (size_t i = 0; i < ord.size(); i++) slot_of[ord[i]] = (uint32_t)i;
    return slot_of;
}

// v[i] = v[ord[i]]: a per-problem array from list order into launch order
template <typename T>
static inline void align_permute(std::vector<T> &v, const std::vector<uint32_t> &ord)
{
    std::vector<T> w(v.size());
    for (size_t i = 0; i < ord.size(); i++) w[i] = v[ord[i]];
    v.swap(w);
}

// The number of problems in the first part of the device store (the rest is built beside the first DP launches).  The first
// launch takes 2 048 problems (poa_run, arena mode); small calls are prepared in one go -- and so are calls of narrow-band
// problems (rows ~ read length: the width term stays at its floor; config 5), whose DP launches are short and whose subgraphs
// are cheap: with the second part beside the first launches on a throttled stream, those launches waited 2 x 160 ms for it in
// the command line tool (25 000 reads; the chains' path text is written on the GPU at the same time), against 13 ms for all of
// it up front.  (Mean width term -- config 5: 650-740 from chunk to chunk; config 3: 1 500-2 500; config 4: in between and above.)
static inline uint64_t align_store_split(const std::vector<float> &west, const align_switches &sw, double *mean_west = nullptr)
{
    const uint64_t n = west.size();
    uint64_t split = n > 3072 ? 2048 : n;
    double wsum = 0;
    for (uint64_t i = 0; i < n; i++) wsum += west[i];
    if (n && wsum / (double)n <= 900.0) split = n;
    if (mean_west) *mean_west = n ? wsum / (double)n : 0.0;
    if (sw.has_sg_split) split = sw.sg_split <= 0 ? n : std::min<uint64_t>(n, (uint64_t)sw.sg_split);
    return split;
}

// A very long problem, by what the subgraph kernels report (N rows, `longest` bases on the source-sink path), the query and
// the band parameters: such problems decide how long the call takes and go first, in a launch of their own (poa_run).
static inline uint8_t align_is_giant(uint32_t N, uint32_t longest, uint32_t qlen, int32_t wb, double wf, const align_switches &sw)
{
    if (N >= sw.giant_rows) return 1;
    const double ql = (double)qlen;
    const double w = wb < 0 ? ql : (double)wb + (double)(uint64_t)(wf * ql);
    const double ew = std::min(ql + 1.0, 2.0 * w + 431.0 + 0.3 * std::abs((double)longest - ql));
    return (double)N * ew >= sw.giant_cells ? 1 : 0;
}
