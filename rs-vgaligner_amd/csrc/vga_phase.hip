// vga_phase.hip -- the read-backed linkage of heterozygous sites and the reads' haplotype tags: k_ph_keep, k_ph_obs, k_ph_link,
// k_ph_tag, k_ph_tag_scan and the C entry points vga_phase_begin / _read / _reset / _end / _links / _links_lists / _chain / _tags /
// _tags_lists; and what the tagged reads of each haplotype show at the calls: k_hc_tags, k_hc_cols, k_hc_count and vga_haplotype_counts /
// _counts_lists / _jobs / _call; and which sets the reads tagged in two of them hold together: k_sj_bits, k_sj_pairs and
// vga_phase_set_links / _set_links_lists / vga_phase_join.  See vga_phase.hpp, vga_hapcall.hpp and vga_phase_join.hpp for the shape.
// Links, tags, counts and set links run on one ph_frame; so do the sums of the haplotype paths (hp_run, vga_haplotype_paths / _lists:
// k_hp_sums of vga_hap_paths.hip behind k_ph_obs and k_hc_tags; vga_hap_paths.hpp).
//
// Meaning (include/vga_hip.h): a stored read observes at a site the base's own letter where a run of matches covers it, the
// read's letter where a sparse word names a mismatch, D where one names a deleted base, and nothing where it consumes the base
// not at all.  Per (site, read) three bits are ORed together (saw x, saw y, saw anything else), so a read that consumes a base
// twice gives the same answer in any order; obs = 0 for x alone, 1 for y alone, 2 for anything else consumed.  link[h][d - 1][2 a +
// b] counts the reads with obs a at site h and b at site h + d.  ORs and sums of integers: the tables are exact and repeatable.
#include "vga_phase.hpp"
#include "vga_hapcall.hpp"
#include "vga_phase_join.hpp"
#include "vga_hap_paths.hpp"
#include "vga_pair_tile.hpp"
#include "vga_pileup.hpp"

// the store keeps k_pu_events' words as they are
static_assert(PH_COL_OTHER == PU_COL_N && PH_COL_DEL == PU_COL_DEL && PH_COL_INS == PU_COL_INS && PH_COLS == PU_COLS && PH_MAX_SEQ == PU_MAX_SEQ,
              "the pileup's sparse columns and positions");
// a column of a sparse word is a bit of a byte of k_hc_cols and a counter of a row
static_assert(HC_COLS == PH_COLS && HC_COL_DEL == PH_COL_DEL && HC_COL_INS == PH_COL_INS && HC_ROW == 2u + 2u * HC_COLS && HC_MAX_CALLS == PH_MAX_SITES,
              "the columns of the haplotype counts");
// k_sj_pairs stages a chunk of both ranges with whole rounds of its threads, and a thread owns whole squares of the pair frame
static_assert(PJ_TILE % 16u == 0 && (PJ_CHUNK_ROWS * PJ_TILE) % PAIR_TILE_THREADS == 0 && PJ_CHUNK_ROWS % 2u == 0 && PJ_BITS_SETS == 64u,
              "the tile of the set links");

namespace {

// One wave per winner: its pileup list (device buffer, or the host-built lists for record flags 3) goes to dst[wi] of the store.
// The host has scanned the staged records: dst[wi] + n_a + n_b lies inside the store.
__global__ __launch_bounds__(64) void k_ph_keep(uint32_t n, const oplist_rec *__restrict__ recs, const uint32_t *__restrict__ lists,
                                                 const uint32_t *__restrict__ host_lists, const uint32_t *__restrict__ dst, uint32_t *__restrict__ store)
{
    const uint32_t wi = blockIdx.x;
    if (wi >= n) return;
    const oplist_rec rc = recs[wi];
    const uint32_t *src = ((rc.flags & 3u) == 3u ? host_lists : lists) + rc.off;
    uint32_t *out = store + dst[wi];
    const uint32_t words = rc.n_a + rc.n_b;
    for (uint32_t i = threadIdx.x; i < words; i += 64) out[i] = src[i];
}

// the first site at or behind position p (n_sites when there is none): pos ascends strictly
__device__ __forceinline__ uint32_t ph_lower(const uint32_t *__restrict__ pos, uint32_t n_sites, uint32_t p)
{
    uint32_t lo = 0, hi = n_sites;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pos[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// sets `bits` of (site h, read r of the tile): a byte per pair, site-major, four reads to a 32-bit word
__device__ __forceinline__ void ph_set(uint32_t *__restrict__ obs, uint32_t tile_reads, uint32_t h, uint32_t r, uint32_t bits)
{
    const size_t at = (size_t)h * tile_reads + r;
    atomicOr(obs + (at >> 2), bits << (8u * (uint32_t)(at & 3u)));
}

// One wave per stored read of the tile.  The lanes stride over the sparse words (the site at the word's position, if any, sees
// the word's allele; an insertion word is no observation) and over the pairs of run events (every site in [start, end) sees the
// base's own letter).  A word's position only ever enters the search over the sites: no index is taken from it.
__global__ __launch_bounds__(64) void k_ph_obs(uint32_t n, const ph_rec *__restrict__ recs, const uint32_t *__restrict__ words, uint32_t n_sites,
                                                const uint32_t *__restrict__ pos, const uint8_t *__restrict__ sx, const uint8_t *__restrict__ sy,
                                                const uint8_t *__restrict__ ref, uint32_t tile_reads, uint32_t *__restrict__ obs)
{
    const uint32_t ri = blockIdx.x;
    if (ri >= n) return;
    const uint32_t lane = threadIdx.x;
    const ph_rec rc = recs[ri];
    const uint32_t *ev = words + rc.off, *sp = ev + rc.n_runs;
    for (uint32_t i = lane; i < rc.n_sparse; i += 64) {
        const uint32_t w = sp[i], p = w >> 3, col = w & 7u;
        if (col >= PH_COL_INS) continue;
        const uint32_t h = ph_lower(pos, n_sites, p);
        if (h >= n_sites || pos[h] != p) continue;
        const uint32_t a = col < 4u ? col : col == PH_COL_DEL ? PH_ALLELE_DEL : 0xFFu;
        ph_set(obs, tile_reads, h, ri, a == sx[h] ? PH_SAW_X : a == sy[h] ? PH_SAW_Y : PH_SAW_OTHER);
    }
    for (uint32_t i = lane; i < rc.n_runs / 2u; i += 64) {
        const uint32_t start = ev[2u * i] >> 1, end = ev[2u * i + 1u] >> 1;
        for (uint32_t h = ph_lower(pos, n_sites, start); h < n_sites && pos[h] < end; h++) {
            const uint32_t a = ref[h] < 4u ? ref[h] : 0xFFu;
            ph_set(obs, tile_reads, h, ri, a == sx[h] ? PH_SAW_X : a == sy[h] ? PH_SAW_Y : PH_SAW_OTHER);
        }
    }
}

// the observation of a byte of the tile: 0 x alone, 1 y alone, 2 anything else consumed, 3 not consumed
__device__ __forceinline__ uint32_t ph_code(uint32_t o)
{
    const uint32_t xy = o & (PH_SAW_X | PH_SAW_Y);
    return xy == PH_SAW_X ? 0u : xy == PH_SAW_Y ? 1u : o ? 2u : 3u;
}

// One workgroup per site h.  Its waves stride over the tile's reads, a read per lane: the byte of site h and those of the sites
// h + 1 .. h + PH_WINDOW (each row read coalesced), the four combinations per distance counted with ballots and popcounts into
// wave-uniform counters, the waves' counters summed through LDS.  The workgroup owns link[h] and site_reads[h] and the tiles run
// one after another on the stream: plain loads and stores add the tile's sums.
__global__ __launch_bounds__(PH_LINK_BLOCK) void k_ph_link(uint32_t n_sites, uint32_t tile_reads, uint32_t n, const uint8_t *__restrict__ obs,
                                                            uint32_t *__restrict__ links, uint32_t *__restrict__ site_reads)
{
    __shared__ uint32_t part[PH_LINK_BLOCK / 64u][PH_LINK_ROW + PH_SITE_COLS];
    const uint32_t h = blockIdx.x;
    if (h >= n_sites) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t nd = n_sites - 1u - h < PH_WINDOW ? n_sites - 1u - h : PH_WINDOW;
    const uint8_t *row = obs + (size_t)h * tile_reads;
    // Two passes over the reads, four distances each: the counters of all eight beside the ballots do not fit the scalar
    // registers.  No load is under a lane mask: a lane behind the tile's last read takes that read and is masked out of site h's
    // ballots, and a distance behind the last site is skipped by the whole workgroup (its byte reads "not consumed").
#pragma unroll 1
    for (uint32_t half = 0; half < 2u; half++) {
        uint32_t cnt[PH_LINK_ROW / 2u], seen[PH_SITE_COLS];
#pragma unroll
        for (uint32_t k = 0; k < PH_LINK_ROW / 2u; k++) cnt[k] = 0;
#pragma unroll
        for (uint32_t k = 0; k < PH_SITE_COLS; k++) seen[k] = 0;
        const uint32_t d0 = half * (PH_WINDOW / 2u) + 1u;
        for (uint32_t base = wave * 64u; base < n; base += PH_LINK_BLOCK) {
            const uint32_t r = base + lane < n ? base + lane : n - 1u;
            const uint64_t live = __builtin_amdgcn_ballot_w64(base + lane < n);
            const uint32_t a = ph_code(row[r]);
            uint32_t o[PH_WINDOW / 2u];  // (the four loads are in flight together)
#pragma unroll
            for (uint32_t d = 0; d < PH_WINDOW / 2u; d++) o[d] = d0 + d <= nd ? row[(d0 + d) * tile_reads + r] : 0u;  // (uniform)
            const uint64_t a_x = __builtin_amdgcn_ballot_w64(a == 0u) & live, a_y = __builtin_amdgcn_ballot_w64(a == 1u) & live;
            seen[0] += (uint32_t)__builtin_popcountll(a_x);
            seen[1] += (uint32_t)__builtin_popcountll(a_y);
            seen[2] += (uint32_t)__builtin_popcountll(__builtin_amdgcn_ballot_w64(a == 2u) & live);
#pragma unroll
            for (uint32_t d = 0; d < PH_WINDOW / 2u; d++) {
                const uint32_t b = ph_code(o[d]);
                const uint64_t b_x = __builtin_amdgcn_ballot_w64(b == 0u), b_y = __builtin_amdgcn_ballot_w64(b == 1u);
                uint32_t *c = cnt + d * PH_LINK_COLS;
                c[0] += (uint32_t)__builtin_popcountll(a_x & b_x);
                c[1] += (uint32_t)__builtin_popcountll(a_x & b_y);
                c[2] += (uint32_t)__builtin_popcountll(a_y & b_x);
                c[3] += (uint32_t)__builtin_popcountll(a_y & b_y);
            }
        }
        if (lane == 0) {
#pragma unroll
            for (uint32_t k = 0; k < PH_LINK_ROW / 2u; k++) part[wave][half * (PH_LINK_ROW / 2u) + k] = cnt[k];
#pragma unroll
            for (uint32_t k = 0; k < PH_SITE_COLS; k++) part[wave][PH_LINK_ROW + k] = seen[k];  // (the same in both passes)
        }
    }
    __syncthreads();
    if (tid < PH_LINK_ROW + PH_SITE_COLS) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < PH_LINK_BLOCK / 64u; w++) s += part[w][tid];
        uint32_t *out = tid < PH_LINK_ROW ? links + (size_t)h * PH_LINK_ROW + tid : site_reads + (size_t)h * PH_SITE_COLS + (tid - PH_LINK_ROW);
        *out += s;
    }
}

// The loop of one lane over the sets, behind k_ph_obs (col: the read's byte of site row 0).  The sets come in ascending ps, set s
// holding the sites order[set_start[s]] .. order[set_start[s + 1] - 1] (a word of order is site << 1 | flip); all of that is
// wave-uniform, and the 64 bytes a wave loads of one site row are one line.  A site votes where the read shows x or y alone: vote =
// obs xor flip, 0 for haplotype a.  each(s, votes_a, votes_b) per set; the two counters of a set live in registers.
template <typename Each>
__device__ __forceinline__ void ph_each_set(const uint8_t *__restrict__ col, uint32_t tile_reads, uint32_t n_sets, const uint32_t *__restrict__ set_start,
                                            const uint32_t *__restrict__ order, Each each)
{
    uint32_t k = set_start[0];
    for (uint32_t s = 0; s < n_sets; s++) {
        const uint32_t end = set_start[s + 1u];
        uint32_t va = 0, vb = 0;
#pragma unroll 4
        for (; k < end; k++) {
            const uint32_t o = order[k];
            const uint32_t v = ph_code(col[(size_t)(o >> 1) * tile_reads]) ^ (o & 1u);  // (2 and 3 stay above 1 under the flip)
            va += v == 0u ? 1u : 0u;
            vb += v == 1u ? 1u : 0u;
        }
        each(s, va, vb);
    }
}

// One lane per read of the tile (ph_each_set).  EMIT = false counts the sets with a vote into rows_of[read]; EMIT = true finds there
// the read's first row within the tile (k_ph_tag_scan) and writes its rows at run[0] + that, those below cap only.  No load is under
// a lane mask: a lane behind the tile's last read takes that read and writes nothing.
template <bool EMIT>
__global__ __launch_bounds__(PH_TAG_BLOCK) void k_ph_tag(uint32_t n, uint32_t tile_reads, uint32_t r0, const uint8_t *__restrict__ obs, uint32_t n_sets,
                                                          const uint32_t *__restrict__ set_start, const uint32_t *__restrict__ set_ps,
                                                          const uint32_t *__restrict__ order, uint32_t *__restrict__ rows_of,
                                                          const uint64_t *__restrict__ run, uint64_t cap, uint32_t *__restrict__ rows)
{
    const uint32_t i = blockIdx.x * PH_TAG_BLOCK + threadIdx.x;
    const bool live = i < n;
    const uint32_t r = live ? i : n - 1u;
    uint64_t at = 0;
    uint32_t made = 0;
    if (EMIT) at = run[0] + rows_of[r];
    ph_each_set(obs + r, tile_reads, n_sets, set_start, order, [&](uint32_t s, uint32_t va, uint32_t vb) {
        if (va + vb == 0u) return;
        if (EMIT) {
            if (live && at < cap) reinterpret_cast<uint4 *>(rows)[at] = make_uint4(r0 + r, set_ps[s], va, vb);
            at++;
        } else
            made++;
    });
    if (!EMIT && live) rows_of[i] = made;
}

// One workgroup: the exclusive scan of the tile's n row counts, in place, and the running total of the rows of all tiles so far:
// run[0] = the rows before this tile, run[1] = the rows up to its end.  The kernels of a tag call follow each other on one stream.
__global__ __launch_bounds__(PH_SCAN_BLOCK) void k_ph_tag_scan(uint32_t n, uint32_t *__restrict__ rows_of, uint64_t *__restrict__ run)
{
    __shared__ uint32_t sums[PH_SCAN_BLOCK / 64u];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    uint32_t carry = 0;
    for (uint32_t base = 0; base < n; base += PH_SCAN_BLOCK) {
        const uint32_t i = base + tid;
        const uint32_t v = i < n ? rows_of[i] : 0u;
        uint32_t s = v;
#pragma unroll
        for (uint32_t d = 1; d < 64u; d <<= 1) {
            const uint32_t t = __shfl_up(s, d, 64);
            if (lane >= d) s += t;
        }
        if (lane == 63u) sums[wave] = s;
        __syncthreads();
        uint32_t before = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < PH_SCAN_BLOCK / 64u; w++) {
            const uint32_t t = sums[w];
            before += w < wave ? t : 0u;
            all += t;
        }
        if (i < n) rows_of[i] = carry + before + s - v;
        carry += all;
        __syncthreads();
    }
    if (tid == 0) {
        const uint64_t was = run[1];
        run[0] = was;
        run[1] = was + carry;
    }
}

// ---- the haplotype counts (vga_hapcall.hpp), behind the unchanged k_ph_obs

// One lane per read of the tile (ph_each_set, as k_ph_tag), and instead of rows one byte per (set, read): 1 where the read goes with
// haplotype a (votes_a > votes_b), 2 where it goes with b, 0 on a tie or without a vote -- the rule of <out>-haplotag.tsv on the
// same tile.  No load is under a lane mask: a lane behind the tile's last read takes that read and writes nothing (its bytes are
// never counted: k_hc_count masks them out).
__global__ __launch_bounds__(HC_TAG_BLOCK) void k_hc_tags(uint32_t n, uint32_t tile_reads, const uint8_t *__restrict__ obs, uint32_t n_sets,
                                                           const uint32_t *__restrict__ set_start, const uint32_t *__restrict__ order, uint8_t *__restrict__ tags)
{
    const uint32_t i = blockIdx.x * HC_TAG_BLOCK + threadIdx.x;
    const bool live = i < n;
    const uint32_t r = live ? i : n - 1u;
    ph_each_set(obs + r, tile_reads, n_sets, set_start, order, [&](uint32_t s, uint32_t va, uint32_t vb) {
        if (live) tags[(size_t)s * tile_reads + i] = (uint8_t)(va > vb ? 1u : vb > va ? 2u : 0u);
    });
}

// One wave per stored read of the tile, the shape of k_ph_obs over the calls: bit k of the byte of (call c, read r) says that the
// read shows column k at cpos[c].  A sparse word sets its own column at the call at its position, if any -- insertion words too; a
// run sets the own letter's column (cref: 0 .. 3, 4 for anything else) at every call in [start, end).  ORed bits: a base consumed
// twice shows a column once.  A word's position only ever enters the search over the calls: no index is taken from it.
__global__ __launch_bounds__(64) void k_hc_cols(uint32_t n, const ph_rec *__restrict__ recs, const uint32_t *__restrict__ words, uint32_t n_calls,
                                                 const uint32_t *__restrict__ cpos, const uint8_t *__restrict__ cref, uint32_t tile_reads,
                                                 uint32_t *__restrict__ cols)
{
    const uint32_t ri = blockIdx.x;
    if (ri >= n) return;
    const uint32_t lane = threadIdx.x;
    const ph_rec rc = recs[ri];
    const uint32_t *ev = words + rc.off, *sp = ev + rc.n_runs;
    for (uint32_t i = lane; i < rc.n_sparse; i += 64) {
        const uint32_t w = sp[i], p = w >> 3, col = w & 7u;
        if (col >= PH_COLS) continue;
        const uint32_t c = ph_lower(cpos, n_calls, p);
        if (c >= n_calls || cpos[c] != p) continue;
        ph_set(cols, tile_reads, c, ri, 1u << col);
    }
    for (uint32_t i = lane; i < rc.n_runs / 2u; i += 64) {
        const uint32_t start = ev[2u * i] >> 1, end = ev[2u * i + 1u] >> 1;
        for (uint32_t c = ph_lower(cpos, n_calls, start); c < n_calls && cpos[c] < end; c++)
            ph_set(cols, tile_reads, c, ri, 1u << (cref[c] < PH_REF_OTHER ? cref[c] : PH_COL_OTHER));
    }
}

// One workgroup per job (call c, set s): jobs holds c, the set's index and its ps.  Its waves stride over the tile's reads, a read
// per lane: the byte of call c and the byte of set s (each row read coalesced), per column a ballot of the bit, cut with the ballots
// of "tagged a" and "tagged b" and popcounted into fourteen wave-uniform counters, the waves' counters summed through LDS.  No load
// is under a lane mask: a lane behind the tile's last read takes that read and is masked out of both tag ballots.  The workgroup
// owns row j and the tiles run one after another on the stream: plain loads and stores add the tile's sums.
__global__ __launch_bounds__(HC_COUNT_BLOCK) void k_hc_count(uint32_t n_jobs, uint32_t tile_reads, uint32_t n, const uint32_t *__restrict__ jobs,
                                                              const uint8_t *__restrict__ tags, const uint8_t *__restrict__ cols, uint32_t *__restrict__ rows)
{
    __shared__ uint32_t part[HC_COUNT_BLOCK / 64u][2u * HC_COLS];
    const uint32_t j = blockIdx.x;
    if (j >= n_jobs) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint8_t *crow = cols + (size_t)jobs[3u * j] * tile_reads, *trow = tags + (size_t)jobs[3u * j + 1u] * tile_reads;
    uint32_t cnt[2u * HC_COLS];
#pragma unroll
    for (uint32_t k = 0; k < 2u * HC_COLS; k++) cnt[k] = 0;
    for (uint32_t base = wave * 64u; base < n; base += HC_COUNT_BLOCK) {
        const uint32_t r = base + lane < n ? base + lane : n - 1u;
        const uint64_t live = __builtin_amdgcn_ballot_w64(base + lane < n);
        const uint32_t bits = crow[r], tag = trow[r];
        const uint64_t is_a = __builtin_amdgcn_ballot_w64(tag == 1u) & live, is_b = __builtin_amdgcn_ballot_w64(tag == 2u) & live;
#pragma unroll
        for (uint32_t k = 0; k < HC_COLS; k++) {
            const uint64_t shows = __builtin_amdgcn_ballot_w64((bits >> k) & 1u);
            cnt[k] += (uint32_t)__builtin_popcountll(shows & is_a);
            cnt[HC_COLS + k] += (uint32_t)__builtin_popcountll(shows & is_b);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (uint32_t k = 0; k < 2u * HC_COLS; k++) part[wave][k] = cnt[k];
    }
    __syncthreads();
    uint32_t *row = rows + (size_t)j * HC_ROW;
    if (tid < 2u)
        row[tid] = jobs[3u * j + 2u * tid];  // c and ps
    else if (tid < HC_ROW) {
        uint32_t s = 0;
#pragma unroll
        for (uint32_t w = 0; w < HC_COUNT_BLOCK / 64u; w++) s += part[w][tid - 2u];
        row[tid] += s;
    }
}

// ---- the set links (vga_phase_join.hpp), behind the unchanged k_ph_obs and k_hc_tags

// One wave per word of 64 reads and PJ_BITS_SETS sets.  Per set a ballot over the 64 tag bytes of the word (one line), "tagged a" and
// "tagged b"; lane k keeps the two words of the k-th set, and the wave stores 64 sets of a bit row at once.  Bit row 2 w is "tagged
// a" of word w for every set, row 2 w + 1 "tagged b": S words each.  No load is under a lane mask: a lane behind the tile's last read
// takes that read and is masked out of both ballots.
__global__ __launch_bounds__(64) void k_sj_bits(uint32_t n, uint32_t tile_reads, uint32_t n_sets, const uint8_t *__restrict__ tags, uint64_t *__restrict__ bits)
{
    const uint32_t w = blockIdx.x, s0 = blockIdx.y * PJ_BITS_SETS, lane = threadIdx.x;
    if (w * 64u >= n || s0 >= n_sets) return;
    const uint32_t r = w * 64u + lane < n ? w * 64u + lane : n - 1u;
    const uint64_t live = __builtin_amdgcn_ballot_w64(w * 64u + lane < n);
    const uint32_t sets = n_sets - s0 < PJ_BITS_SETS ? n_sets - s0 : PJ_BITS_SETS;
    const uint8_t *col = tags + (size_t)s0 * tile_reads + r;
    uint64_t mine_a = 0, mine_b = 0;
    for (uint32_t k = 0; k < sets; k++) {
        const uint32_t tag = col[(size_t)k * tile_reads];
        const uint64_t is_a = __builtin_amdgcn_ballot_w64(tag == 1u) & live, is_b = __builtin_amdgcn_ballot_w64(tag == 2u) & live;
        if (lane == k) { mine_a = is_a; mine_b = is_b; }
    }
    if (lane < sets) {
        bits[(size_t)(2u * w) * n_sets + s0 + lane] = mine_a;
        bits[(size_t)(2u * w + 1u) * n_sets + s0 + lane] = mine_b;
    }
}

// One workgroup per PJ_TILE x PJ_TILE tile of pairs of sets s <= t (the frame of vga_pair_tile.hpp with the bit rows in the place
// of the reads, one group of them), thread (ty, tx) owning the pairs s = s0 + ty + 16 i, t = t0 + tx + 16 j.  Per chunk of
// PJ_CHUNK_ROWS bit rows the words of the s range and of the t range are staged in LDS row-major (row, then set: the sixteen tx of
// a half wave read sixteen neighbouring 64-bit words, the two ty of it two more: no two on one bank); per pair and word four ANDs
// and popcounts into four counters in registers.  A row or a set past the end is staged as zero and counts nothing.  The workgroup
// owns its rows of the table and the tiles of reads run one after another on the stream: plain loads and stores add its sums.
__global__ __launch_bounds__(PAIR_TILE_THREADS) void k_sj_pairs(uint32_t n_rows, uint32_t n_sets, uint32_t n_side, const uint64_t *__restrict__ bits,
                                                                 uint32_t *__restrict__ table)
{
    constexpr uint32_t SUB = PJ_TILE / 16u, ROUNDS = PJ_CHUNK_ROWS * PJ_TILE / PAIR_TILE_THREADS;
    __shared__ uint64_t sh[2][PJ_CHUNK_ROWS][PJ_TILE];
    const pair_tile T = pair_tile_open<PJ_TILE>(n_rows, n_sets, n_side, n_rows);
    const uint32_t tid = threadIdx.x;
    uint32_t cnt[SUB][SUB][PJ_COLS];
#pragma unroll
    for (uint32_t i = 0; i < SUB; i++)
#pragma unroll
        for (uint32_t j = 0; j < SUB; j++)
#pragma unroll
            for (uint32_t k = 0; k < PJ_COLS; k++) cnt[i][j][k] = 0;
    for (uint32_t r0 = T.r_begin; r0 < T.r_end; r0 += PJ_CHUNK_ROWS) {
        uint64_t v[2][ROUNDS];  // (the loads of both ranges are in flight together)
#pragma unroll
        for (uint32_t side = 0; side < 2u; side++)
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot e = pair_tile_slot<PJ_TILE>(T, n_sets, k, tid, r0, side);
                const uint64_t got = bits[e.have ? (size_t)e.read * n_sets + e.path : 0];
                v[side][k] = e.have ? got : 0ull;
            }
        __syncthreads();  // (the chunk before has been counted)
#pragma unroll
        for (uint32_t side = 0; side < 2u; side++)
#pragma unroll
            for (uint32_t k = 0; k < ROUNDS; k++) {
                const pair_slot e = pair_tile_slot<PJ_TILE>(T, n_sets, k, tid, r0, side);
                sh[side][e.row][e.col] = v[side][k];
            }
        __syncthreads();
#pragma unroll 4
        for (uint32_t w = 0; w < PJ_CHUNK_ROWS; w += 2u) {
            uint64_t sa[SUB], sb[SUB], ta[SUB], tb[SUB];
#pragma unroll
            for (uint32_t i = 0; i < SUB; i++) {
                sa[i] = sh[0][w][T.ty + 16u * i];
                sb[i] = sh[0][w + 1u][T.ty + 16u * i];
                ta[i] = sh[1][w][T.tx + 16u * i];
                tb[i] = sh[1][w + 1u][T.tx + 16u * i];
            }
#pragma unroll
            for (uint32_t i = 0; i < SUB; i++)
#pragma unroll
                for (uint32_t j = 0; j < SUB; j++) {
                    cnt[i][j][0] += (uint32_t)__builtin_popcountll(sa[i] & ta[j]);
                    cnt[i][j][1] += (uint32_t)__builtin_popcountll(sa[i] & tb[j]);
                    cnt[i][j][2] += (uint32_t)__builtin_popcountll(sb[i] & ta[j]);
                    cnt[i][j][3] += (uint32_t)__builtin_popcountll(sb[i] & tb[j]);
                }
        }
    }
    if (!T.live) return;
    uint4 *rows = reinterpret_cast<uint4 *>(table);
    pair_tile_each<SUB>(T, n_sets, [&](uint32_t i, uint32_t j, uint64_t at) {
        uint4 n = rows[at];
        n.x += cnt[i][j][0]; n.y += cnt[i][j][1]; n.z += cnt[i][j][2]; n.w += cnt[i][j][3];
        rows[at] = n;
    });
}

}  // namespace

// The store of a context's index while it is on (vga_dev_index::ph: released with the index): the words on the device, the
// records on the host
struct ph_state {
    uint32_t *d_words = nullptr;
    uint64_t cap = 0, n_words = 0, first_words = PH_STORE_WORDS0;
    std::vector<ph_rec> recs;
    vga_hbuf<uint32_t> h_dst;
    vga_dbuf<uint32_t> d_dst;
    vga_owned<hp_state> hp{nullptr, nullptr};  // the deficit rows of the kept reads while the haplotype paths are on
    ~ph_state()
    {
        if (d_words) (void)hipFree(d_words);
    }
};

ph_state *ph_active(vga_ctx *ctx) { return ctx && ctx->index.loaded && ctx->index.pu ? ctx->index.ph.get() : nullptr; }

uint64_t ph_kept_reads(const ph_state *ph) { return ph->recs.size(); }

vga_owned<hp_state> &ph_hap_paths(ph_state *ph) { return ph->hp; }

int ph_keep_winners(vga_ctx *ctx, ph_state *ph, const oplist_call &lists, size_t nw)
{
    if (nw == 0) return VGA_OK;
    hipStream_t st = ctx->stream;
    VGA_HIP_CHECK(ctx, ph->h_dst.reserve(nw));
    VGA_HIP_CHECK(ctx, ph->d_dst.reserve(nw));
    uint64_t at = ph->n_words;
    for (size_t i = 0; i < nw; i++) {
        ph->h_dst.p[i] = (uint32_t)at;
        at += (uint64_t)lists.h_win.p[i].n_a + lists.h_win.p[i].n_b;
        if (at > PH_MAX_WORDS)
            return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_align_batch: the phase store would pass 2^32 - 1 words: %zu reads kept", ph->recs.size());
    }
    if (at > ph->cap) {  // grows by doubling; what is stored moves on the context's stream
        uint64_t cap = ph->cap ? ph->cap : std::max<uint64_t>(ph->first_words, 1);
        while (cap < at) cap *= 2;
        cap = std::min<uint64_t>(cap, PH_MAX_WORDS);
        uint32_t *grown = nullptr;
        {
            vga_alloc_urgent urgent;
            if (hipMalloc((void **)&grown, cap * 4) != hipSuccess) {
                (void)hipGetLastError();
                return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_align_batch: the phase store cannot grow to %llu words: %zu reads kept", (unsigned long long)cap,
                                     ph->recs.size());
            }
        }
        if (ph->n_words) {
            const hipError_t e = hipMemcpyAsync(grown, ph->d_words, ph->n_words * 4, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) {
                (void)hipFree(grown);
                return vga_set_error(ctx, VGA_ERR_HIP, "vga_align_batch: moving the phase store: %s", hipGetErrorString(e));
            }
        }
        if (ph->d_words) vga_defer_release(ph->d_words, nullptr, nullptr, 0);
        if (getenv("VGA_TRACE")) fprintf(stderr, "[vga-trace] phase: the store grows from %llu to %llu words\n", (unsigned long long)ph->cap, (unsigned long long)cap);
        ph->d_words = grown;
        ph->cap = cap;
    }
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(ph->d_dst.p, ph->h_dst.p, nw * 4, hipMemcpyHostToDevice, st));
    const int rc = vga_launch(ctx, "k_ph_keep", (at - ph->n_words) * 8, k_ph_keep, dim3((unsigned)nw), dim3(64), nw, lists.d_win.p, lists.d_lists.p, lists.d_host_lists.p,
                             ph->d_dst.p, ph->d_words);
    if (rc != VGA_OK) return rc;
    for (size_t i = 0; i < nw; i++) ph->recs.push_back(ph_rec{ph->h_dst.p[i], lists.h_win.p[i].n_a, lists.h_win.p[i].n_b});
    ph->n_words = at;
    return VGA_OK;
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_phase_begin(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_phase_begin: no index uploaded");
    if (!ctx->index.pu) return vga_set_error(ctx, VGA_ERR_ARG, "vga_phase_begin: the pileup is not counted (vga_pileup_begin): its lists are what the store keeps");
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (!ctx->index.ph && !(ctx->index.ph = vga_make_owned<ph_state>())) return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_phase_begin: out of host memory");
    ph_state *ph = ctx->index.ph.get();
    ph->n_words = 0;
    ph->recs.clear();
    if (ph->hp) hp_empty(ph->hp.get());
    if (const char *e = getenv("VGA_PHASE_STORE_WORDS")) ph->first_words = (uint64_t)std::max(1ll, atoll(e));
    return VGA_OK;
}

extern "C" int vga_phase_reset(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ph_state *ph = ph_active(ctx);
    if (!ph) return vga_set_error(ctx, VGA_ERR_ARG, "vga_phase_reset: the store is off (vga_phase_begin)");
    ph->n_words = 0;
    ph->recs.clear();
    if (ph->hp) hp_empty(ph->hp.get());
    return VGA_OK;
}

extern "C" int vga_phase_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ctx->index.ph.reset();
    return VGA_OK;
}

extern "C" int vga_phase_read(vga_ctx *ctx, uint32_t *recs, uint32_t *words, uint64_t *n_reads, uint64_t *n_words)
{
    if (!ctx) return VGA_ERR_ARG;
    ph_state *ph = ph_active(ctx);
    if (!ph) return vga_set_error(ctx, VGA_ERR_ARG, "vga_phase_read: the store is off (vga_phase_begin)");
    (void)hipSetDevice(ctx->device);
    if (recs && !ph->recs.empty()) memcpy(recs, ph->recs.data(), ph->recs.size() * sizeof(ph_rec));
    if (words && ph->n_words) {
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(words, ph->d_words, ph->n_words * 4, hipMemcpyDeviceToHost, ctx->stream));
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    }
    if (n_reads) *n_reads = ph->recs.size();
    if (n_words) *n_words = ph->n_words;
    return VGA_OK;
}

namespace {

static_assert(sizeof(ph_rec) == 12, "a record is three words in the interface");

struct ph_sites {
    uint64_t n;
    const uint32_t *pos;
    const uint8_t *x, *y, *ref;
};

// What k_ph_obs and k_hc_cols rely on, for the sites and for the calls (noun: "site" / "call"): at most 2^24 positions, their arrays there (have_all),
// ascending strictly inside the graph, the own letters 0 .. 4 where given.  more(h) checks what else position h carries, in its place.
template <typename More>
int ph_check_positions(vga_ctx *ctx, const char *who, const char *noun, uint64_t n, const uint32_t *pos, const uint8_t *own, bool have_all, uint64_t n_bases,
                       More more)
{
    if (n > PH_MAX_SITES) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu %ss, 2^24 at most", who, (unsigned long long)n, noun);
    if (n && !have_all) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with %llu %ss", who, (unsigned long long)n, noun);
    for (uint64_t h = 0; h < n; h++) {
        if (pos[h] >= n_bases)
            return vga_set_error(ctx, VGA_ERR_ARG, "%s: %s %llu at base %u, the graph has %llu", who, noun, (unsigned long long)h, pos[h], (unsigned long long)n_bases);
        if (h && pos[h] <= pos[h - 1]) return vga_set_error(ctx, VGA_ERR_ARG, "%s: %s %llu does not lie behind the one before it", who, noun, (unsigned long long)h);
        const int rc = more(h);
        if (rc != VGA_OK) return rc;
        if (own && own[h] > PH_REF_OTHER) return vga_set_error(ctx, VGA_ERR_ARG, "%s: %s %llu has own letter %u (0 .. 4)", who, noun, (unsigned long long)h, own[h]);
    }
    return VGA_OK;
}

// what the kernels rely on: sites that ascend strictly inside the graph, x < y <= D, ref <= other
int ph_check_sites(vga_ctx *ctx, const char *who, const ph_sites &s, uint64_t n_bases, bool have_outputs)
{
    return ph_check_positions(ctx, who, "site", s.n, s.pos, s.ref, s.pos && s.x && s.y && have_outputs, n_bases, [&](uint64_t h) -> int {
        if (s.x[h] < s.y[h] && s.y[h] <= PH_ALLELE_DEL) return VGA_OK;
        return vga_set_error(ctx, VGA_ERR_ARG, "%s: site %llu has alleles %u, %u (x < y <= 4)", who, (unsigned long long)h, s.x[h], s.y[h]);
    });
}

// The store's half of the checks, as ph_check_lists is the lists': the store is on, and the sites lie in its index
int ph_check_store(vga_ctx *ctx, const char *who, const ph_sites &s, bool have_outputs)
{
    if (!ph_active(ctx)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: the store is off (vga_phase_begin)", who);
    return ph_check_sites(ctx, who, s, ctx->index.seq_length, have_outputs);
}

// the own letters of n positions inside the context's index, as the store's routes take them for the sites and for the calls
std::vector<uint8_t> ph_own_letters(const vga_ctx *ctx, uint64_t n, const uint32_t *pos)
{
    std::vector<uint8_t> own(n + 1);
    for (uint64_t h = 0; h < n; h++) own[h] = ph_ref_of(ctx->index.seq_fwd[pos[h]]);
    return own;
}

// what vga_phase_links_lists and vga_phase_tags_lists check before anything is launched: the sizes, the sites, and every word of
// every record that a kernel follows
int ph_check_lists(vga_ctx *ctx, const char *who, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words,
                   const ph_sites &s, bool have_outputs)
{
    if (n_bases > PH_MAX_SEQ || n_words > PH_MAX_WORDS || n_reads > PH_MAX_WORDS)
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu bases, %llu reads, %llu words: 2^29 bases and 2^32 - 1 reads and words at most", who,
                             (unsigned long long)n_bases, (unsigned long long)n_reads, (unsigned long long)n_words);
    const int rc = ph_check_sites(ctx, who, s, n_bases, have_outputs);
    if (rc != VGA_OK) return rc;
    if ((s.n && !s.ref) || (n_reads && !recs) || (n_words && !words)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array", who);
    const ph_rec *rr = (const ph_rec *)recs;
    for (uint64_t r = 0; r < n_reads; r++) {
        const ph_rec &c = rr[r];
        if ((uint64_t)c.off + c.n_runs + c.n_sparse > n_words || (c.n_runs & 1u))
            return vga_set_error(ctx, VGA_ERR_ARG, "%s: read %llu: words %u + %u + %u of %llu, run words in pairs", who, (unsigned long long)r, c.off, c.n_runs,
                                 c.n_sparse, (unsigned long long)n_words);
        const uint32_t *ev = words + c.off, *sp = ev + c.n_runs;
        for (uint32_t i = 0; i < c.n_runs; i += 2) {
            const uint32_t a = ev[i], b = ev[i + 1];
            if ((a & 1u) || !(b & 1u) || (b >> 1) <= (a >> 1) || (b >> 1) > n_bases)
                return vga_set_error(ctx, VGA_ERR_ARG, "%s: read %llu: run words %u, %u are no start and end inside %llu bases", who, (unsigned long long)r, a, b,
                                     (unsigned long long)n_bases);
        }
        for (uint32_t i = 0; i < c.n_sparse; i++)
            if ((sp[i] >> 3) >= n_bases || (sp[i] & 7u) >= PH_COLS)
                return vga_set_error(ctx, VGA_ERR_ARG, "%s: read %llu: sparse word %u (position below %llu, column below 7)", who, (unsigned long long)r, sp[i],
                                     (unsigned long long)n_bases);
    }
    return VGA_OK;
}

// the rule of a set's name: ps[h] names the site that opens the set of h (1-based, at or before h), and that site names itself
bool ph_set_named(const uint32_t *ps, uint64_t h) { return ps[h] >= 1u && ps[h] <= h + 1u && ps[ps[h] - 1u] == ps[h]; }

// the sets as vga_phase_chain numbers them (ph_set_named), flip is 0 or 1
int ph_check_sets(vga_ctx *ctx, const char *who, uint64_t n_sites, const uint32_t *ps, const uint8_t *flip, uint64_t cap, const uint32_t *rows,
                  const uint64_t *n_rows)
{
    if (!n_rows || (cap && !rows)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null output (n_rows always, rows with cap above 0)", who);
    if (n_sites && (!ps || !flip)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with %llu sites", who, (unsigned long long)n_sites);
    for (uint64_t h = 0; h < n_sites; h++) {
        if (!ph_set_named(ps, h))
            return vga_set_error(ctx, VGA_ERR_ARG, "%s: site %llu is in set %u: a set is named by the site that opens it, 1 .. %llu here", who, (unsigned long long)h,
                                 ps[h], (unsigned long long)(h + 1u));
        if (flip[h] > 1u) return vga_set_error(ctx, VGA_ERR_ARG, "%s: site %llu has flip %u (0 or 1)", who, (unsigned long long)h, flip[h]);
    }
    return VGA_OK;
}

uint32_t ph_tile_reads(uint64_t n_reads, uint64_t n_sites)
{
    const uint64_t all = (n_reads + 63u) & ~63ull;
    uint64_t t = (PH_TILE_BYTES / n_sites) & ~63ull;
    if (const char *e = getenv("VGA_PHASE_READ_TILE")) t = ((uint64_t)std::max(1ll, atoll(e)) + 63u) & ~63ull;
    return (uint32_t)std::max<uint64_t>(64, std::min<uint64_t>(t, std::min<uint64_t>(all, 1ull << 24)));
}

// What the three calls over the stored reads share.  An entry point checks its arguments, makes the frame (from then on the context's
// timers hold this call's kernels, also when it launches none), takes the reads from_store or from_lists and runs ph_run, ph_tag_run or
// hc_run: group the sets if there are any, open the tile, each_tile behind k_ph_obs with the run's own kernels, copy back, close.
struct ph_frame {
    vga_ctx *ctx;
    vga_ctx_scope scope;
    ph_sites s;  // on the host
    const ph_rec *recs = nullptr;  // the reads: the records on the host, the words on the device
    const uint32_t *d_words = nullptr;
    uint64_t n_reads = 0;
    vga_dbuf<uint32_t> own_words;  // from_lists: what d_words points to
    std::vector<uint8_t> own_ref;  // from_store: what s.ref points to
    // H sites in S sets (group); T reads to a tile of obs_words words, the first clear_words of the whole tile zeroed per tile (open)
    uint32_t H, S = 0, T = 0;
    size_t obs_words = 0, clear_words = 0;
    std::vector<uint32_t> set_of, sets;  // group: the index of the set that a site opens; what d_sets takes
    vga_dbuf<ph_rec> d_recs;
    vga_dbuf<uint32_t> d_pos, d_tile, d_sets;  // d_tile: obs, then the rows the run asked for; d_sets: set_start (S + 1), set_ps (S), order
    vga_dbuf<uint8_t> d_bytes;                 // x, y, ref

    ph_frame(vga_ctx *c, const ph_sites &sites) : ctx(c), scope(c), s(sites), H((uint32_t)sites.n)
    {
        (void)hipSetDevice(ctx->device);
        vga_timers_reset(ctx);  // (a call that launches nothing reports no kernel)
    }

    // the reads of the context's store (checked: it is on, the sites lie in its index), the sites' own letters from the index
    void from_store(uint64_t *n_reads_out)
    {
        const ph_state *ph = ph_active(ctx);
        own_ref = ph_own_letters(ctx, s.n, s.pos);
        s.ref = own_ref.data();
        recs = ph->recs.data();
        n_reads = ph->recs.size();
        d_words = ph->d_words;
        if (n_reads_out) *n_reads_out = n_reads;
    }

    // the reads of explicit lists (checked: ph_check_lists): their words on the device, behind whatever the context's stream still runs
    int from_lists(uint64_t n, const uint32_t *list_recs, uint64_t n_words, const uint32_t *words)
    {
        if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
        VGA_HIP_CHECK_OOM(ctx, own_words.reserve((size_t)n_words + 1));
        if (n_words) VGA_HIP_CHECK(ctx, hipMemcpyAsync(own_words.p, words, (size_t)n_words * 4, hipMemcpyHostToDevice, ctx->stream));
        recs = (const ph_rec *)list_recs;
        n_reads = n;
        d_words = own_words.p;
        return VGA_OK;
    }

    // The sites by set, the sets in ascending ps (a set is named by the site that opens it: its first site), stable by site inside.
    // -> the number of sets S; set_of[h]: the index of the set that site h opens; sets, for open() to upload: set_start (S + 1 words),
    // set_ps (S) and order (H words: site << 1 | flip), as the kernels take them.
    uint32_t group(const uint32_t *ps, const uint8_t *flip)
    {
        set_of.assign(H, 0);
        sets.assign(3 * (size_t)H + 1, 0);
        for (uint32_t h = 0; h < H; h++)
            if (ps[h] == h + 1u) set_of[h] = S++;
        uint32_t *set_start = sets.data(), *set_ps = set_start + S + 1u, *order = set_ps + S;
        for (uint32_t h = 0; h < H; h++) set_start[set_of[ps[h] - 1u] + 1u]++;
        for (uint32_t k = 0; k < S; k++) set_start[k + 1u] += set_start[k];
        std::vector<uint32_t> fill(set_start, set_start + S);
        for (uint32_t h = 0; h < H; h++) {
            const uint32_t k = set_of[ps[h] - 1u];
            set_ps[k] = ps[h];
            order[fill[k]++] = h << 1 | flip[h];
        }
        return S;
    }

    // T for a tile of H rows of obs, `cleared` rows zeroed per tile as obs is and `more` rows that are not; records, sites and sets go up
    int open(uint32_t cleared = 0, uint32_t more = 0)
    {
        T = ph_tile_reads(n_reads, (uint64_t)H + cleared + more);
        obs_words = (size_t)H * T / 4u;
        clear_words = obs_words + (size_t)cleared * T / 4u;
        const size_t set_words = S ? 2 * (size_t)S + 1u + H : 0;
        VGA_HIP_CHECK_OOM(ctx, d_recs.reserve(n_reads));
        VGA_HIP_CHECK_OOM(ctx, d_pos.reserve(H));
        VGA_HIP_CHECK_OOM(ctx, d_bytes.reserve((size_t)H * 3));
        VGA_HIP_CHECK_OOM(ctx, d_tile.reserve(clear_words + (size_t)more * T / 4u));
        VGA_HIP_CHECK_OOM(ctx, d_sets.reserve(set_words));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_recs.p, recs, n_reads * sizeof(ph_rec), hipMemcpyHostToDevice, ctx->stream));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_pos.p, s.pos, (size_t)H * 4, hipMemcpyHostToDevice, ctx->stream));
        const uint8_t *const bytes[3] = {s.x, s.y, s.ref};
        for (size_t k = 0; k < 3; k++) VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_bytes.p + k * H, bytes[k], H, hipMemcpyHostToDevice, ctx->stream));
        if (set_words) VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_sets.p, sets.data(), set_words * 4, hipMemcpyHostToDevice, ctx->stream));
        return VGA_OK;
    }

    // per tile of reads: the tile cleared, k_ph_obs, then per_tile(r0, n) for the n reads from r0
    template <typename F>
    int each_tile(F per_tile)
    {
        for (uint64_t r0 = 0; r0 < n_reads; r0 += T) {
            const uint32_t n = (uint32_t)std::min<uint64_t>(T, n_reads - r0);
            VGA_HIP_CHECK(ctx, hipMemsetAsync(d_tile.p, 0, clear_words * 4, ctx->stream));
            int rc = vga_launch(ctx, "k_ph_obs", 0, k_ph_obs, dim3(n), dim3(64), n, d_recs.p + r0, d_words, H, d_pos.p, d_bytes.p, d_bytes.p + H, d_bytes.p + 2 * (size_t)H,
                               T, d_tile.p);
            if (rc == VGA_OK) rc = per_tile(r0, n);
            if (rc != VGA_OK) return rc;
        }
        return VGA_OK;
    }

    // behind the run's copies back: everything has arrived, and the timers hold the call's kernels
    int close()
    {
        VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        vga_timers_collect(ctx);
        return VGA_OK;
    }
};

// k_ph_link behind k_ph_obs over the frame's reads, tile by tile, and the two tables back to the host.  The caller checked everything.
int ph_run(ph_frame &f, uint32_t *links, uint32_t *site_reads)
{
    vga_ctx *ctx = f.ctx;
    const uint32_t H = f.H;
    if (H == 0) return VGA_OK;
    if (f.n_reads == 0) {
        memset(links, 0, (size_t)H * PH_LINK_ROW * 4);
        memset(site_reads, 0, (size_t)H * PH_SITE_COLS * 4);
        return VGA_OK;
    }
    vga_dbuf<uint32_t> d_out;  // links, then site_reads
    const size_t out_words = (size_t)H * (PH_LINK_ROW + PH_SITE_COLS);
    VGA_HIP_CHECK_OOM(ctx, d_out.reserve(out_words));
    uint32_t *d_links = d_out.p, *d_sr = d_out.p + (size_t)H * PH_LINK_ROW;
    int rc = f.open();
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_out.p, 0, out_words * 4, ctx->stream));
    rc = f.each_tile([&](uint64_t, uint32_t n) {
        return vga_launch(ctx, "k_ph_link", (uint64_t)H * n, k_ph_link, dim3(H), dim3(PH_LINK_BLOCK), H, f.T, n, (const uint8_t *)f.d_tile.p, d_links, d_sr);
    });
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(links, d_links, (size_t)H * PH_LINK_ROW * 4, hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(site_reads, d_sr, (size_t)H * PH_SITE_COLS * 4, hipMemcpyDeviceToHost, ctx->stream));
    return f.close();
}

// k_ph_tag (count), k_ph_tag_scan and k_ph_tag (emit) behind k_ph_obs over the frame's reads, tile by tile: the rows of all tiles
// land in one array in (read, ps) order, the first `cap` of them, and the total in *n_rows.  Everything was checked by the caller.
int ph_tag_run(ph_frame &f, const uint32_t *ps, const uint8_t *flip, uint64_t cap, uint32_t *rows, uint64_t *n_rows)
{
    vga_ctx *ctx = f.ctx;
    hipStream_t st = ctx->stream;
    *n_rows = 0;
    if (f.H == 0 || f.n_reads == 0) return VGA_OK;
    const uint32_t H = f.H, S = f.group(ps, flip);
    const uint64_t room = std::min<uint64_t>(cap, f.n_reads * (uint64_t)S);  // (no more rows than (read, set) pairs can ever be written)
    vga_dbuf<uint32_t> d_rows_of, d_rows;
    vga_dbuf<uint64_t> d_run;
    int rc = f.open();
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK_OOM(ctx, d_rows_of.reserve(f.T));
    VGA_HIP_CHECK_OOM(ctx, d_rows.reserve((size_t)room * PH_TAG_COLS + PH_TAG_COLS));
    VGA_HIP_CHECK_OOM(ctx, d_run.reserve(2));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_run.p, 0, 16, st));
    const uint32_t *d_sets = f.d_sets.p;  // set_start, set_ps, order
    const auto tag = [&](auto kernel, uint64_t r0, uint32_t n) {
        return vga_launch(ctx, "k_ph_tag", (uint64_t)H * n, kernel, dim3((n + PH_TAG_BLOCK - 1u) / PH_TAG_BLOCK), dim3(PH_TAG_BLOCK), n, f.T, r0, (const uint8_t *)f.d_tile.p,
                         S, d_sets, d_sets + S + 1u, d_sets + 2 * (size_t)S + 1u, d_rows_of.p, d_run.p, room, d_rows.p);
    };
    rc = f.each_tile([&](uint64_t r0, uint32_t n) {
        int rc = tag(k_ph_tag<false>, r0, n);
        if (rc == VGA_OK) rc = vga_launch(ctx, "k_ph_tag_scan", (uint64_t)n * 8, k_ph_tag_scan, dim3(1), dim3(PH_SCAN_BLOCK), n, d_rows_of.p, d_run.p);
        if (rc == VGA_OK) rc = tag(k_ph_tag<true>, r0, n);
        return rc;
    });
    if (rc != VGA_OK) return rc;
    uint64_t run[2] = {0, 0};
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(run, d_run.p, 16, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    const uint64_t written = std::min<uint64_t>(run[1], room);
    if (written) VGA_HIP_CHECK(ctx, hipMemcpyAsync(rows, d_rows.p, (size_t)written * PH_TAG_COLS * 4, hipMemcpyDeviceToHost, st));
    rc = f.close();
    if (rc == VGA_OK) *n_rows = run[1];
    return rc;
}

struct hc_calls {
    uint64_t n;
    const uint32_t *cpos;
    const uint8_t *cref;
};

// what k_hc_cols relies on: calls that ascend strictly inside the graph, own letters 0 .. 4
int hc_check_calls(vga_ctx *ctx, const char *who, const hc_calls &c, uint64_t n_bases)
{
    return ph_check_positions(ctx, who, "call", c.n, c.cpos, c.cref, c.cpos != nullptr, n_bases, [](uint64_t) { return VGA_OK; });
}

// The jobs (hc_jobs), then per tile of reads k_hc_tags, k_hc_cols and k_hc_count behind k_ph_obs over the frame's reads: *n_rows =
// J always; the J rows when cap has room for them, nothing launched otherwise.  Everything was checked by the caller.
int hc_run(ph_frame &f, const uint32_t *ps, const uint8_t *flip, const hc_calls &c, uint64_t cap, uint32_t *rows, uint64_t *n_rows)
{
    vga_ctx *ctx = f.ctx;
    hipStream_t st = ctx->stream;
    const ph_sites &s = f.s;
    if (s.n == 0 || c.n == 0 || f.n_reads == 0) {
        *n_rows = 0;
        return VGA_OK;
    }
    const uint64_t J = hc_jobs(c.n, c.cpos, s.n, s.pos, ps, 0, nullptr);
    if (J > HC_MAX_JOBS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "vga_haplotype_counts: %llu jobs, 2^24 at most", (unsigned long long)J);
    *n_rows = J;
    if (cap < J || J == 0) return VGA_OK;
    const uint32_t H = f.H, C = (uint32_t)c.n, S = f.group(ps, flip);
    std::vector<uint32_t> jobs(3 * (size_t)J);
    hc_jobs(c.n, c.cpos, s.n, s.pos, ps, J, jobs.data());
    for (uint64_t j = J; j-- > 0;) {  // (c, ps) pairs become c, set index, ps, from the back: in place
        const uint32_t cj = jobs[2 * j], pj = jobs[2 * j + 1];
        jobs[3 * j] = cj;
        jobs[3 * j + 1] = f.set_of[pj - 1u];
        jobs[3 * j + 2] = pj;
    }
    vga_dbuf<uint32_t> d_calls, d_rows;  // d_calls: cpos, the bytes of cref in whole words, then the jobs
    VGA_HIP_CHECK_OOM(ctx, d_calls.reserve(C + (C + 3u) / 4u + 3 * (size_t)J));
    VGA_HIP_CHECK_OOM(ctx, d_rows.reserve((size_t)J * HC_ROW));
    uint32_t *d_cpos = d_calls.p, *d_jobs = d_cpos + C + (C + 3u) / 4u;
    uint8_t *d_cref = (uint8_t *)(d_cpos + C);
    int rc = f.open(C, S);  // the tile: obs, cols, tags (every tag byte that is counted is written)
    if (rc != VGA_OK) return rc;
    uint32_t *d_cols = f.d_tile.p + f.obs_words;
    uint8_t *d_tags = (uint8_t *)(f.d_tile.p + f.clear_words);
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_jobs, jobs.data(), 3 * (size_t)J * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_cpos, c.cpos, (size_t)C * 4, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_cref, c.cref, C, hipMemcpyHostToDevice, st));
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_rows.p, 0, (size_t)J * HC_ROW * 4, st));
    rc = f.each_tile([&](uint64_t r0, uint32_t n) {
        int rc = vga_launch(ctx, "k_hc_tags", (uint64_t)(H + S) * n, k_hc_tags, dim3((n + HC_TAG_BLOCK - 1u) / HC_TAG_BLOCK), dim3(HC_TAG_BLOCK), n, f.T, (const uint8_t *)f.d_tile.p, S,
                           f.d_sets.p, f.d_sets.p + 2 * (size_t)S + 1u, d_tags);
        if (rc == VGA_OK) rc = vga_launch(ctx, "k_hc_cols", 0, k_hc_cols, dim3(n), dim3(64), n, f.d_recs.p + r0, f.d_words, C, d_cpos, d_cref, f.T, d_cols);
        if (rc == VGA_OK) rc = vga_launch(ctx, "k_hc_count", 2 * J * n, k_hc_count, dim3((uint32_t)J), dim3(HC_COUNT_BLOCK), J, f.T, n, d_jobs, d_tags, (const uint8_t *)d_cols, d_rows.p);
        return rc;
    });
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(rows, d_rows.p, (size_t)J * HC_ROW * 4, hipMemcpyDeviceToHost, st));
    return f.close();
}

// the sets of a checked ps: the sites that open one
uint64_t sj_count_sets(uint64_t n_sites, const uint32_t *ps)
{
    uint64_t sets = 0;
    for (uint64_t h = 0; h < n_sites; h++) sets += ps[h] == h + 1u ? 1u : 0u;
    return sets;
}

// The sets of the set links: somewhere for their number, and for the table when it has room; everything ph_check_sets asks of ps
// and flip; PJ_MAX_SETS sets at most.  Before the frame is made: a refusal uploads and launches nothing.
int sj_check_sets(vga_ctx *ctx, const char *who, uint64_t n_sites, const uint32_t *ps, const uint8_t *flip, uint64_t cap_rows, const uint32_t *table,
                  const uint64_t *n_sets)
{
    if (!n_sets || (cap_rows && !table)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null output (n_sets always, table with cap_rows above 0)", who);
    const int rc = ph_check_sets(ctx, who, n_sites, ps, flip, cap_rows, table, n_sets);
    if (rc != VGA_OK) return rc;
    const uint64_t sets = sj_count_sets(n_sites, ps);
    if (sets > PJ_MAX_SETS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu phase sets, %u at most", who, (unsigned long long)sets, PJ_MAX_SETS);
    return VGA_OK;
}

// Per tile of reads k_hc_tags, k_sj_bits and k_sj_pairs behind k_ph_obs over the frame's reads; the table stays on the device across
// the tiles and comes back once.  *n_sets = S always (0 without a site or a read); the S (S + 1) / 2 rows when cap_rows has room for
// them, nothing launched otherwise.  Everything was checked by the caller (sj_check_sets).
int sj_run(ph_frame &f, const uint32_t *ps, const uint8_t *flip, uint64_t cap_rows, uint32_t *table, uint64_t *n_sets)
{
    vga_ctx *ctx = f.ctx;
    hipStream_t st = ctx->stream;
    const uint64_t sets = f.n_reads ? sj_count_sets(f.s.n, ps) : 0;
    *n_sets = sets;
    const uint64_t n_pairs = vga_pair_count(sets);
    if (sets == 0 || cap_rows < n_pairs) return VGA_OK;
    const uint32_t H = f.H, S = f.group(ps, flip), side = (S + PJ_TILE - 1u) / PJ_TILE;
    vga_dbuf<uint32_t> d_table;
    int rc = pair_exact_alloc(ctx, d_table, (size_t)n_pairs * PJ_COLS);
    if (rc == VGA_OK) rc = f.open(0, S + (S + 3u) / 4u);  // the tile: obs, tags, and two bits per tag byte
    if (rc != VGA_OK) return rc;
    uint8_t *d_tags = (uint8_t *)(f.d_tile.p + f.clear_words);
    uint64_t *d_bits = (uint64_t *)(d_tags + (size_t)S * f.T);
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_table.p, 0, (size_t)n_pairs * PJ_COLS * 4, st));
    rc = f.each_tile([&](uint64_t, uint32_t n) {
        const uint32_t words = (n + 63u) / 64u;
        int rc = vga_launch(ctx, "k_hc_tags", (uint64_t)(H + S) * n, k_hc_tags, dim3((n + HC_TAG_BLOCK - 1u) / HC_TAG_BLOCK), dim3(HC_TAG_BLOCK), n, f.T, (const uint8_t *)f.d_tile.p, S,
                           f.d_sets.p, f.d_sets.p + 2 * (size_t)S + 1u, d_tags);
        if (rc == VGA_OK)
            rc = vga_launch(ctx, "k_sj_bits", (uint64_t)S * n + (uint64_t)S * words * 16u, k_sj_bits, dim3(words, (S + PJ_BITS_SETS - 1u) / PJ_BITS_SETS), dim3(64), n, f.T, S,
                            (const uint8_t *)d_tags, d_bits);
        if (rc == VGA_OK)
            rc = vga_launch(ctx, "k_sj_pairs", (uint64_t)side * S * words * 16u + 2 * n_pairs * PJ_COLS * 4u, k_sj_pairs, dim3((uint32_t)vga_pair_count(side)), dim3(PAIR_TILE_THREADS),
                            2u * words, S, side, (const uint64_t *)d_bits, d_table.p);
        return rc;
    });
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(table, d_table.p, (size_t)n_pairs * PJ_COLS * 4, hipMemcpyDeviceToHost, st));
    return f.close();
}

// The sets of the haplotype paths: somewhere for their number, and for reads and table when they have room; everything ph_check_sets
// asks of ps and flip; HP_MAX_SETS sets and HP_MAX_ENTRIES table entries at most (refused with the counts, *n_sets written).  Before
// the frame is made: a refusal uploads and launches nothing.
int hp_check_sets(vga_ctx *ctx, const char *who, uint64_t n_sites, const uint32_t *ps, const uint8_t *flip, uint32_t n_paths, uint64_t cap_groups,
                  const uint64_t *reads, const uint64_t *table, uint64_t *n_sets)
{
    if (!n_sets || (cap_groups && (!reads || !table))) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null output (n_sets always, reads and table with cap_groups above 0)", who);
    const int rc = ph_check_sets(ctx, who, n_sites, ps, flip, 0, nullptr, n_sets);
    if (rc != VGA_OK) return rc;
    const uint64_t sets = sj_count_sets(n_sites, ps);
    if (sets > HP_MAX_SETS || 2u * sets * n_paths > HP_MAX_ENTRIES) {
        *n_sets = sets;
        if (sets > HP_MAX_SETS) return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu phase sets, %u at most", who, (unsigned long long)sets, HP_MAX_SETS);
        return vga_set_error(ctx, VGA_ERR_UNSUPPORTED, "%s: %llu phase sets and %u paths are %llu table entries, %llu at most", who, (unsigned long long)sets, n_paths,
                             (unsigned long long)(2u * sets * n_paths), (unsigned long long)HP_MAX_ENTRIES);
    }
    return VGA_OK;
}

// Per tile of reads k_hc_tags and k_hp_sums (vga_hap_paths.hip) behind k_ph_obs over the frame's reads, whose deficit rows v holds in
// the frame's order; reads and table stay on the device across the tiles and come back once.  *n_sets = S always (0 without a site
// or a read); the 2 S groups when cap_groups has room for them, nothing launched otherwise.  Everything was checked by the caller
// (hp_check_sets, and v.n_rows is the frame's number of reads).
int hp_run(ph_frame &f, const uint32_t *ps, const uint8_t *flip, const hp_view &v, uint64_t cap_groups, uint64_t *reads, uint64_t *table, uint64_t *n_sets)
{
    vga_ctx *ctx = f.ctx;
    hipStream_t st = ctx->stream;
    const uint64_t sets = f.n_reads ? sj_count_sets(f.s.n, ps) : 0;
    *n_sets = sets;
    if (sets == 0 || cap_groups < 2u * sets) return VGA_OK;
    const uint32_t H = f.H, S = f.group(ps, flip);
    const size_t group_words = 2 * (size_t)S, table_words = group_words * v.n_paths * HP_COLS;
    vga_dbuf<unsigned long long> d_out;  // reads, then the table (2 S is even: its entries stay 16-byte aligned)
    VGA_HIP_CHECK_OOM(ctx, d_out.reserve(group_words + table_words));
    int rc = f.open(0, S);  // the tile: obs, tags (every tag byte that is counted is written)
    if (rc != VGA_OK) return rc;
    uint8_t *d_tags = (uint8_t *)(f.d_tile.p + f.clear_words);
    VGA_HIP_CHECK(ctx, hipMemsetAsync(d_out.p, 0, (group_words + table_words) * 8, st));
    rc = f.each_tile([&](uint64_t r0, uint32_t n) {
        int rc = vga_launch(ctx, "k_hc_tags", (uint64_t)(H + S) * n, k_hc_tags, dim3((n + HC_TAG_BLOCK - 1u) / HC_TAG_BLOCK), dim3(HC_TAG_BLOCK), n, f.T, (const uint8_t *)f.d_tile.p, S,
                           f.d_sets.p, f.d_sets.p + 2 * (size_t)S + 1u, d_tags);
        if (rc == VGA_OK) rc = hp_sums_tile(ctx, n, f.T, S, v.n_paths, v.pitch, d_tags, v.d_deficits + r0 * v.pitch, v.d_scored + r0, d_out.p, d_out.p + group_words);
        return rc;
    });
    if (rc != VGA_OK) return rc;
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(reads, d_out.p, group_words * 8, hipMemcpyDeviceToHost, st));
    VGA_HIP_CHECK(ctx, hipMemcpyAsync(table, d_out.p + group_words, table_words * 8, hipMemcpyDeviceToHost, st));
    return f.close();
}

}  // namespace

extern "C" int vga_phase_links(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, uint32_t *links, uint32_t *site_reads,
                               uint64_t *n_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, nullptr};
    const int rc = ph_check_store(ctx, "vga_phase_links", s, links && site_reads);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    f.from_store(n_reads);
    return ph_run(f, links, site_reads);
}

extern "C" int vga_phase_links_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words,
                                     uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint8_t *ref, uint32_t *links,
                                     uint32_t *site_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, ref};
    const int rc = ph_check_lists(ctx, "vga_phase_links_lists", n_bases, n_reads, recs, n_words, words, s, links && site_reads);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    const int up = f.from_lists(n_reads, recs, n_words, words);
    return up != VGA_OK ? up : ph_run(f, links, site_reads);
}

extern "C" int vga_phase_tags(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint32_t *ps, const uint8_t *flip,
                              uint64_t cap, uint32_t *rows, uint64_t *n_rows, uint64_t *n_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, nullptr};
    int rc = ph_check_store(ctx, "vga_phase_tags", s, true);
    if (rc == VGA_OK) rc = ph_check_sets(ctx, "vga_phase_tags", n_sites, ps, flip, cap, rows, n_rows);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    f.from_store(n_reads);
    return ph_tag_run(f, ps, flip, cap, rows, n_rows);
}

extern "C" int vga_phase_tags_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words,
                                    uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint8_t *ref, const uint32_t *ps,
                                    const uint8_t *flip, uint64_t cap, uint32_t *rows, uint64_t *n_rows)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, ref};
    int rc = ph_check_lists(ctx, "vga_phase_tags_lists", n_bases, n_reads, recs, n_words, words, s, true);
    if (rc == VGA_OK) rc = ph_check_sets(ctx, "vga_phase_tags_lists", n_sites, ps, flip, cap, rows, n_rows);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    const int up = f.from_lists(n_reads, recs, n_words, words);
    return up != VGA_OK ? up : ph_tag_run(f, ps, flip, cap, rows, n_rows);
}

extern "C" int vga_haplotype_counts(vga_ctx *ctx, uint64_t n_calls, const uint32_t *cpos, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y,
                                    const uint32_t *ps, const uint8_t *flip, uint64_t cap, uint32_t *rows, uint64_t *n_rows, uint64_t *n_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, nullptr};
    hc_calls c = {n_calls, cpos, nullptr};
    int rc = ph_check_store(ctx, "vga_haplotype_counts", s, true);
    if (rc == VGA_OK) rc = ph_check_sets(ctx, "vga_haplotype_counts", n_sites, ps, flip, cap, rows, n_rows);
    if (rc == VGA_OK) rc = hc_check_calls(ctx, "vga_haplotype_counts", c, ctx->index.seq_length);
    if (rc != VGA_OK) return rc;
    const std::vector<uint8_t> cref = ph_own_letters(ctx, n_calls, cpos);
    c.cref = cref.data();
    ph_frame f(ctx, s);
    f.from_store(n_reads);
    return hc_run(f, ps, flip, c, cap, rows, n_rows);
}

extern "C" int vga_haplotype_counts_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words,
                                          uint64_t n_calls, const uint32_t *cpos, const uint8_t *cref, uint64_t n_sites, const uint32_t *pos, const uint8_t *x,
                                          const uint8_t *y, const uint8_t *ref, const uint32_t *ps, const uint8_t *flip, uint64_t cap, uint32_t *rows,
                                          uint64_t *n_rows)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, ref};
    const hc_calls c = {n_calls, cpos, cref};
    int rc = ph_check_lists(ctx, "vga_haplotype_counts_lists", n_bases, n_reads, recs, n_words, words, s, true);
    if (rc == VGA_OK) rc = ph_check_sets(ctx, "vga_haplotype_counts_lists", n_sites, ps, flip, cap, rows, n_rows);
    if (rc == VGA_OK) rc = hc_check_calls(ctx, "vga_haplotype_counts_lists", c, n_bases);
    if (rc == VGA_OK && n_calls && !cref) rc = vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_counts_lists: null array with %llu calls", (unsigned long long)n_calls);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    const int up = f.from_lists(n_reads, recs, n_words, words);
    return up != VGA_OK ? up : hc_run(f, ps, flip, c, cap, rows, n_rows);
}

extern "C" int vga_haplotype_jobs(uint64_t n_calls, const uint32_t *cpos, uint64_t n_sites, const uint32_t *pos, const uint32_t *ps, uint64_t cap, uint32_t *jobs,
                                  uint64_t *n_jobs)
{
    if (!n_jobs || (cap && !jobs) || (n_calls && !cpos) || (n_sites && (!pos || !ps))) return VGA_ERR_ARG;
    for (uint64_t j = 1; j < n_calls; j++)
        if (cpos[j] <= cpos[j - 1]) return VGA_ERR_ARG;
    for (uint64_t h = 0; h < n_sites; h++)
        if ((h && pos[h] <= pos[h - 1]) || !ph_set_named(ps, h)) return VGA_ERR_ARG;
    *n_jobs = hc_jobs(n_calls, cpos, n_sites, pos, ps, cap, jobs);
    return VGA_OK;
}

extern "C" int vga_haplotype_call(const uint32_t *counts, char *text)
{
    if (!counts || !text) return VGA_ERR_ARG;
    hc_call_text(hc_call(counts), text);
    return VGA_OK;
}

extern "C" int vga_phase_set_links(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint32_t *ps, const uint8_t *flip,
                                   uint64_t cap_rows, uint32_t *table, uint64_t *n_sets, uint64_t *n_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, nullptr};
    int rc = ph_check_store(ctx, "vga_phase_set_links", s, true);
    if (rc == VGA_OK) rc = sj_check_sets(ctx, "vga_phase_set_links", n_sites, ps, flip, cap_rows, table, n_sets);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    f.from_store(n_reads);
    return sj_run(f, ps, flip, cap_rows, table, n_sets);
}

extern "C" int vga_phase_set_links_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words,
                                         uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint8_t *ref, const uint32_t *ps,
                                         const uint8_t *flip, uint64_t cap_rows, uint32_t *table, uint64_t *n_sets)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, ref};
    int rc = ph_check_lists(ctx, "vga_phase_set_links_lists", n_bases, n_reads, recs, n_words, words, s, true);
    if (rc == VGA_OK) rc = sj_check_sets(ctx, "vga_phase_set_links_lists", n_sites, ps, flip, cap_rows, table, n_sets);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    const int up = f.from_lists(n_reads, recs, n_words, words);
    return up != VGA_OK ? up : sj_run(f, ps, flip, cap_rows, table, n_sets);
}

extern "C" int vga_haplotype_paths(vga_ctx *ctx, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y, const uint32_t *ps, const uint8_t *flip,
                                   uint64_t cap_groups, uint64_t *reads, uint64_t *table, uint64_t *n_sets, uint64_t *n_reads)
{
    if (!ctx) return VGA_ERR_ARG;
    const ph_sites s = {n_sites, pos, x, y, nullptr};
    int rc = ph_check_store(ctx, "vga_haplotype_paths", s, true);
    if (rc != VGA_OK) return rc;
    const hp_state *hp = hp_active(ctx);
    if (!hp) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths: the deficit store is off (vga_haplotype_paths_begin)");
    const hp_view v = hp_view_of(hp);
    if (v.n_rows != ph_kept_reads(ph_active(ctx)))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths: the deficit store holds %llu rows and the phase store %llu reads: it was turned on behind kept reads",
                             (unsigned long long)v.n_rows, (unsigned long long)ph_kept_reads(ph_active(ctx)));
    rc = hp_check_sets(ctx, "vga_haplotype_paths", n_sites, ps, flip, v.n_paths, cap_groups, reads, table, n_sets);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    f.from_store(n_reads);
    return hp_run(f, ps, flip, v, cap_groups, reads, table, n_sets);
}

extern "C" int vga_haplotype_paths_lists(vga_ctx *ctx, uint64_t n_bases, uint64_t n_reads, const uint32_t *recs, uint64_t n_words, const uint32_t *words, uint32_t n_paths,
                                         const uint8_t *deficits, const uint8_t *scored, uint64_t n_sites, const uint32_t *pos, const uint8_t *x, const uint8_t *y,
                                         const uint8_t *ref, const uint32_t *ps, const uint8_t *flip, uint64_t cap_groups, uint64_t *reads, uint64_t *table,
                                         uint64_t *n_sets)
{
    if (!ctx) return VGA_ERR_ARG;
    const char *who = "vga_haplotype_paths_lists";
    const ph_sites s = {n_sites, pos, x, y, ref};
    int rc = ph_check_lists(ctx, who, n_bases, n_reads, recs, n_words, words, s, true);
    if (rc != VGA_OK) return rc;
    if (n_paths < 1u || n_paths > HP_MAX_PATHS) return vga_set_error(ctx, VGA_ERR_ARG, "%s: %u paths (1 .. %u)", who, n_paths, HP_MAX_PATHS);
    if (n_reads && (!deficits || !scored)) return vga_set_error(ctx, VGA_ERR_ARG, "%s: null array with %llu reads", who, (unsigned long long)n_reads);
    for (uint64_t r = 0; r < n_reads; r++)
        if (scored[r] > 1u) return vga_set_error(ctx, VGA_ERR_ARG, "%s: read %llu has scored %u (0 or 1)", who, (unsigned long long)r, scored[r]);
    rc = hp_check_sets(ctx, who, n_sites, ps, flip, n_paths, cap_groups, reads, table, n_sets);
    if (rc != VGA_OK) return rc;
    ph_frame f(ctx, s);
    const int up = f.from_lists(n_reads, recs, n_words, words);
    if (up != VGA_OK) return up;
    // the rows at the store's pitch, the bytes behind the last path zero
    const uint32_t pitch = hp_pitch(n_paths);
    vga_dbuf<uint8_t> d_rows;  // deficits, then scored
    VGA_HIP_CHECK_OOM(ctx, d_rows.reserve((size_t)n_reads * pitch + n_reads + 4));
    if (n_reads) {
        VGA_HIP_CHECK(ctx, hipMemsetAsync(d_rows.p, 0, (size_t)n_reads * pitch, ctx->stream));
        VGA_HIP_CHECK(ctx, hipMemcpy2DAsync(d_rows.p, pitch, deficits, n_paths, n_paths, n_reads, hipMemcpyHostToDevice, ctx->stream));
        VGA_HIP_CHECK(ctx, hipMemcpyAsync(d_rows.p + (size_t)n_reads * pitch, scored, n_reads, hipMemcpyHostToDevice, ctx->stream));
    }
    const hp_view v = {n_reads, n_paths, pitch, d_rows.p, d_rows.p + (size_t)n_reads * pitch};
    return hp_run(f, ps, flip, v, cap_groups, reads, table, n_sets);
}

extern "C" int vga_phase_join(uint64_t n_sets, const uint32_t *table, uint32_t min_reads, uint32_t *set_root, uint8_t *set_flip, uint32_t *joins, uint64_t *n_joins,
                              uint64_t *n_agree, uint64_t *n_conflict)
{
    if (min_reads < 1u || min_reads > PJ_MIN_READS_MAX || n_sets > PJ_MAX_SETS) return VGA_ERR_ARG;
    if (!n_joins || !n_agree || !n_conflict || (n_sets && (!table || !set_root || !set_flip)) || (n_sets > 1 && !joins)) return VGA_ERR_ARG;
    pj_join(n_sets, table, min_reads, set_root, set_flip, joins, n_joins, n_agree, n_conflict);
    return VGA_OK;
}

extern "C" int vga_phase_chain(uint64_t n_sites, const uint32_t *links, uint32_t min_links, uint32_t *ps, uint8_t *flip, uint8_t *link_d)
{
    if (min_links < 1u || min_links > PH_MIN_LINKS_MAX || n_sites > PH_MAX_SITES) return VGA_ERR_ARG;
    if (n_sites && (!links || !ps || !flip || !link_d)) return VGA_ERR_ARG;
    ph_chain(n_sites, links, min_links, ps, flip, link_d);
    return VGA_OK;
}
