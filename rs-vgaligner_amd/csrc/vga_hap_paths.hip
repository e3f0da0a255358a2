// vga_hap_paths.hip -- the deficit store beside the phase store and the sums of its rows by (set, haplotype): k_hp_keep, k_hp_sums and
// the C entry points vga_haplotype_paths_begin / _end / _store / _rank.  vga_haplotype_paths and _lists run k_hp_sums on the tile
// frame of vga_phase.hip (hp_run there) behind the unchanged k_ph_obs and k_hc_tags.  See vga_hap_paths.hpp for the definitions.
#include "vga_hap_paths.hpp"
#include "vga_path_edit.hpp"
#include "vga_path_support.hpp"
#include "vga_phase.hpp"

#include <algorithm>

// a tile holds at most 2^24 reads (ph_tile_reads), and a read adds at most 255 to a lane's 32-bit counter
static_assert(255ull * (1ull << 24) < (1ull << 32), "a tile's reads fit the 32-bit accumulators of k_hp_sums");
static_assert(HP_SUM_BLOCK % 64u == 0 && HP_CHUNK_PATHS == HP_SUM_BLOCK && HP_LANE_PATHS == 4u, "a thread of k_hp_sums owns one path of the chunk at the end");
static_assert(HP_MAX_PATHS == PS_MAX_PATHS, "the paths of path support");

namespace {

// One wave per winner i (hp_keep_row, vga_hap_paths.hpp); the caller passes the store from kept_before on.
__global__ __launch_bounds__(64) void k_hp_keep(uint32_t n, uint32_t n_paths, uint32_t pitch, uint32_t cap, const uint32_t *__restrict__ rows,
                                                 const uint32_t *__restrict__ bases, const uint32_t *__restrict__ edges, uint8_t *__restrict__ deficits,
                                                 uint8_t *__restrict__ scored)
{
    const uint32_t i = blockIdx.x, lane = threadIdx.x;
    if (i >= n) return;
    hp_keep_row(i, lane, n_paths, pitch, cap, rows, bases, edges, deficits, scored);
}

// the four bytes of a word of a row, added to a lane's counters: the deficit to cost, one to best where it is zero
__device__ __forceinline__ void hp_add(uint32_t w, uint32_t (&cost)[HP_LANE_PATHS], uint32_t (&best)[HP_LANE_PATHS])
{
#pragma unroll
    for (uint32_t k = 0; k < HP_LANE_PATHS; k++) {
        const uint32_t d = (w >> (8u * k)) & 0xFFu;
        cost[k] += d;
        best[k] += d == 0u ? 1u : 0u;
    }
}

// One workgroup per (chunk of HP_CHUNK_PATHS paths, set s), the shape of k_hc_count with paths where that has columns.  Its waves
// split the tile's 64-read words.  Per word a wave loads the 64 tag bytes of set s and the 64 scored bytes (one line each; a lane
// behind the tile's last read takes that read and is masked out), ballots "tagged a and scored" and "tagged b and scored", and
// walks the set bits of the two masks (wave-uniform: the masks are ballots).  Per read the lanes load one 32-bit word of its row,
// four neighbouring paths each, coalesced, and add into sixteen registers.  The waves' counters are summed through LDS; thread t
// then owns path chunk + t and adds, with plain 64-bit adds, into the two entries of the table that the workgroup alone owns (the
// tiles run one after another on the stream).  The workgroups of chunk 0 count reads[2 s] and reads[2 s + 1] as well.
__global__ __launch_bounds__(HP_SUM_BLOCK) void k_hp_sums(uint32_t n, uint32_t tile_reads, uint32_t n_paths, uint32_t pitch, const uint8_t *__restrict__ tags,
                                                           const uint8_t *__restrict__ deficits, const uint8_t *__restrict__ scored,
                                                           unsigned long long *__restrict__ reads, unsigned long long *__restrict__ table)
{
    constexpr uint32_t WAVES = HP_SUM_BLOCK / 64u;
    __shared__ __attribute__((aligned(16))) uint32_t part[WAVES][4][HP_CHUNK_PATHS];  // cost a, cost b, best a, best b
    __shared__ uint32_t part_reads[WAVES][2];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t s = blockIdx.y, col = blockIdx.x * HP_CHUNK_PATHS + lane * HP_LANE_PATHS;
    const bool have = col < pitch;  // (pitch is whole words: the lane's four bytes lie inside the row)
    const uint8_t *trow = tags + (size_t)s * tile_reads;
    const uint32_t *drow = reinterpret_cast<const uint32_t *>(deficits + (have ? col : 0u));
    const uint32_t wpitch = pitch / 4u;
    uint32_t cost_a[HP_LANE_PATHS] = {0, 0, 0, 0}, cost_b[HP_LANE_PATHS] = {0, 0, 0, 0}, best_a[HP_LANE_PATHS] = {0, 0, 0, 0}, best_b[HP_LANE_PATHS] = {0, 0, 0, 0};
    uint32_t n_a = 0, n_b = 0;
    for (uint32_t base = wave * 64u; base < n; base += HP_SUM_BLOCK) {
        const uint32_t r = base + lane < n ? base + lane : n - 1u;
        const uint64_t live = __builtin_amdgcn_ballot_w64(base + lane < n);
        const uint32_t tag = trow[r], sc = scored[r];
        uint64_t is_a = __builtin_amdgcn_ballot_w64(tag == 1u && sc != 0u) & live, is_b = __builtin_amdgcn_ballot_w64(tag == 2u && sc != 0u) & live;
        n_a += (uint32_t)__builtin_popcountll(is_a);
        n_b += (uint32_t)__builtin_popcountll(is_b);
        // (no load is under a lane mask either: a lane behind the row's last word takes word 0 and owns no path at the end)
        while (is_a) {
            const uint32_t k = (uint32_t)__builtin_ctzll(is_a);
            is_a &= is_a - 1u;
            hp_add(drow[(size_t)(base + k) * wpitch], cost_a, best_a);
        }
        while (is_b) {
            const uint32_t k = (uint32_t)__builtin_ctzll(is_b);
            is_b &= is_b - 1u;
            hp_add(drow[(size_t)(base + k) * wpitch], cost_b, best_b);
        }
    }
    *reinterpret_cast<uint4 *>(&part[wave][0][lane * HP_LANE_PATHS]) = make_uint4(cost_a[0], cost_a[1], cost_a[2], cost_a[3]);
    *reinterpret_cast<uint4 *>(&part[wave][1][lane * HP_LANE_PATHS]) = make_uint4(cost_b[0], cost_b[1], cost_b[2], cost_b[3]);
    *reinterpret_cast<uint4 *>(&part[wave][2][lane * HP_LANE_PATHS]) = make_uint4(best_a[0], best_a[1], best_a[2], best_a[3]);
    *reinterpret_cast<uint4 *>(&part[wave][3][lane * HP_LANE_PATHS]) = make_uint4(best_b[0], best_b[1], best_b[2], best_b[3]);
    if (lane == 0) { part_reads[wave][0] = n_a; part_reads[wave][1] = n_b; }
    __syncthreads();
    if (blockIdx.x == 0 && tid < 2u) {
        uint32_t sum = 0;
#pragma unroll
        for (uint32_t w = 0; w < WAVES; w++) sum += part_reads[w][tid];
        reads[2u * s + tid] += sum;
    }
    const uint32_t p = blockIdx.x * HP_CHUNK_PATHS + tid;
    if (p >= n_paths) return;
    uint32_t sum[4] = {0, 0, 0, 0};
#pragma unroll
    for (uint32_t w = 0; w < WAVES; w++)
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) sum[k] += part[w][k][tid];
    ulonglong2 *ea = reinterpret_cast<ulonglong2 *>(table) + (size_t)(2u * s) * n_paths + p, *eb = ea + n_paths;
    ulonglong2 a = *ea, b = *eb;
    a.x += sum[0]; a.y += sum[2];
    b.x += sum[1]; b.y += sum[3];
    *ea = a;
    *eb = b;
}

}  // namespace

// The deficit store of a context while it is on.  It belongs to the phase store (ph_hap_paths: released with it, so with the pileup
// and the index as well) and path support drops it when it ends.
struct hp_state {
    uint32_t n_paths = 0, pitch = 0, cap = HP_CAP_DEFAULT, source = HP_FROM_SUPPORT;
    uint8_t *d_deficits = nullptr, *d_scored = nullptr;
    uint64_t cap_rows = 0, n_rows = 0, first_rows = HP_STORE_ROWS0;
    ~hp_state()
    {
        if (d_deficits) (void)hipFree(d_deficits);
        if (d_scored) (void)hipFree(d_scored);
    }
};

hp_state *hp_active(vga_ctx *ctx)
{
    ph_state *ph = ph_active(ctx);
    return ph && ps_active(ctx) ? ph_hap_paths(ph).get() : nullptr;
}

bool hp_from_edit(const hp_state *hp) { return hp->source == HP_FROM_EDIT; }

void hp_empty(hp_state *hp) { hp->n_rows = 0; }

hp_view hp_view_of(const hp_state *hp) { return hp_view{hp->n_rows, hp->n_paths, hp->pitch, hp->d_deficits, hp->d_scored}; }

int hp_store_grow(vga_ctx *ctx, const char *what, uint8_t *&d_deficits, uint8_t *&d_scored, uint64_t &cap_rows, uint64_t n_rows, uint64_t first_rows,
                  uint32_t pitch, uint64_t at)
{
    if (at <= cap_rows) return VGA_OK;
    hipStream_t st = ctx->stream;
    uint64_t cap = cap_rows ? cap_rows : std::max<uint64_t>(first_rows, 1);  // grows by doubling; what is stored moves on the context's stream
    while (cap < at) cap *= 2;
    uint8_t *grown = nullptr, *grown_scored = nullptr;
    {
        vga_alloc_urgent urgent;
        if (hipMalloc((void **)&grown, cap * pitch) != hipSuccess || hipMalloc((void **)&grown_scored, cap) != hipSuccess) {
            (void)hipGetLastError();
            if (grown) (void)hipFree(grown);
            return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_align_batch: the %s store cannot grow to %llu rows of %u bytes: %llu reads kept", what,
                                 (unsigned long long)cap, pitch, (unsigned long long)n_rows);
        }
    }
    hipError_t e = hipSuccess;
    if (n_rows) {
        e = hipMemcpyAsync(grown, d_deficits, n_rows * pitch, hipMemcpyDeviceToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(grown_scored, d_scored, n_rows, hipMemcpyDeviceToDevice, st);
    }
    if (e != hipSuccess) {
        (void)hipFree(grown);
        (void)hipFree(grown_scored);
        return vga_set_error(ctx, VGA_ERR_HIP, "vga_align_batch: moving the %s store: %s", what, hipGetErrorString(e));
    }
    if (d_deficits) vga_defer_release(d_deficits, nullptr, nullptr, 0);
    if (d_scored) vga_defer_release(d_scored, nullptr, nullptr, 0);
    if (getenv("VGA_TRACE"))
        fprintf(stderr, "[vga-trace] %s: the store grows from %llu to %llu rows\n", what, (unsigned long long)cap_rows, (unsigned long long)cap);
    d_deficits = grown;
    d_scored = grown_scored;
    cap_rows = cap;
    return VGA_OK;
}

int hp_keep_winners(vga_ctx *ctx, hp_state *hp, ps_state *ps, const uint32_t *d_rows, size_t nw)
{
    if (nw == 0) return VGA_OK;
    if (hp->n_paths != ps->n_paths)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_align_batch: the haplotype paths store was made for %u paths, path support has %u", hp->n_paths, ps->n_paths);
    if (hp_from_edit(hp) && !ps->pe)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_align_batch: the haplotype paths read the edit distance (vga_haplotype_paths_begin), which is off (vga_path_edit_begin)");
    const uint64_t at = hp->n_rows + nw;
    const int grown = hp_store_grow(ctx, "haplotype paths", hp->d_deficits, hp->d_scored, hp->cap_rows, hp->n_rows, hp->first_rows, hp->pitch, at);
    if (grown != VGA_OK) return grown;
    const bool edit = hp_from_edit(hp);
    const uint32_t *d_bases = edit ? pe_gl_bases(ps->pe.get()) : ps->d_bases.p, *d_edges = edit ? pe_gl_edges(ps->pe.get()) : ps->d_edges.p;
    const int rc = vga_launch(ctx, "k_hp_keep", nw * ((uint64_t)hp->n_paths * 8u + hp->pitch), k_hp_keep, dim3((unsigned)nw), dim3(64), nw, hp->n_paths, hp->pitch, hp->cap,
                              d_rows, d_bases, d_edges, hp->d_deficits + hp->n_rows * hp->pitch, hp->d_scored + hp->n_rows);
    if (rc != VGA_OK) return rc;
    hp->n_rows = at;
    return VGA_OK;
}

int hp_sums_tile(vga_ctx *ctx, uint32_t n, uint32_t tile_reads, uint32_t n_sets, uint32_t n_paths, uint32_t pitch, const uint8_t *d_tags, const uint8_t *d_deficits,
                 const uint8_t *d_scored, unsigned long long *d_reads, unsigned long long *d_table)
{
    const uint32_t chunks = (pitch + HP_CHUNK_PATHS - 1u) / HP_CHUNK_PATHS;
    return vga_launch(ctx, "k_hp_sums", (uint64_t)n_sets * chunks * 2u * n + (uint64_t)n * pitch, k_hp_sums, dim3(chunks, n_sets), dim3(HP_SUM_BLOCK), n, tile_reads, n_paths,
                      pitch, d_tags, d_deficits, d_scored, d_reads, d_table);
}

// ---------------------------------------------------------------------------------------- C entry points (include/vga_hip.h)
extern "C" int vga_haplotype_paths_begin(vga_ctx *ctx, uint32_t cap, uint32_t source)
{
    if (!ctx) return VGA_ERR_ARG;
    if (!ctx->index.loaded) return vga_set_error(ctx, VGA_ERR_NO_INDEX, "vga_haplotype_paths_begin: no index uploaded");
    ps_state *ps = ps_active(ctx);
    ph_state *ph = ph_active(ctx);
    if (!ps) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_begin: path support is off (vga_path_support_begin)");
    if (!ph) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_begin: the phase store is off (vga_phase_begin): the rows lie beside its reads");
    if (cap < 1u || cap > HP_CAP_MAX) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_begin: cap %u (1 .. %u)", cap, HP_CAP_MAX);
    if (source != HP_FROM_SUPPORT && source != HP_FROM_EDIT) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_begin: source %u (0 support, 1 edit)", source);
    if (source == HP_FROM_EDIT && !ps->pe)
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_begin: the edit distance is off (vga_path_edit_begin), which source edit reads");
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    vga_owned<hp_state> &slot = ph_hap_paths(ph);
    slot.reset();  // (a second begin starts over)
    if (!(slot = vga_make_owned<hp_state>())) return vga_set_error(ctx, VGA_ERR_NOMEM, "vga_haplotype_paths_begin: out of host memory");
    hp_state *hp = slot.get();
    hp->n_paths = ps->n_paths;
    hp->pitch = hp_pitch(ps->n_paths);
    hp->cap = cap;
    hp->source = source;
    if (const char *e = getenv("VGA_HAP_PATHS_STORE_ROWS")) hp->first_rows = (uint64_t)std::max(1ll, atoll(e));
    return VGA_OK;
}

extern "C" int vga_haplotype_paths_end(vga_ctx *ctx)
{
    if (!ctx) return VGA_ERR_ARG;
    ph_state *ph = ph_active(ctx);
    if (!ph) return VGA_OK;  // (gone with the phase store)
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    ph_hap_paths(ph).reset();
    return VGA_OK;
}

extern "C" int vga_haplotype_paths_store(vga_ctx *ctx, uint8_t *deficits, uint8_t *scored, uint64_t *n_reads, uint32_t *n_paths)
{
    if (!ctx) return VGA_ERR_ARG;
    hp_state *hp = hp_active(ctx);
    if (!hp) return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_store: the store is off (vga_haplotype_paths_begin)");
    if (n_reads) *n_reads = hp->n_rows;
    if (n_paths) *n_paths = hp->n_paths;
    if (hp->n_rows != ph_kept_reads(ph_active(ctx)))
        return vga_set_error(ctx, VGA_ERR_ARG, "vga_haplotype_paths_store: the store holds %llu rows and the phase store %llu reads: it was turned on behind kept reads",
                             (unsigned long long)hp->n_rows, (unsigned long long)ph_kept_reads(ph_active(ctx)));
    (void)hipSetDevice(ctx->device);
    if (hp->n_rows && deficits)
        VGA_HIP_CHECK(ctx, hipMemcpy2DAsync(deficits, hp->n_paths, hp->d_deficits, hp->pitch, hp->n_paths, hp->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    if (hp->n_rows && scored) VGA_HIP_CHECK(ctx, hipMemcpyAsync(scored, hp->d_scored, hp->n_rows, hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return VGA_OK;
}

extern "C" int vga_haplotype_paths_rank(uint32_t n_paths, const uint64_t *cost_best, uint32_t *order, uint32_t *tied)
{
    if (n_paths < 1u || n_paths > HP_MAX_PATHS || !cost_best || !order || !tied) return VGA_ERR_ARG;
    *tied = hp_rank(n_paths, cost_best, order);
    return VGA_OK;
}
