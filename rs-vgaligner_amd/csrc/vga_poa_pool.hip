// vga_poa_pool.hip -- the traceback pool of the POA engine: the context's workspace (poa_ws: staging slots, chunk segments and
// their grower thread, state regions, the classic pool) and a call's hold on it (poa_pool: how much it may take, chunk-pool or
// classic mode, the keeper thread).  DESIGN.md section 9 has the reasons behind the orders kept here.
#include "vga_poa_pool.hpp"

#include <algorithm>

poa_ws &poa_ws_of(vga_ctx *ctx)
{
    if (!ctx->poa_ws && !(ctx->poa_ws = vga_make_owned<poa_ws>())) throw std::bad_alloc();
    poa_ws &W = *ctx->poa_ws;
    W.device = ctx->device;
    W.owner = ctx;
    return W;
}

uint64_t poa_state_size(uint32_t max_q)
{
    const uint64_t maxrow_all = (6ull * (uint64_t)((max_q + 8) & ~3u) + 15ull) & ~15ull;
    return (maxrow_all * (POA_RING_SPAN + 1) + 12ull * poa_lds_cols(max_q) + 4096ull + 65535ull) & ~65535ull;
}

// The context's share of `avail`.  Contexts that share a GPU: vga_ctx_set_pool_fraction (the driver: 1 / their number, as for
// vgaligner map --devices 0,0); VGA_POOL_FRACTION is the diagnostic override, VGA_POOL_BYTES a cap.  Returns the share (1.0: all)
static double poa_pool_share(const vga_ctx *ctx, const poa_switches &sw, uint64_t &avail)
{
    double share = 1.0;
    const double f = sw.has_pool_fraction ? sw.pool_fraction : ctx->pool_fraction;
    if (f > 0.0 && f < 1.0) { avail = (uint64_t)((double)avail * f); share = f; }
    if (sw.has_pool_bytes) avail = std::min<uint64_t>(avail, sw.pool_bytes);
    return share;
}

// State regions: one per workgroup of a launch (16 two-wave workgroups per CU at most) -- fewer, and the rest of a launch spins for
// one on CUs the holders need -- halved until they take no more than a quarter of `avail`.  cap: VGA_POA_ARENAS (0: none)
static uint64_t poa_state_regions(const vga_ctx *ctx, uint64_t n, uint64_t state_size, uint64_t avail, uint64_t cap)
{
    uint64_t ns = std::min<uint64_t>(16ull * (uint64_t)ctx->n_cu, std::max<uint64_t>(n, 64));
    if (cap) ns = std::min<uint64_t>(ns, cap);
    while (ns > 1 && ns * state_size > avail / 4) ns /= 2;
    return ns;
}

void poa_pool_prepare(vga_ctx *ctx, const poa_switches &sw, uint64_t n_reads, uint32_t max_read_len)
{
    poa_ws &W = poa_ws_of(ctx);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    // (ahead of a call this keeps 0.85 of what is free above 16 GB; poa_pool::measure, which also counts what the pool already
    // holds, reserves max(15 %, 16 GB): each keeps its own formula)
    uint64_t avail = free_b > (16ull << 30) ? (uint64_t)((double)free_b * 0.85) : free_b / 4;
    const double share = poa_pool_share(ctx, sw, avail);  // of the GPU: its memory, and the workgroups that will be resident at a time
    const uint64_t state_size = poa_state_size(max_read_len);
    // (a context that shares the GPU with others has its share of the resident workgroups, which is what the chunk pool is sized
    // for below: eight contexts that each provided for a whole GPU spent 5.3 s of a 12 s run in allocations that the driver
    // serialises and clears at 40 GB/s)
    const uint64_t ns = poa_state_regions(ctx, n_reads, state_size, avail, 0);  // (VGA_POA_ARENAS caps them in the call itself)
    if (ns * state_size > avail / 2) return;
    // the direction rows of a read of L bases against its subgraph: about 1.7 L rows of a band about 0.25 L wide plus the kept
    // value rows -- half of what the resident problems of such a call will hold (poa_run asks for the rest, from its probe)
    const double per_problem = 0.5 * (double)max_read_len * (double)max_read_len + 2.0 * (double)POA_CHUNK;
    const uint64_t resident = std::min<uint64_t>(n_reads, std::max<uint64_t>(32, (uint64_t)(6.0 * (double)ctx->n_cu * share)));
    uint64_t pool_want = (uint64_t)std::min<double>((double)resident * per_problem * 0.35, (double)avail / 4.0) & ~(POA_CHUNK - 1);
    if (pool_want < 16 * POA_CHUNK) pool_want = 0;
    W.prepare_async(ns * state_size, pool_want, (uint32_t)ctx->n_cu);
}

// what this context may take of the GPU: everything else it allocates (staging of three sub-batches, the subgraph store,
// the map workspace) keeps 15 % of what is free, at least 16 GB -- two processes sharing a GPU otherwise starve each other
int poa_pool::measure()
{
    size_t free_b = 0, total_b = 0;
    VGA_HIP_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
    uint64_t have;
    { std::lock_guard<std::mutex> lk(W.mu); have = free_b + W.pool_size; }
    have += W.classic_size;
    const uint64_t reserve = std::max<uint64_t>((uint64_t)((double)have * 0.15), 16ull << 30);
    avail = have > reserve ? have - reserve : have / 4;
    (void)poa_pool_share(ctx, sw, avail);
    return VGA_OK;
}

// Chunk-pool mode: the state regions now, the chunk segments on the grower thread (the first launch starts as soon
// as one segment is there; its workgroups all begin with empty hands).  The pool should hold what the resident
// workgroups have written so far: about six per CU, each on average two thirds through a problem of the probe's mean
// size -- a workgroup that finds the free list empty waits for chunks to come back (and gives its problem up after a
// bounded wait: the classic pass takes it).
int poa_pool::obtain_chunks(const poa_probe &pr, hipStream_t st)
{
    const uint64_t ns = poa_state_regions(ctx, n, state_size, avail, sw.has_arenas ? std::max<uint64_t>(1, sw.arenas) : 0);
    // (not scaled by the context's share of the GPU: a context whose slice holds a call's longest problems needs their whole
    // footprint whatever its share -- scaled, eight contexts on one GPU waited seconds for chunks and gave problems up)
    const uint64_t resident = std::min<uint64_t>(n, 6ull * (uint64_t)ctx->n_cu);
    // what is resident at a time: every long problem of the call (a launch of their own, one CU each: poa_feed::klass) and
    // `resident` workgroups of the others.  The probe is the head of the launch order, where the long problems stand: their
    // footprints are summed, not taken for the mean of the rest (config 4, 12 000 reads: 217 GB asked for where 75 GB do)
    const uint64_t bulk_resident = std::min<uint64_t>(n - std::min<uint64_t>(n, pr.long_all), resident);
    uint64_t want = (uint64_t)((pr.long_sum + (double)bulk_resident * pr.bulk_mean) * W.pool_scale * sw.pool_fill) + 64 * POA_CHUNK;
    want = std::max<uint64_t>(want, (uint64_t)(pr.big * W.pool_scale * 1.5));
    want = std::min<uint64_t>(want, avail > ns * state_size ? avail - ns * state_size : avail / 2);
    want = (want + POA_CHUNK - 1) & ~(POA_CHUNK - 1);
    if (ns * state_size > avail / 2 || want < 16 * POA_CHUNK) return VGA_OK;
    if (W.state_bytes < ns * state_size) {
        if (W.state) { (void)hipFree(W.state); W.state = nullptr; W.state_bytes = 0; }
        VGA_HIP_CHECK(ctx, hipMalloc((void **)&W.state, ns * state_size));
        W.state_bytes = ns * state_size;
    }
    if (W.classic && want > 0) {  // (memory the classic pool holds is memory the segments cannot have)
        size_t free_b = 0, total_b = 0;
        VGA_HIP_CHECK(ctx, hipMemGetInfo(&free_b, &total_b));
        uint64_t have;
        { std::lock_guard<std::mutex> lk(W.mu); have = W.pool_size; }
        if (have < want && free_b < want - have + (8ull << 30)) { (void)hipFree(W.classic); W.classic = nullptr; W.classic_size = 0; }
    }
    {
        std::lock_guard<std::mutex> lk(W.mu);  // (the grower may be at work already: vga_align_prepare)
        W.seg_bytes = std::min<uint64_t>(1ull << POA_SEG_LOG2, std::max<uint64_t>(want, 16 * POA_CHUNK));
        if (sw.has_pool_seg) W.seg_bytes = std::max<uint64_t>(16 * POA_CHUNK, sw.pool_seg & ~(POA_CHUNK - 1));
        W.seg_bytes = std::min<uint64_t>(W.seg_bytes, 1ull << POA_SEG_LOG2);  // (chunks are numbered segment << 12 | chunk in segment)
    }
    tr.mark("pool: state regions");
    VGA_HIP_CHECK(ctx, W.ensure_tables((uint32_t)ctx->n_cu));
    tr.mark("pool: tables");
    W.request(want);
    // The launches start when the pool holds what their resident workgroups need: on memory that was used before, the driver
    // clears a segment as it hands it out (0.1 s per 4 GiB), and launches that fill the GPU with workgroups waiting for chunks
    // leave the kernel that lists new segments no slot to run in (a 12 000-read call of config 4 that started with a sixth
    // of its pool took 19 s).  On fresh memory this waits a few milliseconds.
    const uint64_t got = W.wait_for(want);
    tr.mark("pool: segments");
    if (got < 16 * POA_CHUNK) return VGA_OK;
    const uint32_t max_chunks = (uint32_t)(POA_MAX_SEGS * (1ull << (POA_SEG_LOG2 - 20)));
    W.h_short.p[0] = 0;
    // (on the context's stream, and waited for: hipMemset runs on the null stream and may return before the device has
    // done it -- no stream of this library waits for the null stream, and on a GPU that other contexts keep full the
    // flags were cleared AFTER the first workgroups of slots 1 and 2 had taken their state regions: a second workgroup
    // took the same region, and both problems came back with wrong alignments)
    VGA_HIP_CHECK(ctx, hipMemsetAsync(W.d_slot_flag.p, 0, ns * sizeof(uint32_t), st));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
    tr.mark("pool: flags cleared");
    n_arenas = (uint32_t)ns;
    CP.head = W.d_head.p; CP.next = W.d_next_chunk.p; CP.seg_base = W.d_seg_base.p;
    CP.cps_log2 = POA_SEG_LOG2 - 20; CP.n_slots = n_arenas; CP.state_base = W.state; CP.state_size = state_size;
    CP.slot_flag = W.d_slot_flag.p; CP.stats = W.d_head.p + POA_LISTS * POA_LIST_STRIDE;
    CP.short_flag = W.h_short.p;
    if (sw.pool_check) {  // (diagnostics: poa_chunk_pool::owner)
        if (!W.d_owner.p) {
            VGA_HIP_CHECK(ctx, W.d_owner.reserve(max_chunks));
            VGA_HIP_CHECK(ctx, hipMemsetAsync(W.d_owner.p, 0, W.d_owner.cap * sizeof(uint32_t), st));
            VGA_HIP_CHECK(ctx, hipStreamSynchronize(st));
        }
        CP.owner = W.d_owner.p;
    }
    return VGA_OK;
}

// new segments' chunks join the free list (a tiny kernel on a stream of its own), and requests that found every list empty
// make the pool grow.  Called before every launch and, every millisecond, by the keeper thread below
hipError_t poa_pool::list_new_segments()
{
    std::lock_guard<std::mutex> list_lk(list_mu);
    std::vector<poa_ws::seg_t> fresh;
    {
        std::lock_guard<std::mutex> lk(W.mu);
        for (size_t k = W.segs_listed; k < W.segs.size(); k++) fresh.push_back(W.segs[k]);
    }
    for (const poa_ws::seg_t &g : fresh) {
        const uint32_t first = (uint32_t)W.segs_listed << (POA_SEG_LOG2 - 20), cnt = (uint32_t)(g.size >> 20);
        W.h_seg_base.p[W.segs_listed] = (uint64_t)g.p;
        (void)hipMemcpyAsync(W.d_seg_base.p + W.segs_listed, W.h_seg_base.p + W.segs_listed, sizeof(uint64_t), hipMemcpyHostToDevice, W.add_stream);
        poa_launch_chunks_add(W.add_stream, CP, first, cnt);
        W.segs_listed++;
        W.chunks_listed += cnt;
        if (tr.on && W.segs_listed > 1) fprintf(stderr, "[vga-trace] poa: segment %zu listed (%u chunks)\n", W.segs_listed, cnt);
    }
    hipError_t e = fresh.empty() ? hipSuccess : hipStreamSynchronize(W.add_stream);
    // requests that found the list empty: the pool is short of what the resident workgroups need -- more segments.
    // (The kernels raise a flag in pinned host memory: reading it costs no GPU work.)
    volatile uint32_t *flag = W.h_short.p;
    // one step at a time: what is raised while a step is still being allocated and listed is the shortage that step
    // answers -- without this the target runs away, +50 % every few milliseconds
    bool settled;
    { std::lock_guard<std::mutex> lk(W.mu); settled = !W.growing && W.segs_listed == W.segs.size(); }
    if (e == hipSuccess && *flag) {
        *flag = 0;
        if (settled) {
            uint64_t ps; { std::lock_guard<std::mutex> lk(W.mu); ps = std::max(W.pool_size, W.grow_target); }
            const uint64_t more = std::min<uint64_t>(ps + ps / 2 + (4ull << 30), avail);
            if (more > ps) W.request(more);
            if (tr.on) fprintf(stderr, "[vga-trace] poa: requests have found every free list empty: pool target %.1f -> %.1f GB\n", (double)ps / 1e9, (double)more / 1e9);
        }
    }
    return e;
}

// the keeper: the thread that runs this call may be held up for as long as a launch takes (a staging buffer that grows, the
// look-ahead preparation waiting for its kernel), and workgroups that wait for chunks meanwhile keep the launch from ending --
// so the pool is looked after by a thread that does nothing else
void poa_pool::start_keeper()
{
    if (!n_arenas) return;
    keeper = std::thread([this]() {
        (void)hipSetDevice(ctx->device);
        vga_ctx_scope scope(ctx);
        while (!keeper_stop) {
            (void)list_new_segments();
            std::this_thread::sleep_for(std::chrono::milliseconds(1));
        }
    });
}

void poa_pool::stop_keeper()
{
    keeper_stop = true;
    if (keeper.joinable()) keeper.join();
}

// ---- the classic pool: one contiguous piece, cut into a part per slot; allocated when a classic launch is first needed
int poa_pool::ensure_classic()
{
    if (half_pool) return VGA_OK;
    const double want_d = classic_need * W.pool_scale * 1.3 + std::min<double>((double)n, classic_need / std::max(1.0, probe_mean) + 64.0) * 3.0 * (double)POA_CHUNK;
    const uint64_t want = (uint64_t)want_d + 64 * POA_CHUNK;
    uint64_t target = std::min(std::max<uint64_t>(2 * want, n_arenas ? 1ull << 30 : 8ull << 30), avail) & ~(POA_CHUNK - 1);
    if (W.classic_size < std::min<uint64_t>(want, target)) {
        if (W.classic) { (void)hipFree(W.classic); W.classic = nullptr; W.classic_size = 0; }
        if (target < 64 * POA_CHUNK) return vga_set_error(ctx, VGA_ERR_NOMEM, "only %llu bytes of HBM for the traceback pool", (unsigned long long)target);
        // the chunk segments give way (no chunk-mode launch is in flight when a classic one starts)
        size_t free_b = 0, total_b = 0;
        (void)hipMemGetInfo(&free_b, &total_b);
        if (free_b < target + (4ull << 30)) {
            std::lock_guard<std::mutex> list_lk(list_mu);  // (the keeper is not listing segments meanwhile)
            W.stop_grower();
            std::lock_guard<std::mutex> lk(W.mu);
            for (auto &g : W.segs) (void)hipFree(g.p);
            W.segs.clear(); W.pool_size = 0; W.segs_listed = 0; W.chunks_listed = 0; W.empties_seen = 0;
            if (W.d_head.p) (void)W.reset_lists();
            (void)hipMemGetInfo(&free_b, &total_b);
            target = std::min<uint64_t>(target, free_b > (4ull << 30) ? (free_b - (4ull << 30)) & ~(POA_CHUNK - 1) : target);
        }
        const hipError_t e = hipMalloc((void **)&W.classic, target);
        if (e != hipSuccess) return vga_set_error(ctx, VGA_ERR_NOMEM, "hipMalloc of the %llu byte traceback pool failed: %s", (unsigned long long)target, hipGetErrorString(e));
        W.classic_size = target;
    }
    half_pool = (W.classic_size / (uint64_t)n_slots) & ~(POA_CHUNK - 1);
    return VGA_OK;
}

void poa_pool::trace_mode()
{
    if (!tr.on) return;
    uint64_t ps; { std::lock_guard<std::mutex> lk(W.mu); ps = W.pool_size; }
    fprintf(stderr, "[vga-trace] poa: %s; chunk segments so far %.1f GB, %u state regions of %.2f MB, classic pool %.1f GB\n", n_arenas ? "chunk-pool mode" : "classic mode",
            (double)ps / 1e9, n_arenas, (double)state_size / 1e6, (double)W.classic_size / 1e9);
}

int poa_pool::check_and_trace_end()
{
    if (n_arenas && CP.owner) {
        unsigned long long bad[4] = {0, 0, 0, 0};
        (void)hipMemcpy(bad, CP.stats + 4, sizeof bad, hipMemcpyDeviceToHost);
        if (bad[0] || bad[1])
            return vga_set_error(ctx, VGA_ERR_HIP, "chunk pool check: %llu chunks were handed out while somebody held them, %llu (+ %llu broken chains) came back from somebody else "
                                 "(the first: chunk %llu held by %llu, pushed by %llu, position %llu of its chain, %llu threads)",
                                 bad[0], bad[1] & 0xFFFFFFFFull, bad[1] >> 32, bad[2] & 0xFFFFFFFFull, bad[2] >> 32, bad[3] & 0xFFFFFFFFull, (bad[3] >> 32) & 0xFFFFull, bad[3] >> 48);
    }
    if (tr.on && n_arenas) {
        unsigned long long empties = 0;
        (void)hipMemcpy(&empties, W.d_head.p + POA_LISTS * POA_LIST_STRIDE, sizeof empties, hipMemcpyDeviceToHost);
        uint64_t ps; { std::lock_guard<std::mutex> lk(W.mu); ps = W.pool_size; }
        fprintf(stderr, "[vga-trace] poa: chunk pool %.1f GB in %zu segments (%u chunks listed); since the context began %llu requests found every free list empty\n",
                (double)ps / 1e9, W.segs_listed, W.chunks_listed, empties);
    }
    return VGA_OK;
}
