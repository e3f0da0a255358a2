// vga_poa_pool.hpp -- the traceback pool of the POA engine as poa_run sees it (vga_poa_pool.hip): the context's workspace
// poa_ws (staging slots, chunk segments, state regions, classic pool) and a call's hold on it, poa_pool.
#pragma once

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "vga_common.hpp"
#include "vga_poa_launch.hpp"

// device + pinned staging of one sub-batch; sub-batches alternate between two of these (and two streams)
struct poa_slot {
    vga_dbuf<poa_prob> d_probs;
    vga_dbuf<uint4> d_ntab;
    vga_dbuf<uint32_t> d_seq32, d_preds, d_sink, d_orow, d_ids;
    vga_dbuf<uint8_t> d_ops;
    vga_dbuf<poa_row> d_rows;
    vga_dbuf<poa_out> d_outs;
    vga_dbuf<char> d_q;
    vga_hbuf<poa_prob> h_probs;
    vga_hbuf<uint4> h_ntab;
    vga_hbuf<uint32_t> h_seq32, h_preds, h_sink, h_ids;
    vga_hbuf<char> h_q;
    // results come back into one of two sets, alternating per use of the slot: the host is still reading set A of the
    // sub-batch that just finished when the next sub-batch on this slot is enqueued (it will write set B)
    // k_poa_text: cs / CIGAR / node path of every problem as text in a compact arena (claimed through d_tcur), one record each
    vga_dbuf<char> d_text;
    vga_dbuf<poa_text_out> d_touts;
    vga_dbuf<unsigned long long> d_tcur;
    struct out_set {
        vga_hbuf<uint32_t> h_orow;
        vga_hbuf<uint8_t> h_ops;
        vga_hbuf<char> h_seq;     // device store: the bases of the sub-batch's problems (row r of a problem is byte seq0 + r - 1)
        vga_hbuf<poa_out> h_outs;
        vga_hbuf<char> h_text;
        char *text_p = nullptr;  // where this launch's text is: h_text.p, or a buffer of poa_ws::text_live (poa_feed::keep_text)
        vga_hbuf<poa_text_out> h_touts;
        vga_hbuf<unsigned long long> h_tcur;
        bool text = false;        // this sub-batch's strings were written on the device
        uint64_t tot_ops = 0, tot_seq = 0;
    } outs[2];
    uint32_t uses = 0;
};

// The traceback pool: SEGMENTS of HBM, allocated one after the other by a thread of its own (`grower`) so that the first launch
// does not wait for all of it -- on a GPU whose memory was used before, the driver clears what it hands out at ~40 GB/s, and
// rounds 1-2 spent 0.4-7 s in one 257 GB hipMalloc before the first kernel of a process (and 1.6 s in the hipFree at its end).
// k_poa_dp_t5 takes the segments' 1 MiB chunks through a device-side free list (vga_poa_launch.hpp: poa_chunk_pool);
// classic launches (k_poa_dp_t4 / k_poa_dp_lds, problems the chunk mode hands back) bump-allocate inside whole segments --
// never at the same time as chunk-mode launches.
#define POA_SEG_LOG2 32  // 4 GiB segments (4 096 chunks)
#define POA_MAX_SEGS 80
struct poa_ws {
    poa_slot slot[POA_SLOTS];
    vga_dbuf<unsigned long long> d_next;
    vga_hbuf<unsigned long long> h_next;
    hipStream_t extra[POA_SLOTS] = {};  // streams of slots 1.. (slot 0 runs on the context's stream)
    double pool_scale = 1.35;  // measured pool bytes / estimated bytes, adapted after every sub-batch.  (Starts where config 3 ends up
                               // after a call: from 1.0 the second call of a process asked for a third more pool than the first --
                               // on memory the driver has to clear that is 0.4 s inside what bench.py times)
    // segments (guarded by mu)
    struct seg_t { uint8_t *p; uint64_t size; };
    std::mutex mu;
    std::condition_variable cv;
    std::vector<seg_t> segs;
    uint64_t pool_size = 0;     // bytes in segs
    uint64_t grow_target = 0;   // the grower stops at this many bytes
    uint8_t *classic = nullptr; // the classic pool: one contiguous piece (launches that do not run in chunk-pool mode)
    uint64_t classic_size = 0;
    bool growing = false, grow_failed = false;
    std::thread grower;
    int device = 0;
    vga_ctx *owner = nullptr;  // (the grower holds back while owner->alloc_urgent: vga_common.hpp)
    uint64_t seg_bytes = 1ull << POA_SEG_LOG2;
    // chunk pool (device side)
    vga_dbuf<unsigned long long> d_head;  // the free-list heads (POA_LISTS of them, a cache line apart), then the statistics
    vga_dbuf<uint32_t> d_next_chunk, d_slot_flag, d_owner;
    vga_hbuf<uint32_t> h_short;           // poa_chunk_pool::short_flag
    vga_hbuf<uint64_t> h_seg_base;        // staging of ...
    vga_dbuf<uint64_t> d_seg_base;        // ... the segment table the kernels read (an entry is copied before its chunks are listed)
    hipStream_t add_stream = nullptr;
    uint32_t chunks_listed = 0;           // chunks of segments [0, segs_listed) are in the free list
    uint64_t polls = 0, empties_seen = 0; // how often the kernels found the free list empty (poa_chunk_pool::stats[1]), as last read
    size_t segs_listed = 0;
    uint8_t *state = nullptr;             // the state regions
    uint64_t state_bytes = 0;
    // poa_feed::keep_text: the text of every launch of a call in a pinned buffer of its own, alive until the next call
    std::vector<std::unique_ptr<vga_hbuf<char>>> text_live, text_free;
    hipError_t reset_lists()  // every free list empty, statistics zero
    {
        std::vector<unsigned long long> init(POA_LISTS * POA_LIST_STRIDE + 16, 0ull);
        for (int l = 0; l < POA_LISTS; l++) init[(size_t)l * POA_LIST_STRIDE] = (unsigned long long)POA_NIL;
        const hipError_t e = hipMemcpy(d_head.p, init.data(), init.size() * sizeof(unsigned long long), hipMemcpyHostToDevice);
        return e != hipSuccess ? e : hipStreamSynchronize(nullptr);  // (the copy is on the device before anything is launched: see d_slot_flag)
    }
    // The small tables of the chunk pool (free-list heads, per-chunk links, state-region flags, the segment table and its pinned
    // staging, the kernels' shortage flag, the stream new segments are listed on).  Allocated BEFORE the grower is started: the
    // runtime serialises allocations, and a 16 KB hipMalloc or hipHostMalloc that queues behind the grower's 4 GiB segments
    // (0.1 s each while the driver clears them) held the first launch of a process back by 1.8-5.3 s
    bool tables_ready = false;
    hipError_t ensure_tables(uint32_t n_cu)
    {
        if (tables_ready) return hipSuccess;
        const uint32_t max_chunks = (uint32_t)(POA_MAX_SEGS * (1ull << (POA_SEG_LOG2 - 20)));
        hipError_t e;
        if ((e = d_head.reserve(POA_LISTS * POA_LIST_STRIDE + 16)) != hipSuccess) return e;
        if ((e = d_next_chunk.reserve(max_chunks)) != hipSuccess) return e;
        if ((e = d_slot_flag.reserve(16ull * (uint64_t)n_cu + 64)) != hipSuccess) return e;
        if ((e = h_seg_base.reserve(POA_MAX_SEGS)) != hipSuccess) return e;
        if ((e = h_short.reserve(16)) != hipSuccess) return e;
        h_short.p[0] = 0;
        if ((e = d_seg_base.reserve(POA_MAX_SEGS)) != hipSuccess) return e;
        if (!add_stream) {
            // (highest priority: when the pool does run short with the GPU full, the kernel that lists a new segment must be the
            // first to get the slot a workgroup frees)
            int pr_lo = 0, pr_hi = 0;
            (void)hipDeviceGetStreamPriorityRange(&pr_lo, &pr_hi);
            if ((e = hipStreamCreateWithPriority(&add_stream, hipStreamNonBlocking, pr_hi)) != hipSuccess) return e;
            if ((e = reset_lists()) != hipSuccess) return e;
        }
        tables_ready = true;
        return hipSuccess;
    }
    // vga_align_prepare: the state regions and the first segments, allocated on a thread of its own before the first
    // vga_align_batch call needs them (on memory another process used the driver clears what it hands out: 13 GB = 0.2 s)
    std::thread preparer;
    void prepare_async(uint64_t state_want, uint64_t pool_want, uint32_t n_cu)
    {
        join_preparer();
        preparer = std::thread([this, state_want, pool_want, n_cu]() {
            (void)hipSetDevice(device);
            if (ensure_tables(n_cu) != hipSuccess) (void)hipGetLastError();  // (poa_run asks again, and reports)
            if (state_bytes < state_want) {
                uint8_t *q = nullptr;
                if (hipMalloc((void **)&q, state_want) == hipSuccess) {
                    if (state) (void)hipFree(state);
                    state = q;
                    state_bytes = state_want;
                } else
                    (void)hipGetLastError();  // (poa_run asks again, and reports)
            }
            if (pool_want) request(pool_want);
        });
    }
    void join_preparer() { if (preparer.joinable()) preparer.join(); }
    void stop_grower()
    {
        { std::lock_guard<std::mutex> lk(mu); grow_target = 0; }
        if (grower.joinable()) grower.join();
    }
    ~poa_ws()
    {
        join_preparer();
        stop_grower();
        for (auto &g : segs) (void)hipFree(g.p);
        if (classic) (void)hipFree(classic);
        if (state) (void)hipFree(state);
        if (add_stream) (void)hipStreamDestroy(add_stream);
        for (int i = 0; i < POA_SLOTS; i++)
            if (extra[i]) (void)hipStreamDestroy(extra[i]);
    }
    // asks for a pool of at least `target` bytes; returns at once (the grower thread allocates)
    void request(uint64_t target)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (target <= pool_size || (growing && target <= grow_target)) return;
        grow_target = target;
        grow_failed = false;
        if (growing) return;
        if (grower.joinable()) grower.join();
        growing = true;
        grower = std::thread([this]() {
            (void)hipSetDevice(device);
            for (;;) {
                uint64_t want;
                {
                    std::lock_guard<std::mutex> lk2(mu);
                    if (pool_size >= grow_target || segs.size() >= POA_MAX_SEGS) { growing = false; cv.notify_all(); return; }
                    want = std::min<uint64_t>(seg_bytes, (grow_target - pool_size + POA_CHUNK - 1) & ~(POA_CHUNK - 1));
                }
                // allocations of the context's calls go first: none in progress, and none for the last 3 ms (a call reserves its
                // buffers one after the other)
                if (owner) {
                    auto quiet_since = std::chrono::steady_clock::now();
                    for (;;) {
                        if (owner->alloc_urgent.load() > 0) quiet_since = std::chrono::steady_clock::now();
                        else if (std::chrono::steady_clock::now() - quiet_since >= std::chrono::milliseconds(3)) break;
                        { std::lock_guard<std::mutex> lk2(mu); if (grow_target == 0) break; }  // (stop_grower)
                        std::this_thread::sleep_for(std::chrono::microseconds(300));
                    }
                }
                uint8_t *q = nullptr;
                const hipError_t e = hipMalloc((void **)&q, want);
                std::lock_guard<std::mutex> lk2(mu);
                if (e != hipSuccess) { (void)hipGetLastError(); growing = false; grow_failed = true; cv.notify_all(); return; }
                segs.push_back({q, want});
                pool_size += want;
                cv.notify_all();
            }
        });
    }
    // waits until `bytes` of pool exist or the grower has stopped; returns what exists
    uint64_t wait_for(uint64_t bytes)
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&]() { return pool_size >= bytes || !growing; });
        return pool_size;
    }
};

// the context's workspace, created on first use
poa_ws &poa_ws_of(vga_ctx *ctx);

// bytes of one state region of chunk-pool mode: the value-row ring, the wide-row scratch and a few kept value rows of a
// problem whose query has max_q bases
uint64_t poa_state_size(uint32_t max_q);

// What the first vga_align_batch call would allocate before its first kernel -- the state regions and about half of the chunk
// segments it is going to ask for -- starts to be allocated on a thread of its own (vga_align_prepare)
void poa_pool_prepare(vga_ctx *ctx, const poa_switches &sw, uint64_t n_reads, uint32_t max_read_len);

// the head of a call's launch order (its largest problems), as the pool's sizing sees it
struct poa_probe {
    uint64_t n = 0;            // problems probed
    double sum = 0, big = 0;   // their footprint estimates: total and largest
    double mean = 0;
    double long_sum = 0;       // estimated footprint of all very long problems of the call (poa_feed::klass), scaled up from the probed ones
    uint64_t long_all = 0;     // how many of those the call holds
    double bulk_mean = 0;      // mean footprint of the others
};

// A call's hold on the traceback pool: how much it may take, the chunk pool (state regions, segments, free lists and the
// keeper thread that looks after them) or the classic pool.
struct poa_pool {
    vga_ctx *ctx;
    poa_ws &W;
    const poa_switches &sw;
    vga_trace &tr;
    uint64_t n;                 // problems of the call
    int n_slots = 2;            // launches in flight (the classic pool is cut into a part for each)
    uint64_t avail = 0;         // bytes this context may take of the GPU for the pool
    uint64_t state_size = 0;
    uint32_t n_arenas = 0;      // state regions (0: classic mode for the whole call)
    poa_chunk_pool CP = {};
    uint64_t half_pool = 0;     // a slot's part of the classic pool (0: not obtained yet)
    double classic_need = 0;    // estimated bytes of the problems that will run in classic mode (the whole call, or what chunk mode handed back)
    double probe_mean = 0;
    std::mutex list_mu;         // (locking order: list_mu, then poa_ws::mu)
    std::atomic<bool> keeper_stop{false};
    std::thread keeper;

    poa_pool(vga_ctx *c, poa_ws &w, const poa_switches &s, vga_trace &t, uint64_t n_problems) : ctx(c), W(w), sw(s), tr(t), n(n_problems) {}
    ~poa_pool() { stop_keeper(); }
    int measure();                               // fills `avail`
    int obtain_chunks(const poa_probe &pr, hipStream_t st);  // chunk-pool mode: sets n_arenas and CP when the pool stands (else leaves classic mode)
    hipError_t list_new_segments();              // new segments' chunks join the free lists; a shortage makes the pool grow
    void start_keeper();
    void stop_keeper();
    int ensure_classic();                        // the classic pool, when a classic launch is first needed
    void trace_mode();
    int check_and_trace_end();                   // VGA_POOL_CHECK's verdict, and the trace's summary of the chunk pool
};
