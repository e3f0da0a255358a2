// vga_sort_scan.hpp -- the exclusive scan and the stable radix sort of the index build (vga_index.hip), which the deletion call
// (vga_deletion.hip) runs as well: k_ix_scan_block / _add, k_ix_radix_hist / _scatter and their drivers ix_build::scan / radix, moved
// here as they were.  Everything is in an anonymous namespace: each translation unit that includes this keeps its own copy of the
// kernels, so nothing is shared at link time and the index build's code objects are what they were.
#pragma once

#include "vga_common.hpp"

#include <algorithm>

namespace {

constexpr int IX_SCAN_NT = 256, IX_SCAN_PER = 4;
constexpr int IX_RADIX_NT = 256, IX_RADIX_ROWS = 16;  // radix tile: 16 rows of 256 elements
constexpr uint64_t IX_RADIX_TILE = (uint64_t)IX_RADIX_NT * IX_RADIX_ROWS;

// ---------------------------------------------------------------- exclusive scan (u64), out[n] = total
__global__ __launch_bounds__(IX_SCAN_NT) void k_ix_scan_block(const uint64_t *in, uint64_t n_in, uint64_t n_out, uint64_t *out,
                                                               uint64_t *block_sum)
{
    __shared__ uint64_t s[IX_SCAN_NT];
    const uint64_t b0 = (uint64_t)blockIdx.x * IX_SCAN_NT * IX_SCAN_PER + (uint64_t)threadIdx.x * IX_SCAN_PER;
    uint64_t v[IX_SCAN_PER], sum = 0;
    for (int r = 0; r < IX_SCAN_PER; r++) {
        v[r] = b0 + r < n_in ? in[b0 + r] : 0;
        sum += v[r];
    }
    s[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < IX_SCAN_NT; d <<= 1) {
        const uint64_t x = threadIdx.x >= (unsigned)d ? s[threadIdx.x - d] : 0;
        __syncthreads();
        s[threadIdx.x] += x;
        __syncthreads();
    }
    uint64_t run = s[threadIdx.x] - sum;
    for (int r = 0; r < IX_SCAN_PER; r++) {
        if (b0 + r < n_out) out[b0 + r] = run;
        run += v[r];
    }
    if (threadIdx.x == IX_SCAN_NT - 1) block_sum[blockIdx.x] = s[threadIdx.x];
}

__global__ void k_ix_scan_add(uint64_t *out, uint64_t n_out, const uint64_t *block_off)
{
    const uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < n_out) out[e] += block_off[e / (IX_SCAN_NT * IX_SCAN_PER)];
}

// ---------------------------------------------------------------- stable LSD radix sort of (u64 key, u32 value)
__global__ __launch_bounds__(IX_RADIX_NT) void k_ix_radix_hist(const uint64_t *key, uint64_t n, uint32_t shift, uint64_t n_tiles,
                                                                uint64_t *hist)
{
    __shared__ uint32_t cnt[256];
    cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t)blockIdx.x * IX_RADIX_TILE;
    for (int r = 0; r < IX_RADIX_ROWS; r++) {
        const uint64_t e = t0 + (uint64_t)r * IX_RADIX_NT + threadIdx.x;
        if (e < n) atomicAdd(&cnt[(key[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * n_tiles + blockIdx.x] = cnt[threadIdx.x];  // digit-major: the scan gives global offsets
}

// Element e of a tile goes to off[digit] + (elements of the same digit before it in this tile); ranks within a row of 256
// come from the wave's ballot match of the 8 digit bits (as K2, k_anchor_sort), rows are taken in order.
__global__ __launch_bounds__(IX_RADIX_NT) void k_ix_radix_scatter(const uint64_t *key, const uint32_t *val, uint64_t n, uint32_t shift,
                                                                   uint64_t n_tiles, const uint64_t *hoff, uint64_t *key_out,
                                                                   uint32_t *val_out)
{
    __shared__ uint64_t base[256];
    __shared__ uint32_t wave_cnt[IX_RADIX_NT / 64][256];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    base[tid] = hoff[(uint64_t)tid * n_tiles + blockIdx.x];
    const uint64_t lt = (1ull << lane) - 1ull;
    const uint64_t t0 = (uint64_t)blockIdx.x * IX_RADIX_TILE;
    for (int r = 0; r < IX_RADIX_ROWS; r++) {
        for (int x = 0; x < IX_RADIX_NT / 64; x++) wave_cnt[x][tid] = 0;
        __syncthreads();
        const uint64_t e = t0 + (uint64_t)r * IX_RADIX_NT + tid;
        const bool valid = e < n;
        const uint64_t kv = valid ? key[e] : 0;
        const uint32_t d = (uint32_t)(kv >> shift) & 255u;
        uint64_t m = __ballot(valid);
        for (int b = 0; b < 8; b++) {
            const uint64_t bal = __ballot((d >> b) & 1u);
            m &= ((d >> b) & 1u) ? bal : ~bal;
        }
        const uint32_t rank = __popcll(m & lt);
        if (valid && rank == 0) wave_cnt[w][d] = __popcll(m);
        __syncthreads();
        if (valid) {
            uint64_t p = base[d] + rank;
            for (int x = 0; x < w; x++) p += wave_cnt[x][d];
            key_out[p] = kv;
            val_out[p] = val[e];
        }
        __syncthreads();
        uint32_t row = 0;
        for (int x = 0; x < IX_RADIX_NT / 64; x++) row += wave_cnt[x][tid];
        base[tid] += row;
        __syncthreads();
    }
}

// ---------------------------------------------------------------- host side
inline unsigned ix_grid(uint64_t n, unsigned nt) { return (unsigned)((n + nt - 1) / nt); }

// device buffers of one build, released together (hipFree waits for the work queued on them)
struct ix_scratch {
    std::vector<void *> ptrs;
    hipError_t err = hipSuccess;
    template <typename T>
    T *get(uint64_t n)
    {
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, std::max<uint64_t>(n, 1) * sizeof(T));
        if (e != hipSuccess) { (void)hipGetLastError(); if (err == hipSuccess) err = e; return nullptr; }
        ptrs.push_back(p);
        return (T *)p;
    }
    ~ix_scratch() { for (void *p : ptrs) (void)hipFree(p); }
};

struct ix_build {
    vga_ctx *ctx;
    ix_scratch mem;
    hipStream_t st;
    const char *who = "vga_index_build_kmers";  // the entry point the messages name

    int nomem(const char *what, uint64_t n)
    {
        return vga_set_error(ctx, VGA_ERR_NOMEM, "%s: no device memory for %s (%llu elements)", who, what,
                             (unsigned long long)n);
    }

    // out[0..n] = exclusive scan of in[0..n), out[n] = the total
    int scan(const uint64_t *in, uint64_t n, uint64_t *out)
    {
        const uint64_t per = (uint64_t)IX_SCAN_NT * IX_SCAN_PER, n_out = n + 1, nb = (n_out + per - 1) / per;
        uint64_t *bs = mem.get<uint64_t>(nb + 1);
        if (!bs) return nomem("scan", nb);
        hipLaunchKernelGGL(k_ix_scan_block, dim3((unsigned)nb), dim3(IX_SCAN_NT), 0, st, in, n, n_out, out, bs);
        if (nb > 1) {
            uint64_t *bo = mem.get<uint64_t>(nb + 1);
            if (!bo) return nomem("scan", nb);
            if (int rc = scan(bs, nb, bo)) return rc;
            hipLaunchKernelGGL(k_ix_scan_add, dim3(ix_grid(n_out, 256)), dim3(256), 0, st, out, n_out, (const uint64_t *)bo);
        }
        return VGA_OK;
    }

    uint64_t read_u64(const uint64_t *d)
    {
        uint64_t v = 0;
        if (hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return UINT64_MAX;
        return v;
    }

    // stable sort of (key, val) by the low `bits` bits of key; on return (key, val) point to the sorted copy (two new
    // buffers take the passes in turn: the input arrays are left as they were)
    int radix(uint64_t *&key, uint32_t *&val, uint64_t n, uint32_t bits)
    {
        if (n == 0) return VGA_OK;
        const uint64_t n_tiles = (n + IX_RADIX_TILE - 1) / IX_RADIX_TILE;
        uint64_t *k2 = mem.get<uint64_t>(n), *k3 = mem.get<uint64_t>(n), *hist = mem.get<uint64_t>(256 * n_tiles),
                 *hoff = mem.get<uint64_t>(256 * n_tiles + 1);
        uint32_t *v2 = mem.get<uint32_t>(n), *v3 = mem.get<uint32_t>(n);
        if (!k2 || !k3 || !v2 || !v3 || !hist || !hoff) return nomem("the radix sort", n);
        for (uint32_t shift = 0; shift < bits; shift += 8) {
            hipLaunchKernelGGL(k_ix_radix_hist, dim3((unsigned)n_tiles), dim3(IX_RADIX_NT), 0, st, (const uint64_t *)key, n, shift, n_tiles, hist);
            if (int rc = scan(hist, 256 * n_tiles, hoff)) return rc;
            hipLaunchKernelGGL(k_ix_radix_scatter, dim3((unsigned)n_tiles), dim3(IX_RADIX_NT), 0, st, (const uint64_t *)key,
                               (const uint32_t *)val, n, shift, n_tiles, (const uint64_t *)hoff, k2, v2);
            key = k2;
            val = v2;
            std::swap(k2, k3);
            std::swap(v2, v3);
        }
        return VGA_OK;
    }
};

}  // namespace
