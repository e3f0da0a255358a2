// vga_strand.hip -- the reverse complement of a read batch, for vga_map_params.strands = VGA_STRANDS_BOTH.
//
// The reverse complement of read r is written once per batch, directly after the forward bases of the same device
// allocation: it starts at total_bases + read_off[r].  K1-K3 (vga_map.hip) then run unchanged over 2 n_reads virtual reads
// (d_read_off2), and vga_align_batch takes the query of a reverse read from that half.  The reference has no such mode: its
// reverse_complement (src/dna.rs:5-17) is only used on graph sequence; the byte map is its switch_base (src/dna.rs:20-33).
#include "vga_common.hpp"

#include <algorithm>
#include <cstring>

#define VGA_RC_NT 256
#define VGA_RC_TILE (VGA_RC_NT * 4)  // output bytes per tile: one 32-bit word per thread

// switch_base: A<->T, C<->G, a<->t, c<->g, U->A, u->a; any other byte becomes N (the reference panics on bytes outside
// is_dna; nothing panics across the C ABI)
__host__ __device__ static inline uint8_t vga_switch_base(uint8_t c)
{
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'U': return 'A';
    case 'a': return 't';
    case 'c': return 'g';
    case 'g': return 'c';
    case 't': return 'a';
    case 'u': return 'a';
    default: return 'N';
    }
}

// One block per read, tiles of 1 024 output bytes.  A tile's source is the mirrored window of the forward read: it is staged
// in LDS with aligned, coalesced 32-bit loads (from the word that holds its first byte), and written complemented and
// mirrored with aligned, coalesced 32-bit stores.  Reads start at any byte offset: a destination word that the tile covers
// only in part (its head and tail) is written byte by byte, so no store touches a byte of another read.  The loads stay
// inside the allocation (total_bases + 64 bytes beyond the forward half).
__global__ __launch_bounds__(VGA_RC_NT) void k_revcomp_reads(char *reads, const uint64_t *__restrict__ read_off, uint64_t total)
{
    __shared__ uint8_t comp[256];
    __shared__ uint32_t tile[VGA_RC_TILE / 4 + 2];
    const uint32_t tid = threadIdx.x;
    comp[tid] = vga_switch_base((uint8_t)tid);
    const uint64_t off = read_off[blockIdx.x], L = read_off[blockIdx.x + 1] - off;
    const uint32_t *rw = (const uint32_t *)reads;
    uint32_t *ww = (uint32_t *)reads;
    for (uint64_t i0 = 0; i0 < L; i0 += VGA_RC_TILE) {
        const uint32_t n = (uint32_t)std::min<uint64_t>(VGA_RC_TILE, L - i0);
        // forward bytes [s0, s0 + n) become output bytes [d0, d0 + n), mirrored
        const uint64_t s0 = off + L - i0 - n, d0 = total + off + i0;
        const uint32_t sh = (uint32_t)(s0 & 3u), dsh = (uint32_t)(d0 & 3u);
        const uint32_t nw = (sh + n + 3) >> 2, ndw = (dsh + n + 3) >> 2;
        __syncthreads();  // (comp, on the first tile; the previous tile's reads of `tile` on the others)
        for (uint32_t w = tid; w < nw; w += VGA_RC_NT) tile[w] = rw[(s0 >> 2) + w];
        __syncthreads();
        const uint8_t *src = (const uint8_t *)tile + sh;  // src[j] = forward byte s0 + j
        for (uint32_t w = tid; w < ndw; w += VGA_RC_NT) {
            const int x0 = (int)(4 * w) - (int)dsh;  // output bytes x0 .. x0 + 3 of the tile
            if (x0 >= 0 && x0 + 4 <= (int)n) {
                uint32_t v = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) v |= (uint32_t)comp[src[n - 1 - (uint32_t)(x0 + q)]] << (8 * q);
                ww[(d0 >> 2) + w] = v;
            } else {
                for (int q = 0; q < 4; q++) {
                    const int x = x0 + q;
                    if (x >= 0 && x < (int)n) reads[d0 + (uint64_t)x] = (char)comp[src[n - 1 - (uint32_t)x]];
                }
            }
        }
    }
}

int vga_batch_revcomp_device(vga_batch *b)
{
    if (b->rc_dev) return VGA_OK;
    vga_ctx *ctx = b->ctx;
    const uint64_t T = b->total_bases, R = b->n_reads;
    hipStream_t st = ctx->stream;
    std::vector<uint64_t> off2(2 * R + 1);
    for (uint64_t r = 0; r <= R; r++) off2[r] = b->read_off[r];
    for (uint64_t r = 1; r <= R; r++) off2[R + r] = T + b->read_off[r];
    char *d2 = nullptr;
    uint64_t *d_off2 = nullptr;
    hipError_t e = hipMalloc((void **)&d2, 2 * T + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&d_off2, (2 * R + 1) * sizeof(uint64_t));
    if (e == hipSuccess && T) e = hipMemcpyAsync(d2, b->d_reads, T, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_off2, off2.data(), (2 * R + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && R) {
        const int t = vga_timer_begin(ctx, "revcomp_reads", 2 * T);
        hipLaunchKernelGGL(k_revcomp_reads, dim3((unsigned)R), dim3(VGA_RC_NT), 0, st, d2, b->d_read_off, T);
        vga_timer_end(ctx, t);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(st);
        if (d2) (void)hipFree(d2);
        if (d_off2) (void)hipFree(d_off2);
        return vga_set_error(ctx, VGA_ERR_HIP, "reverse complement of the batch: %s", hipGetErrorString(e));
    }
    (void)hipFree(b->d_reads);
    b->d_reads = d2;
    b->d_read_off2 = d_off2;
    b->rc_dev = true;
    return VGA_OK;
}

void vga_batch_revcomp_host(vga_batch *b)
{
    if (b->rc_host) return;
    const uint64_t T = b->total_bases;
    b->reads.resize(2 * T);
    char *s = b->reads.data();
    vga_parallel_for(b->n_reads, [&](uint64_t r) {
        const uint64_t off = b->read_off[r], L = b->read_off[r + 1] - off;
        for (uint64_t i = 0; i < L; i++) s[T + off + i] = (char)vga_switch_base((uint8_t)s[off + L - 1 - i]);
    }, (unsigned)std::max<uint64_t>(1, T / 4000000));
    b->rc_host = true;
}

// The kernel seam: what the two routes above left (or now leave) in the batch, copied out.  Nothing else reads a reverse half
// back; the map and align kernels take it where it is.
static int batch_strands(vga_batch *b, int from_host, char *forward, char *reverse)
{
    vga_ctx *ctx = b->ctx;
    (void)hipSetDevice(ctx->device);
    vga_ctx_scope scope(ctx);
    const uint64_t T = b->total_bases;
    if (from_host) {
        vga_batch_revcomp_host(b);
        if (T && forward) memcpy(forward, b->reads.data(), T);
        if (T && reverse) memcpy(reverse, b->reads.data() + T, T);
        return VGA_OK;
    }
    vga_timers_reset(ctx);
    const int rc = vga_batch_revcomp_device(b);
    if (rc != VGA_OK) return rc;
    if (T && forward) VGA_HIP_CHECK(ctx, hipMemcpyAsync(forward, b->d_reads, T, hipMemcpyDeviceToHost, ctx->stream));
    if (T && reverse) VGA_HIP_CHECK(ctx, hipMemcpyAsync(reverse, b->d_reads + T, T, hipMemcpyDeviceToHost, ctx->stream));
    VGA_HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    vga_timers_collect(ctx);
    return VGA_OK;
}

extern "C" int vga_batch_strands(vga_batch *b, int from_host, char *forward, char *reverse)
{
    if (!b || !b->ctx) return VGA_ERR_ARG;  // b->ctx == nullptr: the context was destroyed
    try {
        return batch_strands(b, from_host, forward, reverse);
    } catch (const std::bad_alloc &) {
        return vga_set_error(b->ctx, VGA_ERR_NOMEM, "vga_batch_strands: out of host memory");
    }
}
