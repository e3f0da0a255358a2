// vga_probe_hash.hpp -- the hashed k-mer probe table (16 <= k <= 32): slot layout, hash and slot arithmetic.
//
// The one definition host and device code share: vga_ctx.hip sizes and fills the table (k_probe_hash_insert), vga_map.hip
// walks it (k_kmer_probe<.., true>), and the CPU tests compile this header alone with a host compiler.
//
// Open addressing, linear probing, capacity a power of two >= 2 * keys (load <= 1/2).  The key is the 2-bit packed k-mer
// (A=0 C=1 G=2 T=3, first base in the highest used bits).  At k = 32 every 64-bit pattern is a valid key, so a slot is
// empty when its claim word hdr_all is VGA_HASH_EMPTY, never by a key sentinel: every k-mer of an index has a group in the
// all-orientation position array, so hdr_all of a used slot is a real header index, and hdr_ff is VGA_HASH_EMPTY for a
// k-mer without a forward/forward record (a forward-only probe then misses, as it does in the direct table).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VGA_HD __host__ __device__ __forceinline__
#else
#define VGA_HD inline
#endif

#define VGA_HASH_EMPTY 0xFFFFFFFFu

struct alignas(16) vga_hash_slot {
    uint64_t key;
    uint32_t hdr_all;  // header index into pos_all; the claim word (VGA_HASH_EMPTY: the slot is empty)
    uint32_t hdr_ff;   // header index into pos (forward/forward records), or VGA_HASH_EMPTY
};

// the 64-bit finaliser of MurmurHash3 (public domain, Austin Appleby): a bijection on 64 bits
VGA_HD uint64_t vga_hash_mix64(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return x;
}

// smallest power of two >= 2 * n_keys (and >= 16); 0 when that does not fit 32-bit slot indices
VGA_HD uint64_t vga_hash_capacity(uint64_t n_keys)
{
    if (n_keys > (1ull << 30)) return 0;
    uint64_t cap = 16;
    while (cap < 2 * n_keys) cap <<= 1;
    return cap;
}

VGA_HD uint32_t vga_hash_first_slot(uint64_t key, uint32_t mask) { return (uint32_t)vga_hash_mix64(key) & mask; }
VGA_HD uint32_t vga_hash_next_slot(uint32_t slot, uint32_t mask) { return (slot + 1u) & mask; }

// ---- host-side mirror of the insert kernel and of K1's walk (the upload's self-check, the CPU tests)
// inserts a key that is not in the table yet; false when the table is full
inline bool vga_hash_insert_host(vga_hash_slot *slots, uint32_t mask, uint64_t key, uint32_t hdr_all, uint32_t hdr_ff)
{
    uint32_t s = vga_hash_first_slot(key, mask);
    for (uint64_t n = 0; n <= mask; n++, s = vga_hash_next_slot(s, mask)) {
        if (slots[s].hdr_all != VGA_HASH_EMPTY) continue;
        slots[s].key = key;
        slots[s].hdr_all = hdr_all;
        slots[s].hdr_ff = hdr_ff;
        return true;
    }
    return false;
}

// the slot that holds `key`, or nullptr
inline const vga_hash_slot *vga_hash_find_host(const vga_hash_slot *slots, uint32_t mask, uint64_t key)
{
    uint32_t s = vga_hash_first_slot(key, mask);
    for (uint64_t n = 0; n <= mask; n++, s = vga_hash_next_slot(s, mask)) {
        if (slots[s].hdr_all == VGA_HASH_EMPTY) return nullptr;
        if (slots[s].key == key) return &slots[s];
    }
    return nullptr;
}
