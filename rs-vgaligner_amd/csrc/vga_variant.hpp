// vga_variant.hpp -- the integer-only diploid call at every graph base (vga_variant.hip): the limits host and device share.
//
// Nothing in the reference stands behind this.  It is the first consumer of the pileup table (vga_pileup.hpp) that stays on the
// device: one thread per base turns the seven counters into a genotype over the alleles A C G T D and an insertion state
// (include/vga_hip.h has the definition, tests/variant_ref.py recomputes it), the few bases that differ from the graph are
// compacted in base order, and only those cross PCIe.
#pragma once

#include <cstdint>

// threads of a workgroup of k_vc_count / k_vc_emit (one base each) and of k_vc_scan
#define VC_BLOCK 256u
#define VC_SCAN_BLOCK 1024u
// the cost E of an observation that neither allele explains, in 1/256 bit: more than the 256 a heterozygous pair pays for one it
// does explain, and small enough that 6 * 2^40 * E stays far below 2^64
#define VC_MIN_ERROR 257u
#define VC_MAX_ERROR 8192u
// a counter of the explicit table (vga_variant_call_table) has to stay below this
#define VC_MAX_COUNT (1ull << 40)
// the bases of an explicit table: positions are 32-bit
#define VC_MAX_BASES (1ull << 31)
// gt byte of a call: x | y << 3 | insertion state << 6, with x <= y in 0..4 (A C G T D) and the state 0 none, 1 het, 2 hom
#define VC_GT(x, y) ((uint32_t)(x) | ((uint32_t)(y) << 3))
