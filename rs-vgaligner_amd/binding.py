"""ctypes binding of libvga_hip.so (the C ABI declared in include/vga_hip.h).

This is plumbing for tests, bench.py and the Python drivers; the product is the shared library.
There is no CPU fallback: if the library is missing, or no gfx950 device is visible, every entry
point raises.  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VGA_LIB") or os.path.join(_HERE, "libvga_hip.so")  # VGA_LIB: another build of the library (same-box A/B runs)

VGA_OK = 0
# vga_map_params.strands
VGA_MAX_KMER_LENGTH = 32  # include/vga_hip.h: the longest k-mer vga_index_upload accepts (hashed probe table from k = 16)
VGA_STRANDS_FORWARD = 0
VGA_STRANDS_BOTH = 1
ERR_NAMES = {-1: "VGA_ERR_ARG", -2: "VGA_ERR_HIP", -3: "VGA_ERR_NOMEM", -4: "VGA_ERR_UNSUPPORTED",
             -5: "VGA_ERR_NO_INDEX", -6: "VGA_ERR_NO_DEVICE", -7: "VGA_ERR_POOL"}

# the columns of vga_pileup_read's table
PILEUP_COLUMNS = ("A", "C", "G", "T", "N", "del", "ins")

# every symbol include/vga_hip.h declares
ABI_SYMBOLS = [
    "vga_ctx_create", "vga_ctx_destroy", "vga_last_error", "vga_ctx_synchronize", "vga_abi_version",
    "vga_index_upload", "vga_batch_create", "vga_batch_destroy", "vga_batch_strands", "vga_map_default_params", "vga_map_batch",
    "vga_map_result_free", "vga_poa_default_params", "vga_poa_result_free", "vga_poa_batch", "vga_align_batch",
    "vga_align_result_free", "vga_last_kernel_times", "vga_chain_paths_text", "vga_chain_text_free",
    "vga_align_prepare", "vga_ctx_set_pool_fraction", "vga_ctx_set_host_threads",
    "vga_index_build_kmers", "vga_index_kmers_free",
    "vga_coverage_begin", "vga_coverage_read", "vga_coverage_reset", "vga_coverage_end",
    "vga_path_support_begin", "vga_path_support_read", "vga_path_support_last", "vga_path_support_reset", "vga_path_support_end",
    "vga_path_support_lists",
    "vga_pileup_begin", "vga_pileup_read", "vga_pileup_reset", "vga_pileup_end",
    "vga_genotype_begin", "vga_genotype_read", "vga_genotype_reset", "vga_genotype_end", "vga_genotype_pairs",
    "vga_genotype_lik_table", "vga_genotype_lik_begin", "vga_genotype_lik_read", "vga_genotype_lik_reset", "vga_genotype_lik_end",
    "vga_genotype_lik_pairs", "vga_genotype_lik_source",
    "vga_path_edit_begin", "vga_path_edit_read", "vga_path_edit_last", "vga_path_edit_reset", "vga_path_edit_end", "vga_path_edit_pairs",
    "vga_variant_call", "vga_variant_call_table",
    "vga_insertion_begin", "vga_insertion_read", "vga_insertion_reset", "vga_insertion_end", "vga_insertion_call", "vga_insertion_call_table",
    "vga_deletion_begin", "vga_deletion_read", "vga_deletion_reset", "vga_deletion_end", "vga_deletion_call", "vga_deletion_call_table", "vga_deletion_state",
    "vga_phase_begin", "vga_phase_read", "vga_phase_reset", "vga_phase_end", "vga_phase_links", "vga_phase_links_lists", "vga_phase_chain",
    "vga_phase_tags", "vga_phase_tags_lists",
    "vga_haplotype_counts", "vga_haplotype_counts_lists", "vga_haplotype_jobs", "vga_haplotype_call",
    "vga_phase_set_links", "vga_phase_set_links_lists", "vga_phase_join",
    "vga_haplotype_paths_begin", "vga_haplotype_paths_end", "vga_haplotype_paths_store", "vga_haplotype_paths", "vga_haplotype_paths_lists",
    "vga_haplotype_paths_rank",
    "vga_path_abundance_table", "vga_path_abundance_begin", "vga_path_abundance_reset", "vga_path_abundance_end", "vga_path_abundance_store",
    "vga_path_abundance", "vga_path_abundance_rows",
]

# k_gt_pairs (csrc/vga_genotype.hpp): the paths on a side of a workgroup's tile (GT_TILE), the reads it stages at a time
# (GT_READS), and the chunks of GT_READS reads a workgroup takes before the reads are split over more workgroups (GT_MIN_CHUNKS)
GENOTYPE_TILE = 64
GENOTYPE_READS = 32
GENOTYPE_MIN_CHUNKS = 4
GENOTYPE_MAX_PATHS = 4096

# k_gl_pairs (csrc/vga_genotype_lik.hpp): the paths on a side of a workgroup's tile (GL_TILE), the reads it stages at a time
# (GL_READS), the chunks of GL_READS reads a workgroup takes before the reads are split over more workgroups (GL_MIN_CHUNKS), the
# reads whose cost its 32-bit accumulators hold (GL_MAX_GROUP_READS), and the ranges of the two parameters
GENOTYPE_LIK_TILE = 128
GENOTYPE_LIK_READS = 32
GENOTYPE_LIK_MIN_CHUNKS = 4
GENOTYPE_LIK_MAX_GROUP_READS = 2048
GENOTYPE_LIK_MAX_PATHS = 4096
GENOTYPE_LIK_MAX_LAMBDA = 4096
GENOTYPE_LIK_MAX_CAP = 255
GENOTYPE_LIK_LAMBDA = 512  # the defaults of Context.genotype_likelihood_begin and of `vgaligner map --genotype-likelihood`
GENOTYPE_LIK_CAP = 64
# vga_genotype_lik_source: the matrices the likelihood reads
VGA_GL_FROM_SUPPORT = 0
VGA_GL_FROM_EDIT = 1
GENOTYPE_LIK_SOURCES = {"support": VGA_GL_FROM_SUPPORT, "edit": VGA_GL_FROM_EDIT}

# k_pe_dist (csrc/vga_path_edit.hpp): e of a pair that is not scored, the most 64-row blocks a lane owns (PE_MAX_R; the kernel is
# instantiated for 1, 2 and 4) and the longest query 64 such lanes hold (PE_MAX_QUERY)
PATH_EDIT_NONE = 0xFFFFFFFF
PATH_EDIT_MAX_R = 4
PATH_EDIT_MAX_QUERY = 64 * 64 * PATH_EDIT_MAX_R
PATH_EDIT_FIELDS = ("n_scored", "sum_edit", "best", "best_alone")

# k_vc_count / k_vc_emit (csrc/vga_variant.hpp): the bases of a workgroup, the range of the error cost E, the counters and the
# rows vga_variant_call_table serves, and the defaults of Context.variant_call and of `vgaligner map --call-variants`
VARIANT_BLOCK = 256
VARIANT_MIN_ERROR = 257
VARIANT_MAX_ERROR = 8192
VARIANT_MAX_COUNT = 1 << 40
VARIANT_MAX_BASES = 1 << 31
VARIANT_ERROR = 1280
VARIANT_MIN_DEPTH = 4
VARIANT_MIN_QUAL = 512
VARIANT_ALLELES = "ACGT-"  # alleles 0..4 as <out>-variants.tsv writes them: D, the deleted base, is '-'
VARIANT_INS_STATES = (".", "het", "hom")

# the deletion events (csrc/vga_deletion.hpp): the words of an event (first, len, last), the first size of the grow-only store in
# events, the events one call takes, the bound of a 64-bit counter of vga_deletion_call_table, and the states of a call
DELETION_EVENT_WORDS = 3
DELETION_STORE_EVENTS0 = 1024
DELETION_MAX_EVENTS = (1 << 32) - 1
DELETION_MAX_COUNT = 1 << 40
DELETION_STATES = ("none", "het", "hom")
# the insertion table (csrc/vga_insertion.hpp): the letters of an inserted run that are kept, and the 32-bit counters of a graph
# base -- the bins of length 1 .. 8 and `more`, then per kept position the letters A C G T N; the graph and the counters that
# vga_insertion_begin and vga_insertion_call_table serve
INSERTION_MAX_LEN = 8
INSERTION_COLS = 9 + INSERTION_MAX_LEN * 5
INSERTION_LETTERS = "ACGTN"
INSERTION_MAX_SEQ = 1 << 26
INSERTION_MAX_COUNT = 1 << 40

# the phase links (csrc/vga_phase.hpp): sites at most this far apart in site order are linked, the default of --phase-min-links
# and its upper bound, the columns of a sparse word of the store (A C G T, another letter, deleted, insertion)
PHASE_WINDOW = 8
PHASE_MIN_LINKS = 2
PHASE_MAX_MIN_LINKS = 65535
PHASE_COLS = 7
# a row of the haplotype tags: read, ps, votes_a, votes_b
PHASE_TAG_COLS = 4
# a row of the haplotype counts (csrc/vga_hapcall.hpp): c, ps, a[0 .. 6], b[0 .. 6]; the calls and the jobs of one call at most
HAPLOTYPE_ROW = 16
HAPLOTYPE_MAX_CALLS = 1 << 24
HAPLOTYPE_MAX_JOBS = 1 << 24
# the set links (csrc/vga_phase_join.hpp): a row of the table is (a, a), (a, b), (b, a), (b, b); the sets of one call at most; the
# side of k_sj_pairs' tile of set pairs; --phase-join-min-reads
PHASE_JOIN_COLS = 4
PHASE_JOIN_MAX_SETS = 4096
PHASE_JOIN_TILE = 32
PHASE_JOIN_MIN_READS = 2
PHASE_JOIN_MAX_MIN_READS = 65535
# the haplotype paths (csrc/vga_hap_paths.hpp): an entry of the table is (cost, best); the cap of a deficit and its default; the
# paths, sets and table entries of one call at most; the paths of k_hp_sums' workgroup; the matrices a score is summed from
HAPLOTYPE_PATHS_COLS = 2
HAPLOTYPE_PATHS_CAP = 64
HAPLOTYPE_PATHS_MAX_CAP = 255
HAPLOTYPE_PATHS_MAX_PATHS = 4096
HAPLOTYPE_PATHS_MAX_SETS = 4096
HAPLOTYPE_PATHS_MAX_ENTRIES = 1 << 23
HAPLOTYPE_PATHS_CHUNK = 256
HAPLOTYPE_PATHS_SOURCES = {"support": 0, "edit": 1}
# the path abundance (csrc/vga_abundance.hpp): the defaults and ranges of its parameters (choices, not measurements), the paths and
# scored rows of one estimate, the fractional bits of theta and of a responsibility, the rows and paths of k_ab_estep's workgroup,
# the iterations the host enqueues at a time, the matrices a score is summed from
PATH_ABUNDANCE_LAMBDA = 512
PATH_ABUNDANCE_MAX_LAMBDA = 4096
PATH_ABUNDANCE_CAP = 64
PATH_ABUNDANCE_MAX_CAP = 255
PATH_ABUNDANCE_ITERS = 1000
PATH_ABUNDANCE_MAX_ITERS = 100000
PATH_ABUNDANCE_TOL = 16
PATH_ABUNDANCE_MAX_TOL = 1 << 24
PATH_ABUNDANCE_MAX_PATHS = 4096
PATH_ABUNDANCE_MAX_ROWS = 1 << 23
PATH_ABUNDANCE_THETA_BITS = 24
PATH_ABUNDANCE_RESP_BITS = 16
PATH_ABUNDANCE_GROUP_ROWS = 256
PATH_ABUNDANCE_MAX_GROUPS = 4096
PATH_ABUNDANCE_MAX_ROW_FACTOR = 8
PATH_ABUNDANCE_CHUNK = 1024
PATH_ABUNDANCE_BLOCK_ITERS = 32
PATH_ABUNDANCE_SOURCES = {"support": 0, "edit": 1}


class VgaError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERR_NAMES.get(code, code)}: {msg}")
        self.code = code


class KmerPos(C.Structure):
    _fields_ = [("start", C.c_uint64), ("end", C.c_uint64), ("start_orient", C.c_uint8), ("end_orient", C.c_uint8)]


KMERPOS_DTYPE = np.dtype({"names": ["start", "end", "start_orient", "end_orient"],
                          "formats": ["<u8", "<u8", "u1", "u1"], "offsets": [0, 8, 16, 17], "itemsize": C.sizeof(KmerPos)})


class IndexDesc(C.Structure):
    _fields_ = [
        ("kmer_length", C.c_uint32), ("seq_length", C.c_uint64), ("seq_fwd", C.c_char_p), ("n_nodes", C.c_uint64),
        ("node_seq_idx", C.POINTER(C.c_uint64)), ("node_edge_idx", C.POINTER(C.c_uint64)),
        ("node_edges_to", C.POINTER(C.c_uint64)), ("n_edges", C.c_uint64), ("edges", C.POINTER(C.c_uint64)),
        ("n_kmers", C.c_uint64), ("kmer_keys", C.c_char_p), ("kmer_starts", C.POINTER(C.c_uint64)),
        ("n_kmer_pos", C.c_uint64), ("kmer_pos_table", C.POINTER(KmerPos)),
    ]


class MapParams(C.Structure):
    _fields_ = [("bandwidth", C.c_uint32), ("max_gap", C.c_uint64), ("chain_min_n_anchors", C.c_uint32),
                ("only_forward", C.c_int), ("emit_dp", C.c_int), ("strands", C.c_int32)]


class PoaParams(C.Structure):
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_open1", C.c_int32), ("gap_ext1", C.c_int32),
                ("gap_open2", C.c_int32), ("gap_ext2", C.c_int32), ("wb", C.c_int32), ("remain_rule", C.c_int32), ("wf", C.c_double)]


_P = C.POINTER


class ChainText(C.Structure):
    _fields_ = [("n_chains", C.c_uint64), ("text_off", C.POINTER(C.c_uint64)), ("text", C.POINTER(C.c_char)), ("ms_total", C.c_float)]


class MapResult(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("n_anchors", C.c_uint64), ("anchor_off", _P(C.c_uint64)), ("anchor_id", _P(C.c_uint32)),
        ("query_begin", _P(C.c_uint32)), ("target_begin", _P(C.c_uint32)), ("target_end", _P(C.c_uint32)),
        ("max_chain_score", _P(C.c_double)), ("best_pred_id", _P(C.c_int32)), ("curr_max", _P(C.c_double)),
        ("n_chains", C.c_uint64), ("chain_off", _P(C.c_uint64)), ("chain_placeholder", _P(C.c_uint8)),
        ("chain_anchor_off", _P(C.c_uint64)), ("chain_anchor_idx", _P(C.c_uint32)),
        ("ms_probe", C.c_float), ("ms_sort", C.c_float), ("ms_chain", C.c_float), ("ms_total", C.c_float),
        ("n_hits", C.c_uint64), ("strand", _P(C.c_uint8)),
    ]


class PoaResult(C.Structure):
    _fields_ = [
        ("n", C.c_uint64), ("ok", _P(C.c_uint8)), ("best_score", _P(C.c_int32)), ("path_off", _P(C.c_uint64)),
        ("abpoa_nodes", _P(C.c_uint32)), ("graph_nodes", _P(C.c_uint32)), ("aln_start_offset", _P(C.c_uint32)),
        ("aln_end_offset", _P(C.c_uint32)), ("n_aligned_bases", _P(C.c_uint32)), ("cigar_off", _P(C.c_uint64)),
        ("cigar", _P(C.c_char)), ("cs_off", _P(C.c_uint64)), ("cs", _P(C.c_char)), ("n_rows", _P(C.c_uint64)),
        ("n_cells", _P(C.c_uint64)), ("n_value_cells", _P(C.c_uint64)), ("ms_dp", C.c_float), ("ms_traceback", C.c_float), ("ms_total", C.c_float),
    ]


class AlignResult(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint64), ("aligned", _P(C.c_uint8)), ("path_off", _P(C.c_uint64)), ("path_handles", _P(C.c_uint64)),
        ("path_length", _P(C.c_uint32)), ("path_start", _P(C.c_uint32)), ("path_end", _P(C.c_uint32)),
        ("block_length", _P(C.c_uint32)), ("best_score", _P(C.c_int32)), ("cigar_off", _P(C.c_uint64)),
        ("cigar", _P(C.c_char)), ("cs_off", _P(C.c_uint64)), ("cs", _P(C.c_char)),
        ("poa_rows", C.c_uint64), ("poa_cells", C.c_uint64), ("poa_value_cells", C.c_uint64), ("poa_problems", C.c_uint64),
        ("ms_subgraph", C.c_float), ("ms_dp", C.c_float), ("ms_traceback", C.c_float), ("ms_total", C.c_float),
        ("result_bytes", C.c_uint64),
    ]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char_p), ("ms", C.c_float), ("launches", C.c_uint32), ("algorithmic_bytes", C.c_uint64),
                ("busy_ms", C.c_float), ("reserved", C.c_uint32)]


_lib = None


def load_library():
    """dlopen libvga_hip.so and declare the prototypes.  Raises if the extension has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.vga_ctx_create.argtypes = [C.c_int, _P(vp)]
    L.vga_ctx_destroy.argtypes = [vp]
    L.vga_last_error.argtypes = [vp]
    L.vga_last_error.restype = C.c_char_p
    L.vga_ctx_synchronize.argtypes = [vp]
    L.vga_index_upload.argtypes = [vp, _P(IndexDesc)]
    L.vga_batch_create.argtypes = [vp, C.c_char_p, _P(C.c_uint64), C.c_uint64, _P(vp)]
    L.vga_batch_destroy.argtypes = [vp]
    if hasattr(L, "vga_batch_strands"):  # (absent from an older build named by VGA_LIB; Batch.strands then fails)
        L.vga_batch_strands.argtypes = [vp, C.c_int, _P(C.c_char), _P(C.c_char)]
        L.vga_batch_strands.restype = C.c_int
    L.vga_map_default_params.argtypes = [_P(MapParams)]
    L.vga_map_batch.argtypes = [vp, _P(MapParams), _P(_P(MapResult))]
    L.vga_map_result_free.argtypes = [_P(MapResult)]
    L.vga_poa_default_params.argtypes = [_P(PoaParams)]
    L.vga_poa_result_free.argtypes = [_P(PoaResult)]
    L.vga_poa_batch.argtypes = [vp, C.c_uint64, _P(C.c_uint64), _P(C.c_uint64), C.c_char_p, _P(C.c_uint64),
                                _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint64), C.c_char_p, _P(PoaParams),
                                _P(_P(PoaResult))]
    L.vga_align_batch.argtypes = [vp, _P(MapResult), C.c_uint32, _P(PoaParams), _P(_P(AlignResult))]
    L.vga_align_result_free.argtypes = [_P(AlignResult)]
    L.vga_last_kernel_times.argtypes = [vp, _P(KernelTime), C.c_int]
    L.vga_chain_paths_text.argtypes = [vp, _P(MapResult), _P(_P(ChainText))]
    L.vga_align_prepare.argtypes = [vp, C.c_uint64, C.c_uint32]
    L.vga_align_prepare.restype = C.c_int
    L.vga_ctx_set_pool_fraction.argtypes = [vp, C.c_double]
    L.vga_ctx_set_pool_fraction.restype = C.c_int
    L.vga_ctx_set_host_threads.argtypes = [vp, C.c_uint32]
    L.vga_ctx_set_host_threads.restype = C.c_int
    L.vga_chain_text_free.argtypes = [_P(ChainText)]
    L.vga_index_build_kmers.argtypes = [vp, _P(IndexDesc), C.c_uint64, C.c_uint64]
    L.vga_index_build_kmers.restype = C.c_int
    L.vga_index_kmers_free.argtypes = [_P(IndexDesc)]
    L.vga_index_kmers_free.restype = None
    if hasattr(L, "vga_coverage_begin"):  # (absent from an older build named by VGA_LIB; the Context.coverage_* calls then fail)
        for name in ("vga_coverage_begin", "vga_coverage_reset", "vga_coverage_end"):
            getattr(L, name).argtypes = [vp]
            getattr(L, name).restype = C.c_int
        L.vga_coverage_read.argtypes = [vp, _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint32), _P(C.c_uint64)]
        L.vga_coverage_read.restype = C.c_int
    if hasattr(L, "vga_path_support_begin"):  # (absent from an older build named by VGA_LIB; the Context.path_support_* calls then fail)
        u64p, u32p = _P(C.c_uint64), _P(C.c_uint32)
        L.vga_path_support_begin.argtypes = [vp, C.c_uint32, u64p, u64p, u64p]
        L.vga_path_support_read.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, u64p]
        L.vga_path_support_last.argtypes = [vp, C.c_uint64, u32p, u32p]
        L.vga_path_support_reset.argtypes = [vp]
        L.vga_path_support_end.argtypes = [vp]
        L.vga_path_support_lists.argtypes = [vp, C.c_uint64, u64p, u32p, u32p, u32p, u32p]
        for name in ABI_SYMBOLS:
            if name.startswith("vga_path_support_"):
                getattr(L, name).restype = C.c_int
    if hasattr(L, "vga_pileup_begin"):  # (absent from an older build named by VGA_LIB; the Context.pileup* calls then fail)
        for name in ("vga_pileup_begin", "vga_pileup_reset", "vga_pileup_end"):
            getattr(L, name).argtypes = [vp]
            getattr(L, name).restype = C.c_int
        L.vga_pileup_read.argtypes = [vp, _P(C.c_uint32), _P(C.c_uint64), _P(C.c_uint64)]
        L.vga_pileup_read.restype = C.c_int
    if hasattr(L, "vga_genotype_begin"):  # (absent from an older build named by VGA_LIB; the Context.genotype* calls then fail)
        u64p, u32p = _P(C.c_uint64), _P(C.c_uint32)
        for name in ("vga_genotype_begin", "vga_genotype_reset", "vga_genotype_end"):
            getattr(L, name).argtypes = [vp]
            getattr(L, name).restype = C.c_int
        L.vga_genotype_read.argtypes = [vp, C.c_uint64, u64p, u64p, u64p, u64p]
        L.vga_genotype_read.restype = C.c_int
        L.vga_genotype_pairs.argtypes = [vp, C.c_uint64, C.c_uint32, u32p, u32p, u64p, u64p, u64p, u64p]
        L.vga_genotype_pairs.restype = C.c_int
    if hasattr(L, "vga_genotype_lik_begin"):  # (absent from an older build named by VGA_LIB; the Context.genotype_likelihood* calls then fail)
        u64p, u32p = _P(C.c_uint64), _P(C.c_uint32)
        L.vga_genotype_lik_table.argtypes = [C.c_uint32, C.c_uint32, u32p]
        L.vga_genotype_lik_begin.argtypes = [vp, C.c_uint32, C.c_uint32]
        L.vga_genotype_lik_read.argtypes = [vp, C.c_uint64, u64p, u64p]
        L.vga_genotype_lik_reset.argtypes = [vp]
        L.vga_genotype_lik_end.argtypes = [vp]
        L.vga_genotype_lik_pairs.argtypes = [vp, C.c_uint64, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, _P(C.c_uint8), u64p, u64p]
        for name in ABI_SYMBOLS:
            if name.startswith("vga_genotype_lik_") and name != "vga_genotype_lik_source":  # (declared with path edit below)
                getattr(L, name).restype = C.c_int
    if hasattr(L, "vga_path_edit_begin"):  # (absent from an older build named by VGA_LIB; the Context.path_edit* calls then fail)
        u64p, u32p = _P(C.c_uint64), _P(C.c_uint32)
        for name in ("vga_path_edit_begin", "vga_path_edit_reset", "vga_path_edit_end"):
            getattr(L, name).argtypes = [vp]
        L.vga_path_edit_read.argtypes = [vp, u64p, u64p, u64p, u64p, u64p, u64p]
        L.vga_path_edit_last.argtypes = [vp, C.c_uint64, u32p]
        L.vga_path_edit_pairs.argtypes = [vp, C.c_uint64, u64p, C.c_char_p, u64p, C.c_char_p, u32p]
        L.vga_genotype_lik_source.argtypes = [vp, C.c_uint32]
        L.vga_genotype_lik_source.restype = C.c_int
        for name in ABI_SYMBOLS:
            if name.startswith("vga_path_edit_"):
                getattr(L, name).restype = C.c_int
    if hasattr(L, "vga_variant_call"):  # (absent from an older build named by VGA_LIB; the Context.variant_call* calls then fail)
        u64p, u32p, u64 = _P(C.c_uint64), _P(C.c_uint32), C.c_uint64
        outs = [u64, u32p, _P(C.c_uint8), u32p, u64p, u64p, u64p, u64p, u64p]
        L.vga_variant_call.argtypes = [vp, C.c_uint32, u64, u64] + outs
        L.vga_variant_call_table.argtypes = [vp, u64, u64p, C.c_char_p, C.c_uint32, u64, u64] + outs
        L.vga_variant_call.restype = L.vga_variant_call_table.restype = C.c_int
    if hasattr(L, "vga_insertion_begin"):  # (absent from an older build named by VGA_LIB; the Context.insertion* calls then fail)
        u64p, u32p, u8p, u64 = _P(C.c_uint64), _P(C.c_uint32), _P(C.c_uint8), C.c_uint64
        for name in ("vga_insertion_begin", "vga_insertion_reset", "vga_insertion_end"):
            getattr(L, name).argtypes = [vp]
        L.vga_insertion_read.argtypes = [vp, u32p, u64p, u64p, u64p]
        outs = [u8p, u64p, u8p, u64p, u64p]
        L.vga_insertion_call.argtypes = [vp, u64, u32p] + outs
        L.vga_insertion_call_table.argtypes = [vp, u64, u64p] + outs
        for name in ABI_SYMBOLS:
            if name.startswith("vga_insertion_"):
                getattr(L, name).restype = C.c_int
    if hasattr(L, "vga_deletion_begin"):  # (absent from an older build named by VGA_LIB; the Context.deletion* calls then fail)
        u64p, u32p, u8p, u64 = _P(C.c_uint64), _P(C.c_uint32), _P(C.c_uint8), C.c_uint64
        for name in ("vga_deletion_begin", "vga_deletion_reset", "vga_deletion_end"):
            getattr(L, name).argtypes = [vp]
        L.vga_deletion_read.argtypes = [vp, u32p, u64p, u64p, u64p]
        outs = [u64, u32p, u32p, u32p, u8p, u32p, u64p, u64p, u64p, u64p]
        L.vga_deletion_call.argtypes = [vp, C.c_uint32, u64, u64] + outs
        L.vga_deletion_call_table.argtypes = [vp, u64, u32p, u64, u64p, C.c_uint32, u64, u64] + outs
        L.vga_deletion_state.argtypes = [u64, u64, C.c_uint32, u32p]
        for name in ABI_SYMBOLS:
            if name.startswith("vga_deletion_"):
                getattr(L, name).restype = C.c_int
        L.vga_deletion_state.restype = C.c_uint32
    if hasattr(L, "vga_phase_begin"):  # (absent from an older build named by VGA_LIB; the Context.phase* calls then fail)
        u64p, u32p, u8p, u64 = _P(C.c_uint64), _P(C.c_uint32), _P(C.c_uint8), C.c_uint64
        for name in ("vga_phase_begin", "vga_phase_reset", "vga_phase_end"):
            getattr(L, name).argtypes = [vp]
        L.vga_phase_read.argtypes = [vp, u32p, u32p, u64p, u64p]
        L.vga_phase_links.argtypes = [vp, u64, u32p, u8p, u8p, u32p, u32p, u64p]
        L.vga_phase_links_lists.argtypes = [vp, u64, u64, u32p, u64, u32p, u64, u32p, u8p, u8p, u8p, u32p, u32p]
        L.vga_phase_chain.argtypes = [u64, u32p, C.c_uint32, u32p, u8p, u8p]
        if hasattr(L, "vga_phase_tags"):  # (the haplotype tags came later than the links)
            L.vga_phase_tags.argtypes = [vp, u64, u32p, u8p, u8p, u32p, u8p, u64, u32p, u64p, u64p]
            L.vga_phase_tags_lists.argtypes = [vp, u64, u64, u32p, u64, u32p, u64, u32p, u8p, u8p, u8p, u32p, u8p, u64, u32p, u64p]
        if hasattr(L, "vga_haplotype_counts"):  # (the haplotype counts came later than the tags)
            L.vga_haplotype_counts.argtypes = [vp, u64, u32p, u64, u32p, u8p, u8p, u32p, u8p, u64, u32p, u64p, u64p]
            L.vga_haplotype_counts_lists.argtypes = [vp, u64, u64, u32p, u64, u32p, u64, u32p, u8p, u64, u32p, u8p, u8p, u8p, u32p, u8p, u64, u32p, u64p]
            L.vga_haplotype_jobs.argtypes = [u64, u32p, u64, u32p, u32p, u64, u32p, u64p]
            L.vga_haplotype_call.argtypes = [u32p, C.c_char_p]
        if hasattr(L, "vga_phase_set_links"):  # (the set links came later than the haplotype counts)
            L.vga_phase_set_links.argtypes = [vp, u64, u32p, u8p, u8p, u32p, u8p, u64, u32p, u64p, u64p]
            L.vga_phase_set_links_lists.argtypes = [vp, u64, u64, u32p, u64, u32p, u64, u32p, u8p, u8p, u8p, u32p, u8p, u64, u32p, u64p]
            L.vga_phase_join.argtypes = [u64, u32p, C.c_uint32, u32p, u8p, u32p, u64p, u64p, u64p]
        if hasattr(L, "vga_haplotype_paths"):  # (the haplotype paths came later than the set links)
            L.vga_haplotype_paths_begin.argtypes = [vp, C.c_uint32, C.c_uint32]
            L.vga_haplotype_paths_end.argtypes = [vp]
            L.vga_haplotype_paths_store.argtypes = [vp, u8p, u8p, u64p, u32p]
            L.vga_haplotype_paths.argtypes = [vp, u64, u32p, u8p, u8p, u32p, u8p, u64, u64p, u64p, u64p, u64p]
            L.vga_haplotype_paths_lists.argtypes = [vp, u64, u64, u32p, u64, u32p, C.c_uint32, u8p, u8p, u64, u32p, u8p, u8p, u8p, u32p, u8p, u64, u64p, u64p, u64p]
            L.vga_haplotype_paths_rank.argtypes = [C.c_uint32, u64p, u32p, u32p]
        for name in ABI_SYMBOLS:
            if name.startswith(("vga_phase_", "vga_haplotype_")) and hasattr(L, name):
                getattr(L, name).restype = C.c_int
    if hasattr(L, "vga_path_abundance"):  # (absent from an older build named by VGA_LIB; the Context.path_abundance* calls then fail)
        u64p, u32p, u8p, u64, u32 = _P(C.c_uint64), _P(C.c_uint32), _P(C.c_uint8), C.c_uint64, C.c_uint32
        outs = [u32p, u64p, u64p, u64p, u32p, u32p]
        L.vga_path_abundance_table.argtypes = [u32, u32, u32p]
        L.vga_path_abundance_begin.argtypes = [vp, u32, u32]
        L.vga_path_abundance_reset.argtypes = [vp]
        L.vga_path_abundance_end.argtypes = [vp]
        L.vga_path_abundance_store.argtypes = [vp, u64, u8p, u8p, u64p]
        L.vga_path_abundance.argtypes = [vp, u32, u32, u32] + outs
        L.vga_path_abundance_rows.argtypes = [vp, u64, u32, u8p, u8p, u32, u32, u32] + outs
        for name in ABI_SYMBOLS:
            if name.startswith("vga_path_abundance"):
                getattr(L, name).restype = C.c_int
    _lib = L
    return L


def graph_desc(k: int, seq_fwd: bytes, node_seq_idx, node_edge_idx, node_edges_to, edges) -> IndexDesc:
    """an IndexDesc with the graph half filled and the k-mer half empty (the input of vga_index_build_kmers); the numpy
    arrays it points into are kept on the returned object"""
    a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (node_seq_idx, node_edge_idx, node_edges_to, edges)]
    d = IndexDesc()
    d._keep = (seq_fwd, a)
    d.kmer_length = k
    d.seq_length = len(seq_fwd)
    d.seq_fwd = seq_fwd
    d.n_nodes = len(a[0]) - 1
    d.node_seq_idx, d.node_edge_idx, d.node_edges_to = _u64p(a[0]), _u64p(a[1]), _u64p(a[2])
    d.n_edges = len(a[3])
    d.edges = _u64p(a[3])
    return d


def kmer_arrays(d: IndexDesc) -> dict:
    """numpy copies of the k-mer half of a vga_index_desc"""
    k, nk, npos = int(d.kmer_length), int(d.n_kmers), int(d.n_kmer_pos)
    tab = (np.ctypeslib.as_array(C.cast(d.kmer_pos_table, _P(C.c_uint8)), shape=(npos * C.sizeof(KmerPos),)).copy().view(KMERPOS_DTYPE)
           if npos else np.zeros(0, KMERPOS_DTYPE))
    return dict(kmer_keys=C.string_at(d.kmer_keys, nk * k) if nk else b"", kmer_starts=_np(d.kmer_starts, nk, np.uint64),
                kmer_pos_table=tab)


def index_kmers_free(d: IndexDesc) -> None:
    """vga_index_kmers_free: releases the k-mer half vga_index_build_kmers filled and zeroes it"""
    load_library().vga_index_kmers_free(C.byref(d))


GENOTYPE_FIELDS = ("sum_bases", "sum_edges", "prefer_a", "prefer_b")


def pair_count(n_paths):
    """P (P + 1) / 2: the pairs p <= q of a genotype table over n_paths paths"""
    return n_paths * (n_paths + 1) // 2


def pair_index(n_paths, p, q):
    """where the pair (p, q), p <= q < n_paths, sits in a genotype table: p P - p (p - 1) / 2 + (q - p), the upper triangle
    row-major (csrc/vga_pair_index.hpp).  Python integers, or numpy integer arrays (computed in 64 bits)."""
    if isinstance(p, np.ndarray) or isinstance(q, np.ndarray):
        p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    return p * n_paths - p * (p - 1) // 2 + (q - p)


def genotype_rank(table: dict, top: Optional[int] = None):
    """the pairs (p, q) of a genotype table (Context.genotype / genotype_pairs) from the best down: by sum_bases, then sum_edges,
    both descending, then the homozygous pair before a heterozygous one, then p, then q.  Pairs whose sums are (0, 0) are not
    ranked; an empty list is no call.  top: at most that many (None or 0: all)."""
    n = int(table["n_paths"])
    p, q = np.triu_indices(n)  # (row-major upper triangle: the table's own order)
    sb, se = np.asarray(table["sum_bases"], dtype=np.uint64), np.asarray(table["sum_edges"], dtype=np.uint64)
    keep = np.flatnonzero((sb != 0) | (se != 0))
    # np.lexsort: the last key is the primary one; descending through the complement, which keeps the 64 bits
    order = keep[np.lexsort((q[keep], p[keep], (p[keep] != q[keep]), ~se[keep], ~sb[keep]))]
    if top:
        order = order[:top]
    return [(int(p[i]), int(q[i])) for i in order]


def genotype_likelihood_table(lam: int = GENOTYPE_LIK_LAMBDA, cap: int = GENOTYPE_LIK_CAP) -> np.ndarray:
    """vga_genotype_lik_table -> T, uint32[cap + 1]: T[x] = round(256 (1 - log2(1 + 2^(-lam x / 256)))), the library's one
    definition (csrc/vga_genotype_lik.hpp); needs no context and no device"""
    if not (0 <= int(lam) < 1 << 32 and 0 <= int(cap) < 1 << 32):
        raise VgaError(-1, "genotype_likelihood_table: lam %r, cap %r" % (lam, cap))
    t = np.zeros(int(cap) + 1 if 0 < int(cap) <= GENOTYPE_LIK_MAX_CAP else 1, dtype=np.uint32)
    rc = load_library().vga_genotype_lik_table(int(lam), int(cap), _u32p(t))
    if rc != VGA_OK:
        raise VgaError(rc, "genotype_likelihood_table: lam %r is 1 to %d and cap %r 1 to %d" % (lam, GENOTYPE_LIK_MAX_LAMBDA, cap, GENOTYPE_LIK_MAX_CAP))
    return t


def phase_chain(links, min_links: int = PHASE_MIN_LINKS):
    """vga_phase_chain -> (ps uint32[H], flip uint8[H], link_d uint8[H]) from links[H, 8, 4]: the library's one definition of the
    chain rule (csrc/vga_phase.hpp); needs no context and no device"""
    ln = np.ascontiguousarray(links, dtype=np.uint32).reshape(-1, PHASE_WINDOW, 4)
    n = len(ln)
    if not 0 <= int(min_links) < 1 << 32:
        raise VgaError(-1, "phase_chain: min_links %r" % (min_links,))
    ps, flip, link_d = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint8), np.zeros(max(1, n), dtype=np.uint8)
    u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
    rc = load_library().vga_phase_chain(n, _u32p(ln if n else np.zeros(1, dtype=np.uint32)), int(min_links), _u32p(ps), u8(flip), u8(link_d))
    if rc != VGA_OK:
        raise VgaError(rc, "phase_chain: min_links %r is 1 to %d" % (min_links, PHASE_MAX_MIN_LINKS))
    return ps[:n], flip[:n], link_d[:n]


def phase_join(table, n_sets: int, min_reads: int = PHASE_JOIN_MIN_READS):
    """vga_phase_join -> (set_root uint32[S], set_flip uint8[S], joins[J, 4] uint32 (s, t, cis, trans), n_agree, n_conflict) from the
    table[S (S + 1) / 2, 4] of Context.phase_set_links: the library's one definition of the join rule (csrc/vga_phase_join.hpp);
    needs no context and no device"""
    n = int(n_sets)
    tb = np.ascontiguousarray(table, dtype=np.uint32).reshape(-1, PHASE_JOIN_COLS)
    if n < 0 or len(tb) != n * (n + 1) // 2:
        raise VgaError(-1, "phase_join: %d sets and %d rows" % (n, len(tb)))
    if not 0 <= int(min_reads) < 1 << 32:
        raise VgaError(-1, "phase_join: min_reads %r" % (min_reads,))
    root, flip, joins = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint8), np.zeros((max(1, n), PHASE_JOIN_COLS), dtype=np.uint32)
    n_joins, n_agree, n_conflict = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = load_library().vga_phase_join(n, _u32p(tb if n else np.zeros(4, dtype=np.uint32)), int(min_reads), _u32p(root), flip.ctypes.data_as(_P(C.c_uint8)),
                                       _u32p(joins), C.byref(n_joins), C.byref(n_agree), C.byref(n_conflict))
    if rc != VGA_OK:
        raise VgaError(rc, "phase_join: min_reads %r is 1 to %d, %d sets at most" % (min_reads, PHASE_JOIN_MAX_MIN_READS, PHASE_JOIN_MAX_SETS))
    return root[:n], flip[:n], joins[:n_joins.value], int(n_agree.value), int(n_conflict.value)


def haplotype_paths_rank(cost_best):
    """vga_haplotype_paths_rank -> (order uint32[n_paths], tied) from the entries cost_best[n_paths, 2] (cost, best) of one group of
    Context.haplotype_paths: the paths by cost ascending, then in P-line order, and the number that attain the minimum; the library's
    one definition of the rank rule (csrc/vga_hap_paths.hpp); needs no context and no device"""
    cb = np.ascontiguousarray(cost_best, dtype=np.uint64).reshape(-1, HAPLOTYPE_PATHS_COLS)
    n = len(cb)
    order, tied = np.zeros(max(1, n), dtype=np.uint32), C.c_uint32(0)
    rc = load_library().vga_haplotype_paths_rank(n, _u64p(cb if n else np.zeros(2, dtype=np.uint64)), _u32p(order), C.byref(tied))
    if rc != VGA_OK:
        raise VgaError(rc, "haplotype_paths_rank: %d paths (1 to %d)" % (n, HAPLOTYPE_PATHS_MAX_PATHS))
    return order[:n], int(tied.value)


def path_abundance_table(lam: int = PATH_ABUNDANCE_LAMBDA, cap: int = PATH_ABUNDANCE_CAP) -> np.ndarray:
    """vga_path_abundance_table -> W, uint32[256]: W[d] = max(1, floor(65536 2^(-lam d / 256) + 0.5)) for d <= cap, non-increasing,
    the entries past cap repeating W[cap]; the library's one definition (csrc/vga_abundance.hpp); needs no context and no device"""
    if not (0 <= int(lam) < 1 << 32 and 0 <= int(cap) < 1 << 32):
        raise VgaError(-1, "path_abundance_table: lam %r, cap %r" % (lam, cap))
    w = np.zeros(256, dtype=np.uint32)
    rc = load_library().vga_path_abundance_table(int(lam), int(cap), _u32p(w))
    if rc != 0:
        raise VgaError(rc, "path_abundance_table: lam %r is 1 to %d and cap %r 1 to %d" % (lam, PATH_ABUNDANCE_MAX_LAMBDA, cap, PATH_ABUNDANCE_MAX_CAP))
    return w


def path_abundance_ppm(theta):
    """parts per million of a theta (or an array of them): (theta * 1 000 000) >> 24, as csrc/vga_abundance.hpp defines it"""
    t = np.asarray(theta, dtype=np.uint64)
    out = (t * np.uint64(1000000)) >> np.uint64(PATH_ABUNDANCE_THETA_BITS)
    return int(out) if out.ndim == 0 else out


def haplotype_jobs(cpos, pos, ps):
    """vga_haplotype_jobs -> jobs[J, 2] uint32 (c, ps): a job for every call c (cpos ascending) and phase set whose sites span
    cpos[c], by c and then by ps; the library's one definition of the rule (csrc/vga_hapcall.hpp); needs no context and no device"""
    cp = np.ascontiguousarray(cpos, dtype=np.uint32).reshape(-1)
    at = np.ascontiguousarray(pos, dtype=np.uint32).reshape(-1)
    sets = np.ascontiguousarray(ps, dtype=np.uint32).reshape(-1)
    if len(sets) != len(at):
        raise VgaError(-1, "haplotype_jobs: %d sites and %d ps" % (len(at), len(sets)))
    pad = lambda a: a if len(a) else np.zeros(1, dtype=np.uint32)
    L, cap = load_library(), 0
    while True:
        jobs, n = np.zeros((max(1, cap), 2), dtype=np.uint32), C.c_uint64(0)
        rc = L.vga_haplotype_jobs(len(cp), _u32p(pad(cp)), len(at), _u32p(pad(at)), _u32p(pad(sets)), cap, _u32p(jobs), C.byref(n))
        if rc != VGA_OK:
            raise VgaError(rc, "haplotype_jobs: cpos and pos ascend strictly, ps[h] names the site that opens the set of h")
        if n.value <= cap:
            return jobs[:n.value]
        cap = int(n.value)


def haplotype_call(counts7) -> str:
    """vga_haplotype_call: the haploid call of one haplotype's seven counts (A C G T other del ins) -> "A" "C" "G" "T" "-" "?"
    or ".", with "+" behind it where more than half of the observing reads insert; the library's one definition"""
    n = np.ascontiguousarray(counts7, dtype=np.uint32).reshape(-1)
    if len(n) != 7:
        raise VgaError(-1, "haplotype_call: %d counts, not 7" % len(n))
    text = C.create_string_buffer(3)
    rc = load_library().vga_haplotype_call(_u32p(n), text)
    if rc != VGA_OK:
        raise VgaError(rc, "haplotype_call")
    return text.value.decode()


def genotype_likelihood_rank(cost, n_paths: int, top: Optional[int] = None):
    """the pairs of a cost table (Context.genotype_likelihood / genotype_likelihood_pairs) from the best down, as
    [(p, q, cost, margin)]: by cost ascending, then the homozygous pair before a heterozygous one, then p, then q; margin is the
    cost above the first pair's.  Whether there is a call at all is n_scored's to say (0: no call).  top: at most that many
    (None or 0: all)."""
    n = int(n_paths)
    c = np.asarray(cost, dtype=np.uint64)
    assert c.shape == (pair_count(n),)
    p, q = np.triu_indices(n)  # (row-major upper triangle: the table's own order)
    order = np.lexsort((q, p, p != q, c))  # np.lexsort: the last key is the primary one
    if top:
        order = order[:top]
    first = int(c[order[0]]) if len(order) else 0
    return [(int(p[i]), int(q[i]), int(c[i]), int(c[i]) - first) for i in order]


def _np(ptr, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


def _u64p(a):
    return a.ctypes.data_as(_P(C.c_uint64))


def _u32p(a):
    return a.ctypes.data_as(_P(C.c_uint32))


def default_map_params() -> MapParams:
    p = MapParams()
    load_library().vga_map_default_params(C.byref(p))
    return p


def default_poa_params() -> PoaParams:
    p = PoaParams()
    load_library().vga_poa_default_params(C.byref(p))
    return p


class MapOut:
    """Host copy of a vga_map_result (numpy arrays) that also keeps the C object alive for vga_align_batch."""

    def __init__(self, L, ptr):
        self._L, self._ptr = L, ptr
        r = ptr.contents
        R, A, nc = int(r.n_reads), int(r.n_anchors), int(r.n_chains)
        self.n_reads, self.n_anchors, self.n_chains = R, A, nc
        self.anchor_off = _np(r.anchor_off, R + 1, np.uint64)
        self.anchor_id = _np(r.anchor_id, A, np.uint32) if r.anchor_id else None  # None with emit_dp = 0
        self.query_begin = _np(r.query_begin, A, np.uint32)
        self.target_begin = _np(r.target_begin, A, np.uint32)
        self.target_end = _np(r.target_end, A, np.uint32)
        self.max_chain_score = _np(r.max_chain_score, A, np.float64) if r.max_chain_score else None
        self.best_pred_id = _np(r.best_pred_id, A, np.int32) if r.best_pred_id else None
        self.curr_max = _np(r.curr_max, R, np.float64)
        self.chain_off = _np(r.chain_off, R + 1, np.uint64)
        self.chain_placeholder = _np(r.chain_placeholder, nc, np.uint8)
        self.chain_anchor_off = _np(r.chain_anchor_off, nc + 1, np.uint64)
        self.chain_anchor_idx = _np(r.chain_anchor_idx, int(self.chain_anchor_off[-1]) if nc else 0, np.uint32)
        self.ms = {"probe": r.ms_probe, "sort": r.ms_sort, "chain": r.ms_chain, "total": r.ms_total}
        self.n_hits = int(r.n_hits)
        # per read 0 (+) / 1 (-: the fields above describe its reverse complement) with VGA_STRANDS_BOTH, else None
        self.strand = _np(r.strand, R, np.uint8) if r.strand else None

    def chains_of(self, read: int):
        """[(is_placeholder, [sorted-anchor index, ...]), ...] for one read"""
        out = []
        for c in range(int(self.chain_off[read]), int(self.chain_off[read + 1])):
            s, e = int(self.chain_anchor_off[c]), int(self.chain_anchor_off[c + 1])
            out.append((bool(self.chain_placeholder[c]), self.chain_anchor_idx[s:e].tolist()))
        return out

    def close(self):
        if self._ptr is not None:
            self._L.vga_map_result_free(self._ptr)
            self._ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoaOut:
    def __init__(self, L, ptr):
        r = ptr.contents
        n = int(r.n)
        self.n = n
        self.ok = _np(r.ok, n, np.uint8)
        self.best_score = _np(r.best_score, n, np.int32)
        self.path_off = _np(r.path_off, n + 1, np.uint64)
        tp = int(self.path_off[-1])
        self.abpoa_nodes = _np(r.abpoa_nodes, tp, np.uint32)
        self.graph_nodes = _np(r.graph_nodes, tp, np.uint32)
        self.aln_start_offset = _np(r.aln_start_offset, n, np.uint32)
        self.aln_end_offset = _np(r.aln_end_offset, n, np.uint32)
        self.n_aligned_bases = _np(r.n_aligned_bases, n, np.uint32)
        self.cigar_off = _np(r.cigar_off, n + 1, np.uint64)
        self.cs_off = _np(r.cs_off, n + 1, np.uint64)
        cig = C.string_at(r.cigar, int(self.cigar_off[-1])) if n else b""
        cs = C.string_at(r.cs, int(self.cs_off[-1])) if n else b""
        self.cigar = [cig[int(self.cigar_off[i]):int(self.cigar_off[i + 1]) - 1].decode() for i in range(n)]
        self.cs = [cs[int(self.cs_off[i]):int(self.cs_off[i + 1]) - 1].decode() for i in range(n)]
        self.n_rows = _np(r.n_rows, n, np.uint64)
        self.n_cells = _np(r.n_cells, n, np.uint64)
        self.n_value_cells = _np(r.n_value_cells, n, np.uint64)
        self.ms = {"dp": r.ms_dp, "traceback": r.ms_traceback, "total": r.ms_total}
        L.vga_poa_result_free(ptr)


class AlignOut:
    def __init__(self, L, ptr):
        r = ptr.contents
        R = int(r.n_reads)
        self.n_reads = R
        self.aligned = _np(r.aligned, R, np.uint8)
        self.path_off = _np(r.path_off, R + 1, np.uint64)
        self.path_handles = _np(r.path_handles, int(self.path_off[-1]), np.uint64)
        self.path_length = _np(r.path_length, R, np.uint32)
        self.path_start = _np(r.path_start, R, np.uint32)
        self.path_end = _np(r.path_end, R, np.uint32)
        self.block_length = _np(r.block_length, R, np.uint32)
        self.best_score = _np(r.best_score, R, np.int32)
        self.cigar_off = _np(r.cigar_off, R + 1, np.uint64)
        self.cs_off = _np(r.cs_off, R + 1, np.uint64)
        cig = C.string_at(r.cigar, int(self.cigar_off[-1])) if R else b""
        cs = C.string_at(r.cs, int(self.cs_off[-1])) if R else b""
        self.cigar = [cig[int(self.cigar_off[i]):int(self.cigar_off[i + 1]) - 1].decode() for i in range(R)]
        self.cs = [cs[int(self.cs_off[i]):int(self.cs_off[i + 1]) - 1].decode() for i in range(R)]
        self.poa_rows, self.poa_cells, self.poa_problems = int(r.poa_rows), int(r.poa_cells), int(r.poa_problems)
        self.poa_value_cells = int(r.poa_value_cells)
        self.ms = {"subgraph": r.ms_subgraph, "dp": r.ms_dp, "traceback": r.ms_traceback, "total": r.ms_total}
        L.vga_align_result_free(ptr)


class Batch:
    def __init__(self, ctx: "Context", seqs: Sequence):
        """seqs: str (ASCII) or bytes, which may hold any byte value"""
        self.ctx = ctx
        L = ctx.L
        self.seqs = list(seqs)
        raw = [s if isinstance(s, (bytes, bytearray)) else s.encode() for s in self.seqs]
        self._concat = b"".join(raw)
        off = np.zeros(len(self.seqs) + 1, dtype=np.uint64)
        if self.seqs:
            off[1:] = np.cumsum([len(s) for s in raw], dtype=np.uint64)
        self._off = off
        h = C.c_void_p()
        ctx._check(L.vga_batch_create(ctx.h, self._concat, _u64p(off), len(self.seqs), C.byref(h)))
        self.h = h

    def strands(self, from_host: bool = False):
        """vga_batch_strands, the kernel seam of the reverse complement -> (forward, reverse): the two halves of the batch as
        the map and align kernels read them, read r at its offset in both; the device's copy, or the host's with from_host"""
        n = len(self._concat)
        fwd, rev = C.create_string_buffer(max(1, n)), C.create_string_buffer(max(1, n))
        self.ctx._check(self.ctx.L.vga_batch_strands(self.h, 1 if from_host else 0, fwd, rev))
        return fwd.raw[:n], rev.raw[:n]

    def map(self, params: Optional[MapParams] = None) -> MapOut:
        L = self.ctx.L
        p = params or default_map_params()
        out = _P(MapResult)()
        self.ctx._check(L.vga_map_batch(self.h, C.byref(p), C.byref(out)))
        return MapOut(L, out)

    def align(self, chains: MapOut, best_n: int = 1, params: Optional[PoaParams] = None) -> AlignOut:
        L = self.ctx.L
        p = params or default_poa_params()
        out = _P(AlignResult)()
        self.ctx._check(L.vga_align_batch(self.h, chains._ptr, best_n, C.byref(p), C.byref(out)))
        self.ctx._last_reads = len(self.seqs)
        return AlignOut(L, out)

    def map_raw(self, map_params: Optional[MapParams] = None, on_results=None) -> dict:
        """One map-only pass (anchors + chains; BASELINE config #2) without numpy conversion.  Counters only;
        on_results(map_result, None), when given, sees the C result before it is freed (bench.py --dump-outputs)."""
        L = self.ctx.L
        mp = map_params
        if mp is None:
            mp = default_map_params()
            mp.emit_dp = 0  # the chains GAF reads coordinates and chain membership only
        m = _P(MapResult)()
        self.ctx._check(L.vga_map_batch(self.h, C.byref(mp), C.byref(m)))
        try:
            q = m.contents
            if on_results is not None:
                on_results(q, None)
            R = int(q.n_reads)
            ph = np.ctypeslib.as_array(q.chain_placeholder, shape=(int(q.n_chains),)) if int(q.n_chains) else np.zeros(0, np.uint8)
            co = np.ctypeslib.as_array(q.chain_off, shape=(R + 1,)) if R else np.zeros(1, np.uint64)
            # a read is mapped when its first chain is a real one
            mapped = int((ph[co[:-1].astype(np.int64)] == 0).sum()) if R else 0
            return dict(n_reads=R, aligned=mapped, n_anchors=int(q.n_anchors), n_hits=int(q.n_hits), n_chains=int(q.n_chains),
                        ms_map=float(q.ms_total), ms_probe=float(q.ms_probe), ms_sort=float(q.ms_sort), ms_chain=float(q.ms_chain),
                        kernels=self.ctx.kernel_times())
        finally:
            L.vga_map_result_free(m)

    def map_align_raw(self, map_params: Optional[MapParams] = None, best_n: int = 1,
                      poa_params: Optional[PoaParams] = None, on_results=None) -> dict:
        """One pass of the whole hot path without converting the results to numpy (bench.py's timed step).
        Returns counters only; on_results(map_result, align_result), when given, sees the C results before they are
        freed (bench.py --dump-outputs)."""
        import time as _t
        L = self.ctx.L
        mp = map_params
        if mp is None:
            mp = default_map_params()
            mp.emit_dp = 0  # nothing downstream of the chains reads ids / f(i) / predecessors
        pp = poa_params or default_poa_params()
        m = _P(MapResult)()
        t0 = _t.perf_counter()
        self.ctx._check(L.vga_map_batch(self.h, C.byref(mp), C.byref(m)))
        t1 = _t.perf_counter()
        kt_map = self.ctx.kernel_times()
        try:
            a = _P(AlignResult)()
            self.ctx._check(L.vga_align_batch(self.h, m, best_n, C.byref(pp), C.byref(a)))
            self.ctx._last_reads = len(self.seqs)
            t2 = _t.perf_counter()
            kt_aln = self.ctx.kernel_times()
            r, q = a.contents, m.contents
            R = int(r.n_reads)
            aligned = int(np.ctypeslib.as_array(r.aligned, shape=(R,)).sum()) if R else 0
            out = dict(n_reads=R, aligned=aligned, n_anchors=int(q.n_anchors), n_hits=int(q.n_hits),
                       poa_rows=int(r.poa_rows), poa_cells=int(r.poa_cells), poa_value_cells=int(r.poa_value_cells),
                       poa_problems=int(r.poa_problems), path_bases=int(np.ctypeslib.as_array(r.path_length, shape=(R,)).sum()) if R else 0,
                       cigar_bytes=int(r.cigar_off[R]) if R else 0, result_bytes=int(r.result_bytes),
                       ms_map=float(q.ms_total), ms_probe=float(q.ms_probe), ms_sort=float(q.ms_sort), ms_chain=float(q.ms_chain),
                       ms_align=float(r.ms_total), ms_subgraph=float(r.ms_subgraph), ms_dp_summed_launches=float(r.ms_dp),
                       ms_traceback=float(r.ms_traceback), kernels=kt_map + kt_aln)
            if on_results is not None:
                on_results(q, r)
            t3 = _t.perf_counter()
            L.vga_align_result_free(a)
        finally:
            L.vga_map_result_free(m)
        t4 = _t.perf_counter()
        out["ms_wall_map_call"] = (t1 - t0) * 1e3
        out["ms_wall_align_call"] = (t2 - t1) * 1e3
        out["ms_wall_free"] = (t4 - t3) * 1e3
        return out

    def close(self):
        if self.h:
            self.ctx.L.vga_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One vga_ctx (one GPU)."""

    def __init__(self, device: int = 0):
        self.L = load_library()
        h = C.c_void_p()
        rc = self.L.vga_ctx_create(device, C.byref(h))
        if rc != VGA_OK:
            raise VgaError(rc, f"vga_ctx_create(device={device}) failed: no usable MI355X; this library has no CPU path")
        self.h = h
        self._keep = None
        self._dims = None  # (seq_length, n_nodes, n_edges) of the index this context holds
        self._n_paths = 0  # paths of the last path_support_begin
        self._last_reads = 0  # reads of the last Batch.align

    def _check(self, rc: int):
        if rc != VGA_OK:
            raise VgaError(rc, self.L.vga_last_error(self.h).decode())

    def set_pool_fraction(self, fraction: float):
        """share of the device's free memory this context's traceback pool may take (contexts that share a GPU)"""
        self._check(self.L.vga_ctx_set_pool_fraction(self.h, float(fraction)))

    def set_host_threads(self, n: int):
        """host threads this context's calls fan out to (0: the default)"""
        self._check(self.L.vga_ctx_set_host_threads(self.h, int(n)))

    def upload_index(self, k: int, seq_fwd: bytes, node_seq_idx, node_edge_idx, node_edges_to, edges, kmer_keys: bytes,
                     kmer_starts, kmer_pos_table: np.ndarray):
        """kmer_pos_table: structured array with KMERPOS_DTYPE (records incl. delimiters)."""
        a = [np.ascontiguousarray(x, dtype=np.uint64) for x in (node_seq_idx, node_edge_idx, node_edges_to, edges, kmer_starts)]
        tab = np.ascontiguousarray(kmer_pos_table)
        assert tab.dtype.itemsize == C.sizeof(KmerPos)
        d = IndexDesc()
        d.kmer_length = k
        d.seq_length = len(seq_fwd)
        d.seq_fwd = seq_fwd
        d.n_nodes = len(a[0]) - 1
        d.node_seq_idx, d.node_edge_idx, d.node_edges_to = _u64p(a[0]), _u64p(a[1]), _u64p(a[2])
        d.n_edges = len(a[3])
        d.edges = _u64p(a[3])
        d.n_kmers = len(a[4])
        d.kmer_keys = kmer_keys
        d.kmer_starts = _u64p(a[4])
        d.n_kmer_pos = len(tab)
        d.kmer_pos_table = tab.ctypes.data_as(_P(KmerPos))
        self._dims = None
        self._check(self.L.vga_index_upload(self.h, C.byref(d)))
        self._dims = (int(d.seq_length), int(d.n_nodes), int(d.n_edges))

    def index_build_kmers(self, desc: IndexDesc, max_furcations: int = 100, max_degree: int = 100) -> None:
        """vga_index_build_kmers: fills the k-mer half of `desc` (release it with index_kmers_free) and leaves this
        context holding the index"""
        self._dims = None
        self._check(self.L.vga_index_build_kmers(self.h, C.byref(desc), int(max_furcations), int(max_degree)))
        self._dims = (int(desc.seq_length), int(desc.n_nodes), int(desc.n_edges))

    def batch(self, seqs: Sequence[str]) -> Batch:
        return Batch(self, seqs)

    def poa_batch(self, problems, params: Optional[PoaParams] = None) -> PoaOut:
        """problems: [(node strings, [(src, dst), ...], query), ...] -- the create_align_safe arguments."""
        p = params or default_poa_params()
        n = len(problems)
        node_ptr = np.zeros(n + 1, dtype=np.uint64)
        edge_ptr = np.zeros(n + 1, dtype=np.uint64)
        query_off = np.zeros(n + 1, dtype=np.uint64)
        node_off: List[int] = []
        chunks: List[str] = []
        es: List[int] = []
        ed: List[int] = []
        qs: List[str] = []
        pos = 0
        for i, (nodes, edges, query) in enumerate(problems):
            node_ptr[i] = len(node_off)
            for s in nodes:
                node_off.append(pos)
                pos += len(s)
            chunks.extend(nodes)
            edge_ptr[i] = len(es)
            es.extend(e[0] for e in edges)
            ed.extend(e[1] for e in edges)
            query_off[i + 1] = query_off[i] + len(query)
            qs.append(query)
        node_ptr[n] = len(node_off)
        edge_ptr[n] = len(es)
        node_off.append(pos)
        noff = np.asarray(node_off, dtype=np.uint64)
        esa = np.asarray(es if es else [0], dtype=np.uint32)
        eda = np.asarray(ed if ed else [0], dtype=np.uint32)
        out = _P(PoaResult)()
        self._check(self.L.vga_poa_batch(self.h, n, _u64p(node_ptr), _u64p(noff), "".join(chunks).encode(), _u64p(edge_ptr),
                                         _u32p(esa), _u32p(eda), _u64p(query_off), "".join(qs).encode(), C.byref(p),
                                         C.byref(out)))
        return PoaOut(self.L, out)

    def align_prepare(self, n_reads: int, max_read_len: int) -> None:
        """vga_align_prepare: start allocating what the first align_batch of this context will need (returns at once)"""
        self._check(self.L.vga_align_prepare(self.h, int(n_reads), int(max_read_len)))

    def coverage_begin(self) -> None:
        """vga_coverage_begin: from now on every align() of this context adds its reported alignments to the coverage tables"""
        self._check(self.L.vga_coverage_begin(self.h))

    def coverage(self):
        """vga_coverage_read -> (base_depth[seq_length], node_reads[n_nodes], edge_reads[n_edges], n_alignments); does not reset"""
        sl, nn, ne = self._dims if self._dims else (0, 0, 0)
        base, node, edge = (np.zeros(max(1, x), dtype=np.uint32) for x in (sl, nn, ne))
        n = C.c_uint64(0)
        self._check(self.L.vga_coverage_read(self.h, _u32p(base), _u32p(node), _u32p(edge), C.byref(n)))
        return base[:sl], node[:nn], edge[:ne], int(n.value)

    def coverage_reset(self) -> None:
        """vga_coverage_reset: zero the tables, keep counting"""
        self._check(self.L.vga_coverage_reset(self.h))

    def coverage_end(self) -> None:
        """vga_coverage_end: free the tables, stop counting"""
        self._check(self.L.vga_coverage_end(self.h))

    def pileup_begin(self) -> None:
        """vga_pileup_begin: from now on every align() of this context adds its reported alignments to the pileup table"""
        self._check(self.L.vga_pileup_begin(self.h))

    def pileup(self):
        """vga_pileup_read -> (counts[seq_length, 7] in the column order PILEUP_COLUMNS, n_alignments, leading_ins); does not reset"""
        sl = self._dims[0] if self._dims else 0
        counts = np.zeros((max(1, sl), len(PILEUP_COLUMNS)), dtype=np.uint32)
        n, lead = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_pileup_read(self.h, _u32p(counts), C.byref(n), C.byref(lead)))
        return counts[:sl], int(n.value), int(lead.value)

    def pileup_reset(self) -> None:
        """vga_pileup_reset: zero the table, keep counting"""
        self._check(self.L.vga_pileup_reset(self.h))

    def pileup_end(self) -> None:
        """vga_pileup_end: free the table, stop counting"""
        self._check(self.L.vga_pileup_end(self.h))

    def _variant(self, call, cap) -> dict:
        """`call(cap, *outs)` is one of the two C calls with everything before cap bound: asks again with a larger cap when the
        first answer holds more calls than it had room for"""
        cap = max(0, int(cap))
        while True:
            m = max(1, cap)
            pos, gt, qual = np.zeros(m, dtype=np.uint32), np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint32)
            insq, depth, rows = np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64), np.zeros((m, len(PILEUP_COLUMNS)), dtype=np.uint64)
            nt, nc = C.c_uint64(0), C.c_uint64(0)
            self._check(call(cap, _u32p(pos), gt.ctypes.data_as(_P(C.c_uint8)), _u32p(qual), _u64p(insq), _u64p(depth), _u64p(rows), C.byref(nt), C.byref(nc)))
            n = int(nc.value)
            if n <= cap:
                break
            cap = n
        return {"pos": pos[:n], "x": gt[:n] & 7, "y": (gt[:n] >> 3) & 7, "ins": gt[:n] >> 6, "qual": qual[:n], "ins_qual": insq[:n],
                "depth": depth[:n], "counts": rows[:n], "n_tested": int(nt.value), "n_calls": n}

    def variant_call(self, error: int = VARIANT_ERROR, min_depth: int = VARIANT_MIN_DEPTH, min_qual: int = VARIANT_MIN_QUAL, cap: int = 1024) -> dict:
        """vga_variant_call: the diploid call at every graph base from this context's pileup counters (needs pileup_begin; does
        not reset) -> {pos, x, y (alleles 0..4 = A C G T D), ins (0 none, 1 het, 2 hom), qual, ins_qual, depth, counts[n, 7]:
        arrays over the reported bases in base order, n_tested, n_calls}.  cap: the calls the first request has room for."""
        return self._variant(lambda c, *outs: self.L.vga_variant_call(self.h, int(error), int(min_depth), int(min_qual), c, *outs), cap)

    def variant_call_table(self, counts, letters, error: int = VARIANT_ERROR, min_depth: int = VARIANT_MIN_DEPTH, min_qual: int = VARIANT_MIN_QUAL,
                           cap: int = 1024) -> dict:
        """vga_variant_call_table, the kernel seam: the same call from an explicit table counts[n, 7] (uint64) and its n letters
        (str or bytes).  Needs a context only."""
        tab = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1, len(PILEUP_COLUMNS))
        let = letters.encode() if isinstance(letters, str) else bytes(letters)
        if len(let) != len(tab):
            raise ValueError(f"{len(tab)} rows and {len(let)} letters")
        return self._variant(lambda c, *outs: self.L.vga_variant_call_table(self.h, len(tab), _u64p(tab), let, int(error), int(min_depth), int(min_qual),
                                                                           c, *outs), cap)

    def insertion_begin(self) -> None:
        """vga_insertion_begin: from now on every align() of this context adds the insertions of its reported alignments to the
        table of inserted lengths and letters"""
        self._check(self.L.vga_insertion_begin(self.h))

    def insertions(self):
        """vga_insertion_read -> (counts[seq_length, INSERTION_COLS] uint32: per base the bins of length 1 .. 8 and more, then the
        letters A C G T N of each of the first 8 positions; n_alignments, n_events, n_leading); does not reset"""
        sl = self._dims[0] if self._dims else 0
        counts = np.zeros((max(1, sl), INSERTION_COLS), dtype=np.uint32)
        n, ev, lead = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_insertion_read(self.h, _u32p(counts), C.byref(n), C.byref(ev), C.byref(lead)))
        return counts[:sl], int(n.value), int(ev.value), int(lead.value)

    def insertion_reset(self) -> None:
        """vga_insertion_reset: zero the table, keep counting"""
        self._check(self.L.vga_insertion_reset(self.h))

    def insertion_end(self) -> None:
        """vga_insertion_end: free the table, stop counting"""
        self._check(self.L.vga_insertion_end(self.h))

    def _insertion(self, call, n) -> dict:
        """`call(*outs)` is one of the two C calls with everything before the outputs bound"""
        m = max(1, n)
        length, seq = np.zeros(m, dtype=np.uint8), np.zeros((m, INSERTION_MAX_LEN), dtype=np.uint8)
        lr, sr = np.zeros(m, dtype=np.uint64), np.zeros((m, INSERTION_MAX_LEN), dtype=np.uint64)
        rows = np.zeros((m, INSERTION_COLS), dtype=np.uint64)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        self._check(call(u8(length), _u64p(lr), u8(seq), _u64p(sr), _u64p(rows)))
        return {"length": length[:n], "length_reads": lr[:n], "seq": seq[:n], "seq_reads": sr[:n], "rows": rows[:n]}

    def insertion_call(self, pos) -> dict:
        """vga_insertion_call: length and letters of the insertion behind each of the graph bases `pos`, from this context's own
        counters (needs insertion_begin; does not reset) -> {length (0: none, 1 .. 8, 9: more than 8), length_reads, seq[n, 8]
        (the bytes of A C G T N, 0 behind the last), seq_reads[n, 8], rows[n, INSERTION_COLS]: the sites' counters}"""
        at = np.ascontiguousarray(pos, dtype=np.uint32).reshape(-1)
        return self._insertion(lambda *outs: self.L.vga_insertion_call(self.h, len(at), _u32p(at if len(at) else np.zeros(1, dtype=np.uint32)), *outs), len(at))

    def insertion_call_table(self, rows) -> dict:
        """vga_insertion_call_table, the kernel seam: the same call from explicit rows[n, INSERTION_COLS] (uint64).  Needs a
        context only."""
        tab = np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1, INSERTION_COLS)
        return self._insertion(lambda *outs: self.L.vga_insertion_call_table(self.h, len(tab), _u64p(tab if len(tab) else np.zeros((1, INSERTION_COLS), dtype=np.uint64)),
                                                                             *outs), len(tab))

    def deletion_begin(self) -> None:
        """vga_deletion_begin: from now on every align() of this context appends the deletion events of its reported alignments to
        the context's store (needs pileup_begin)"""
        self._check(self.L.vga_deletion_begin(self.h))

    def deletions(self):
        """vga_deletion_read -> (events[n_events, 3] uint32: first, len, last, in the order of the reported alignments and along
        each; n_alignments, n_end_runs); does not reset"""
        n, ev, ends = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_deletion_read(self.h, None, C.byref(n), C.byref(ev), C.byref(ends)))
        events = np.zeros((max(1, int(ev.value)), DELETION_EVENT_WORDS), dtype=np.uint32)
        self._check(self.L.vga_deletion_read(self.h, _u32p(events), C.byref(n), C.byref(ev), C.byref(ends)))
        return events[:int(ev.value)], int(n.value), int(ends.value)

    def deletion_reset(self) -> None:
        """vga_deletion_reset: empty the store, keep storing"""
        self._check(self.L.vga_deletion_reset(self.h))

    def deletion_end(self) -> None:
        """vga_deletion_end: free the store, stop storing"""
        self._check(self.L.vga_deletion_end(self.h))

    def _deletion(self, call, cap, ask_again) -> dict:
        """`call(cap, *outs)` is one of the two C calls with everything before cap bound: asks again with a larger cap when the
        first answer holds more calls than it had room for (ask_again False: returns the first min(n_calls, cap) calls)"""
        cap = max(0, int(cap))
        while True:
            m = max(1, cap)
            first, length, last, qual = (np.zeros(m, dtype=np.uint32) for _ in range(4))
            state, depth, reads = np.zeros(m, dtype=np.uint8), np.zeros(m, dtype=np.uint64), np.zeros(m, dtype=np.uint64)
            nd, nc = C.c_uint64(0), C.c_uint64(0)
            self._check(call(cap, _u32p(first), _u32p(length), _u32p(last), state.ctypes.data_as(_P(C.c_uint8)), _u32p(qual), _u64p(depth), _u64p(reads),
                             C.byref(nd), C.byref(nc)))
            n = int(nc.value)
            if n <= cap or not ask_again:
                break
            cap = n
        k = min(n, cap)
        return {"first": first[:k], "len": length[:k], "last": last[:k], "state": state[:k], "qual": qual[:k], "depth": depth[:k], "reads": reads[:k],
                "n_distinct": int(nd.value), "n_calls": n}

    def deletion_call(self, error: int = VARIANT_ERROR, min_depth: int = VARIANT_MIN_DEPTH, min_qual: int = VARIANT_MIN_QUAL, cap: int = 1024,
                      ask_again: bool = True) -> dict:
        """vga_deletion_call: the events of this context's store sorted, grouped and called against its pileup counters (needs
        pileup_begin and deletion_begin; does not reset) -> {first, len, last, state (0 none, 1 het, 2 hom), qual, depth, reads:
        arrays over the reported groups in the order of (first, len, last); n_distinct, n_calls}.  cap: the calls the first request
        has room for."""
        return self._deletion(lambda c, *outs: self.L.vga_deletion_call(self.h, int(error), int(min_depth), int(min_qual), c, *outs), cap, ask_again)

    def deletion_call_table(self, events, counts, error: int = VARIANT_ERROR, min_depth: int = VARIANT_MIN_DEPTH, min_qual: int = VARIANT_MIN_QUAL,
                            cap: int = 1024, ask_again: bool = True) -> dict:
        """vga_deletion_call_table, the kernel seam: the same call from explicit events[n, 3] (uint32) and an explicit pileup table
        counts[n_bases, 7] (uint64).  Needs a context only."""
        ev = np.ascontiguousarray(events, dtype=np.uint32).reshape(-1, DELETION_EVENT_WORDS)
        tab = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1, len(PILEUP_COLUMNS))
        evp = _u32p(ev if len(ev) else np.zeros((1, DELETION_EVENT_WORDS), dtype=np.uint32))
        tabp = _u64p(tab if len(tab) else np.zeros((1, len(PILEUP_COLUMNS)), dtype=np.uint64))
        return self._deletion(lambda c, *outs: self.L.vga_deletion_call_table(self.h, len(ev), evp, len(tab), tabp, int(error), int(min_depth), int(min_qual),
                                                                             c, *outs), cap, ask_again)

    def phase_begin(self) -> None:
        """vga_phase_begin: from now on every align() of this context keeps the pileup lists of its reported alignments (needs
        pileup_begin)"""
        self._check(self.L.vga_phase_begin(self.h))

    def phase_reads(self):
        """vga_phase_read -> (recs[n_reads, 3] uint32: off, n_runs, n_sparse; words uint32): the store as phase_links_lists takes
        it; does not reset"""
        n, w = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_phase_read(self.h, None, None, C.byref(n), C.byref(w)))
        recs, words = np.zeros((max(1, n.value), 3), dtype=np.uint32), np.zeros(max(1, w.value), dtype=np.uint32)
        self._check(self.L.vga_phase_read(self.h, _u32p(recs), _u32p(words), C.byref(n), C.byref(w)))
        return recs[:n.value], words[:w.value]

    def phase_reset(self) -> None:
        """vga_phase_reset: empty the store, keep it on"""
        self._check(self.L.vga_phase_reset(self.h))

    def phase_end(self) -> None:
        """vga_phase_end: free the store, stop keeping"""
        self._check(self.L.vga_phase_end(self.h))

    @staticmethod
    def _phase_sites(pos, *alleles):
        at = np.ascontiguousarray(pos, dtype=np.uint32).reshape(-1)
        cols = [np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in alleles]
        if any(len(c) != len(at) for c in cols):
            raise VgaError(-1, "phase: %d sites and alleles of %s" % (len(at), [len(c) for c in cols]))
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        return len(at), pad(at), [pad(c) for c in cols]

    def phase_links(self, pos, x, y):
        """vga_phase_links: the links between the sites pos (ascending graph bases) with alleles x < y (0 .. 4 = A C G T D), from
        this context's own store -> (links[H, 8, 4] uint32, site_reads[H, 3] uint32, n_reads); does not reset"""
        n, at, (xs, ys) = self._phase_sites(pos, x, y)
        links, sr = np.zeros((max(1, n), PHASE_WINDOW, 4), dtype=np.uint32), np.zeros((max(1, n), 3), dtype=np.uint32)
        n_reads = C.c_uint64(0)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        self._check(self.L.vga_phase_links(self.h, n, _u32p(at), u8(xs), u8(ys), _u32p(links), _u32p(sr), C.byref(n_reads)))
        return links[:n], sr[:n], int(n_reads.value)

    def phase_links_lists(self, recs, words, n_bases, pos, x, y, ref):
        """vga_phase_links_lists, the kernel seam: the same from explicit records recs[n_reads, 3] and their words on a graph of
        n_bases bases; ref[h] is the own letter of site h (0 .. 3 = A C G T, 4 anything else) -> (links, site_reads).  Needs a
        context only."""
        rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
        wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        n, at, (xs, ys, rf) = self._phase_sites(pos, x, y, ref)
        links, sr = np.zeros((max(1, n), PHASE_WINDOW, 4), dtype=np.uint32), np.zeros((max(1, n), 3), dtype=np.uint32)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
        self._check(self.L.vga_phase_links_lists(self.h, int(n_bases), len(rc), _u32p(pad(rc)), len(wd), _u32p(pad(wd)), n, _u32p(at), u8(xs), u8(ys), u8(rf),
                                                 _u32p(links), _u32p(sr)))
        return links[:n], sr[:n]

    def _phase_tags(self, call, n, ps, flip, cap):
        """`call(ps, flip, cap, rows, n_rows)` is one of the two C calls with everything else bound: asked again with room for
        every row when the first answer holds more rows than it had room for"""
        sets = np.ascontiguousarray(ps, dtype=np.uint32).reshape(-1)
        fl = np.ascontiguousarray(flip, dtype=np.uint8).reshape(-1)
        if len(sets) != n or len(fl) != n:
            raise VgaError(-1, "phase tags: %d sites, %d ps and %d flip" % (n, len(sets), len(fl)))
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        cap = max(0, int(cap))
        while True:
            rows, n_rows = np.zeros((max(1, cap), PHASE_TAG_COLS), dtype=np.uint32), C.c_uint64(0)
            self._check(call(_u32p(pad(sets)), pad(fl).ctypes.data_as(_P(C.c_uint8)), cap, _u32p(rows), C.byref(n_rows)))
            if n_rows.value <= cap:
                return rows[:n_rows.value]
            cap = int(n_rows.value)

    def phase_tags(self, pos, x, y, ps, flip, cap: int = 1 << 16):
        """vga_phase_tags: which stored reads of this context go with which haplotype of which phase set, at the sites pos, x, y
        of phase_links under the ps and flip of phase_chain -> (rows[n, 4] uint32: read (index in the store), ps, votes_a,
        votes_b, in read order and then by ps; n_reads).  A read goes with a when votes_a > votes_b, with b when votes_b > votes_a.
        Does not reset."""
        n, at, (xs, ys) = self._phase_sites(pos, x, y)
        n_reads = C.c_uint64(0)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        rows = self._phase_tags(lambda sets, fl, cap, rows, n_rows: self.L.vga_phase_tags(self.h, n, _u32p(at), u8(xs), u8(ys), sets, fl, cap, rows, n_rows,
                                                                                       C.byref(n_reads)), n, ps, flip, cap)
        return rows, int(n_reads.value)

    def phase_tags_lists(self, recs, words, n_bases, pos, x, y, ref, ps, flip, cap: int = 1 << 16):
        """vga_phase_tags_lists, the kernel seam: the same from explicit records and words (phase_links_lists) -> rows[n, 4].
        Needs a context only."""
        rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
        wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        n, at, (xs, ys, rf) = self._phase_sites(pos, x, y, ref)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
        return self._phase_tags(lambda sets, fl, cap, rows, n_rows: self.L.vga_phase_tags_lists(self.h, int(n_bases), len(rc), _u32p(pad(rc)), len(wd), _u32p(pad(wd)),
                                                                                             n, _u32p(at), u8(xs), u8(ys), u8(rf), sets, fl, cap, rows, n_rows),
                                n, ps, flip, cap)

    def _haplotype_counts(self, call, n, ps, flip, cap):
        """`call(ps, flip, cap, rows, n_rows)` is one of the two C calls with everything else bound: asked again with room for
        every row when the first answer says there are more jobs than it had room for (nothing was counted then)"""
        sets = np.ascontiguousarray(ps, dtype=np.uint32).reshape(-1)
        fl = np.ascontiguousarray(flip, dtype=np.uint8).reshape(-1)
        if len(sets) != n or len(fl) != n:
            raise VgaError(-1, "haplotype counts: %d sites, %d ps and %d flip" % (n, len(sets), len(fl)))
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        cap = max(0, int(cap))
        while True:
            rows, n_rows = np.zeros((max(1, cap), HAPLOTYPE_ROW), dtype=np.uint32), C.c_uint64(0)
            self._check(call(_u32p(pad(sets)), pad(fl).ctypes.data_as(_P(C.c_uint8)), cap, _u32p(rows), C.byref(n_rows)))
            if n_rows.value <= cap:
                return rows[:n_rows.value]
            cap = int(n_rows.value)

    def haplotype_counts(self, cpos, pos, x, y, ps, flip, cap: Optional[int] = None):
        """vga_haplotype_counts: for every call cpos[c] (ascending graph bases) and phase set whose sites span it, what the stored
        reads of this context tagged a and those tagged b show there, at the sites pos, x, y of phase_links under the ps and flip of
        phase_chain -> (rows[J, 16] uint32: c, ps, a[A C G T other del ins], b[..], by c and then by ps; n_reads).  Does not reset."""
        cp = np.ascontiguousarray(cpos, dtype=np.uint32).reshape(-1)
        n, at, (xs, ys) = self._phase_sites(pos, x, y)
        n_reads = C.c_uint64(0)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
        rows = self._haplotype_counts(lambda sets, fl, cap, rows, n_rows: self.L.vga_haplotype_counts(self.h, len(cp), _u32p(pad(cp)), n, _u32p(at), u8(xs), u8(ys), sets,
                                                                                                     fl, cap, rows, n_rows, C.byref(n_reads)),
                                      n, ps, flip, 4 * len(cp) + 64 if cap is None else cap)
        return rows, int(n_reads.value)

    def haplotype_counts_lists(self, recs, words, n_bases, cpos, cref, pos, x, y, ref, ps, flip, cap: Optional[int] = None):
        """vga_haplotype_counts_lists, the kernel seam: the same from explicit records and words (phase_links_lists); cref[c] is the
        own letter of call c (0 .. 3 = A C G T, 4 anything else) -> rows[J, 16].  Needs a context only."""
        rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
        wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        cp = np.ascontiguousarray(cpos, dtype=np.uint32).reshape(-1)
        cr = np.ascontiguousarray(cref, dtype=np.uint8).reshape(-1)
        if len(cr) != len(cp):
            raise VgaError(-1, "haplotype counts: %d calls and %d own letters" % (len(cp), len(cr)))
        n, at, (xs, ys, rf) = self._phase_sites(pos, x, y, ref)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=a.dtype)
        return self._haplotype_counts(lambda sets, fl, cap, rows, n_rows: self.L.vga_haplotype_counts_lists(
            self.h, int(n_bases), len(rc), _u32p(pad(rc)), len(wd), _u32p(pad(wd)), len(cp), _u32p(pad(cp)), u8(pad(cr)), n, _u32p(at), u8(xs), u8(ys), u8(rf), sets,
            fl, cap, rows, n_rows), n, ps, flip, 4 * len(cp) + 64 if cap is None else cap)

    def _phase_set_links(self, call, n, ps, flip):
        """`call(ps, flip, cap_rows, table, n_sets)` is one of the two C calls with everything else bound: asked again with room for
        the whole table when the first answer names more sets than it had room for (nothing was counted then)"""
        sets = np.ascontiguousarray(ps, dtype=np.uint32).reshape(-1)
        fl = np.ascontiguousarray(flip, dtype=np.uint8).reshape(-1)
        if len(sets) != n or len(fl) != n:
            raise VgaError(-1, "phase set links: %d sites, %d ps and %d flip" % (n, len(sets), len(fl)))
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        cap = int((sets == np.arange(1, n + 1, dtype=np.uint32)).sum())
        cap = cap * (cap + 1) // 2
        while True:
            table, n_sets = np.zeros((max(1, cap), PHASE_JOIN_COLS), dtype=np.uint32), C.c_uint64(0)
            self._check(call(_u32p(pad(sets)), pad(fl).ctypes.data_as(_P(C.c_uint8)), cap, _u32p(table), C.byref(n_sets)))
            rows = n_sets.value * (n_sets.value + 1) // 2
            if rows <= cap:
                return table[:rows], int(n_sets.value)
            cap = rows

    def phase_set_links(self, pos, x, y, ps, flip):
        """vga_phase_set_links: for every pair of phase sets s <= t (ascending ps) the stored reads of this context tagged a or b in
        both, at the sites pos, x, y of phase_links under the ps and flip of phase_chain -> (table[S (S + 1) / 2, 4] uint32: (a, a),
        (a, b), (b, a), (b, b), rows in pair_index(S, s, t) order; n_sets; n_reads).  Does not reset."""
        n, at, (xs, ys) = self._phase_sites(pos, x, y)
        n_reads = C.c_uint64(0)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        table, n_sets = self._phase_set_links(lambda sets, fl, cap, table, n_sets: self.L.vga_phase_set_links(self.h, n, _u32p(at), u8(xs), u8(ys), sets, fl, cap, table,
                                                                                                             n_sets, C.byref(n_reads)), n, ps, flip)
        return table, n_sets, int(n_reads.value)

    def phase_set_links_lists(self, recs, words, n_bases, pos, x, y, ref, ps, flip):
        """vga_phase_set_links_lists, the kernel seam: the same from explicit records and words (phase_links_lists) -> (table, n_sets,
        n_reads).  Needs a context only."""
        rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
        wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        n, at, (xs, ys, rf) = self._phase_sites(pos, x, y, ref)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=np.uint32)
        table, n_sets = self._phase_set_links(lambda sets, fl, cap, table, n_sets: self.L.vga_phase_set_links_lists(
            self.h, int(n_bases), len(rc), _u32p(pad(rc)), len(wd), _u32p(pad(wd)), n, _u32p(at), u8(xs), u8(ys), u8(rf), sets, fl, cap, table, n_sets), n, ps, flip)
        return table, n_sets, len(rc)

    def haplotype_paths_begin(self, cap: int = HAPLOTYPE_PATHS_CAP, source: str = "support") -> None:
        """vga_haplotype_paths_begin: from now on every align() of this context keeps, beside the phase store, a row of deficit bytes
        per kept read against every path (needs path_support_begin and phase_begin; source "edit" reads the edit distance and needs
        path_edit_begin).  cap: 1 .. 255."""
        if source not in HAPLOTYPE_PATHS_SOURCES:
            raise VgaError(-1, "haplotype_paths_begin: source %r (support or edit)" % (source,))
        if not 0 <= int(cap) < 1 << 32:
            raise VgaError(-1, "haplotype_paths_begin: cap %r" % (cap,))
        self._check(self.L.vga_haplotype_paths_begin(self.h, int(cap), HAPLOTYPE_PATHS_SOURCES[source]))

    def haplotype_paths_end(self) -> None:
        """vga_haplotype_paths_end: free the deficit store, stop keeping"""
        self._check(self.L.vga_haplotype_paths_end(self.h))

    def haplotype_paths_store(self):
        """vga_haplotype_paths_store -> (deficits uint8[n_reads, n_paths], scored uint8[n_reads]): the rows of the kept reads in the
        order of phase_reads; does not reset"""
        n, np_ = C.c_uint64(0), C.c_uint32(0)
        self._check(self.L.vga_haplotype_paths_store(self.h, None, None, C.byref(n), C.byref(np_)))
        d, sc = np.zeros((max(1, n.value), max(1, np_.value)), dtype=np.uint8), np.zeros(max(1, n.value), dtype=np.uint8)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        self._check(self.L.vga_haplotype_paths_store(self.h, u8(d), u8(sc), C.byref(n), C.byref(np_)))
        return d[:n.value], sc[:n.value]

    def _haplotype_paths(self, call, n, ps, flip, n_paths):
        """`call(ps, flip, cap_groups, reads, table, n_sets)` is one of the two C calls with everything else bound: asked again with
        room for every group when the first answer names more sets than it had room for (nothing was summed then)"""
        sets = np.ascontiguousarray(ps, dtype=np.uint32).reshape(-1)
        fl = np.ascontiguousarray(flip, dtype=np.uint8).reshape(-1)
        if len(sets) != n or len(fl) != n:
            raise VgaError(-1, "haplotype paths: %d sites, %d ps and %d flip" % (n, len(sets), len(fl)))
        pad = lambda a: a if len(a) else np.zeros(1, dtype=a.dtype)
        cap = 2 * int((sets == np.arange(1, n + 1, dtype=np.uint32)).sum())
        while True:
            reads, n_sets = np.zeros(max(1, cap), dtype=np.uint64), C.c_uint64(0)
            table = np.zeros((max(1, cap), max(1, n_paths), HAPLOTYPE_PATHS_COLS), dtype=np.uint64)
            self._check(call(_u32p(pad(sets)), pad(fl).ctypes.data_as(_P(C.c_uint8)), cap, _u64p(reads), _u64p(table), C.byref(n_sets)))
            groups = 2 * int(n_sets.value)
            if groups <= cap:
                return reads[:groups], table[:groups], int(n_sets.value)
            cap = groups

    def haplotype_paths(self, pos, x, y, ps, flip):
        """vga_haplotype_paths: for every phase set s (ascending ps) and haplotype h the scored kept reads of this context tagged h
        in s, at the sites pos, x, y of phase_links under the ps and flip of phase_chain -> (reads uint64[2 S], table[2 S, n_paths,
        2] uint64: (cost, best), group 2 s + h; n_sets; n_reads).  Does not reset."""
        n, at, (xs, ys) = self._phase_sites(pos, x, y)
        n_reads = C.c_uint64(0)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        reads, table, n_sets = self._haplotype_paths(lambda sets, fl, cap, reads, table, n_sets: self.L.vga_haplotype_paths(
            self.h, n, _u32p(at), u8(xs), u8(ys), sets, fl, cap, reads, table, n_sets, C.byref(n_reads)), n, ps, flip, self._n_paths)
        return reads, table, n_sets, int(n_reads.value)

    def haplotype_paths_lists(self, recs, words, n_bases, deficits, scored, pos, x, y, ref, ps, flip):
        """vga_haplotype_paths_lists, the kernel seam: the same from explicit records and words (phase_links_lists), dense deficits
        uint8[n_reads, n_paths] and scored uint8[n_reads] -> (reads, table, n_sets).  Needs a context only."""
        rc = np.ascontiguousarray(recs, dtype=np.uint32).reshape(-1, 3)
        wd = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        df = np.ascontiguousarray(deficits, dtype=np.uint8)
        sc = np.ascontiguousarray(scored, dtype=np.uint8).reshape(-1)
        if df.ndim != 2 or len(df) != len(rc) or len(sc) != len(rc):
            raise VgaError(-1, "haplotype paths: %d reads, deficits of shape %s and %d scored bytes" % (len(rc), df.shape, len(sc)))
        n_paths = int(df.shape[1])
        n, at, (xs, ys, rf) = self._phase_sites(pos, x, y, ref)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        pad = lambda a: a if a.size else np.zeros(3, dtype=a.dtype)
        return self._haplotype_paths(lambda sets, fl, cap, reads, table, n_sets: self.L.vga_haplotype_paths_lists(
            self.h, int(n_bases), len(rc), _u32p(pad(rc)), len(wd), _u32p(pad(wd)), n_paths, u8(pad(df)), u8(pad(sc)), n, _u32p(at), u8(xs), u8(ys), u8(rf), sets, fl, cap,
            reads, table, n_sets), n, ps, flip, n_paths)

    def path_support_begin(self, step_off, steps) -> int:
        """vga_path_support_begin: step_off[n_paths + 1] into steps, the packed handles (id << 1 | is_reverse) of every path
        (hostlib.gfa_paths).  From now on every align() of this context scores its reported alignments against the paths.
        Returns the number of forward step pairs that are no edge of the index."""
        off = np.ascontiguousarray(step_off, dtype=np.uint64)
        st = np.ascontiguousarray(steps, dtype=np.uint64)
        if len(st) == 0:
            st = np.zeros(1, dtype=np.uint64)
        missing = C.c_uint64(0)
        self._n_paths = 0
        self._check(self.L.vga_path_support_begin(self.h, max(0, len(off) - 1), _u64p(off), _u64p(st), C.byref(missing)))
        self._n_paths = len(off) - 1
        return int(missing.value)

    def path_support(self) -> dict:
        """vga_path_support_read -> {sum_bases, sum_edges, top, top_alone: uint64[n_paths], n_alignments, n_unplaced}; does not reset"""
        a = [np.zeros(max(1, self._n_paths), dtype=np.uint64) for _ in range(4)]
        n, un = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_path_support_read(self.h, _u64p(a[0]), _u64p(a[1]), _u64p(a[2]), _u64p(a[3]), C.byref(n), C.byref(un)))
        out = {k: v[:self._n_paths] for k, v in zip(("sum_bases", "sum_edges", "top", "top_alone"), a)}
        out.update(n_alignments=int(n.value), n_unplaced=int(un.value))
        return out

    def path_support_last(self, n_reads: Optional[int] = None):
        """vga_path_support_last -> (bases, edges), uint32[n_reads, n_paths] of the most recent align() of this context"""
        n = self._last_reads if n_reads is None else int(n_reads)
        b, e = (np.zeros((max(1, n), max(1, self._n_paths)), dtype=np.uint32) for _ in range(2))
        self._check(self.L.vga_path_support_last(self.h, n, _u32p(b), _u32p(e)))
        shape = (n, self._n_paths)
        return b.ravel()[:n * self._n_paths].reshape(shape), e.ravel()[:n * self._n_paths].reshape(shape)

    def path_support_reset(self) -> None:
        """vga_path_support_reset: zero the accumulators, keep scoring"""
        self._check(self.L.vga_path_support_reset(self.h))

    def path_support_end(self) -> None:
        """vga_path_support_end: free the state, stop scoring"""
        self._check(self.L.vga_path_support_end(self.h))
        self._n_paths = 0

    def path_support_lists(self, lists, bases):
        """vga_path_support_lists, the kernel seam: lists[i] the node ids of list i in path order, bases[i] the covered bases of
        each of them -> (bases, edges), uint32[len(lists), n_paths]; the accumulators are not touched"""
        n = len(lists)
        off = np.zeros(n + 1, dtype=np.uint64)
        for i, l in enumerate(lists):
            assert len(l) == len(bases[i])
            off[i + 1] = off[i] + len(l)
        ids = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.uint32) for l in lists] + [np.zeros(1, np.uint32)]))
        nb = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.uint32) for l in bases] + [np.zeros(1, np.uint32)]))
        b, e = (np.zeros(max(1, n * self._n_paths), dtype=np.uint32) for _ in range(2))
        self._check(self.L.vga_path_support_lists(self.h, n, _u64p(off), _u32p(ids), _u32p(nb), _u32p(b), _u32p(e)))
        shape = (n, self._n_paths)
        return b[:n * self._n_paths].reshape(shape), e[:n * self._n_paths].reshape(shape)

    def genotype_begin(self) -> None:
        """vga_genotype_begin: needs path_support_begin; from now on every align() of this context adds the pairs of paths of its
        two reads x paths matrices to the pair table"""
        self._check(self.L.vga_genotype_begin(self.h))

    def genotype(self) -> dict:
        """vga_genotype_read -> {sum_bases, sum_edges, prefer_a, prefer_b: uint64[n_paths (n_paths + 1) / 2] at pair_index, n_paths};
        does not reset"""
        n = pair_count(self._n_paths)
        a = [np.zeros(max(1, n), dtype=np.uint64) for _ in range(4)]
        self._check(self.L.vga_genotype_read(self.h, n, _u64p(a[0]), _u64p(a[1]), _u64p(a[2]), _u64p(a[3])))
        out = {k: v[:n] for k, v in zip(GENOTYPE_FIELDS, a)}
        out["n_paths"] = self._n_paths
        return out

    def genotype_reset(self) -> None:
        """vga_genotype_reset: zero the pair table, keep adding"""
        self._check(self.L.vga_genotype_reset(self.h))

    def genotype_end(self) -> None:
        """vga_genotype_end: free the pair table, stop adding"""
        self._check(self.L.vga_genotype_end(self.h))

    def genotype_pairs(self, bases, edges) -> dict:
        """vga_genotype_pairs, the kernel seam: two uint32[n_reads, n_paths] matrices -> the table genotype() returns, from a table
        of its own; needs no index and touches no accumulator"""
        b, e = (np.ascontiguousarray(x, dtype=np.uint32) for x in (bases, edges))
        assert b.ndim == 2 and b.shape == e.shape
        n_reads, n_paths = b.shape
        n = pair_count(n_paths)
        a = [np.zeros(max(1, n), dtype=np.uint64) for _ in range(4)]
        self._check(self.L.vga_genotype_pairs(self.h, n_reads, n_paths, _u32p(b) if b.size else None, _u32p(e) if e.size else None,
                                              _u64p(a[0]), _u64p(a[1]), _u64p(a[2]), _u64p(a[3])))
        out = {k: v[:n] for k, v in zip(GENOTYPE_FIELDS, a)}
        out["n_paths"] = n_paths
        return out

    def genotype_likelihood_begin(self, lam: int = GENOTYPE_LIK_LAMBDA, cap: int = GENOTYPE_LIK_CAP, source: str = "support") -> None:
        """vga_genotype_lik_begin: needs path_support_begin; from now on every align() of this context adds the diploid read
        likelihood cost of every pair of paths, from its two reads x paths matrices, to the cost table.  lam: the cost of one unit
        of deficit in 1/256 bit (1..4096); cap: the largest deficit told apart (1..255); source: "support" (path support's bases and
        edges) or "edit" (vga_genotype_lik_source: m - e of path_edit, which needs path_edit_begin first; a deficit is then a
        count of edits)"""
        if not (0 <= int(lam) < 1 << 32 and 0 <= int(cap) < 1 << 32):
            raise VgaError(-1, "genotype_likelihood_begin: lam %r, cap %r" % (lam, cap))
        if source not in GENOTYPE_LIK_SOURCES:
            raise VgaError(-1, "genotype_likelihood_begin: source %r is neither 'support' nor 'edit'" % (source,))
        self._check(self.L.vga_genotype_lik_begin(self.h, int(lam), int(cap)))
        if source != "support":
            rc = self.L.vga_genotype_lik_source(self.h, GENOTYPE_LIK_SOURCES[source])
            if rc != VGA_OK:
                msg = (self.L.vga_last_error(self.h) or b"").decode()
                self.L.vga_genotype_lik_end(self.h)
                raise VgaError(rc, msg)

    def genotype_likelihood(self) -> dict:
        """vga_genotype_lik_read -> {cost: uint64[n_paths (n_paths + 1) / 2] at pair_index, in 1/256 bit; n_scored; n_paths};
        does not reset"""
        n = pair_count(self._n_paths)
        c = np.zeros(max(1, n), dtype=np.uint64)
        scored = C.c_uint64(0)
        self._check(self.L.vga_genotype_lik_read(self.h, n, _u64p(c), C.byref(scored)))
        return {"cost": c[:n], "n_scored": int(scored.value), "n_paths": self._n_paths}

    def genotype_likelihood_reset(self) -> None:
        """vga_genotype_lik_reset: zero the cost table, keep adding"""
        self._check(self.L.vga_genotype_lik_reset(self.h))

    def genotype_likelihood_end(self) -> None:
        """vga_genotype_lik_end: free the cost table, stop adding"""
        self._check(self.L.vga_genotype_lik_end(self.h))

    def genotype_likelihood_pairs(self, bases, edges, lam: int = GENOTYPE_LIK_LAMBDA, cap: int = GENOTYPE_LIK_CAP) -> dict:
        """vga_genotype_lik_pairs, the kernel seam: two uint32[n_reads, n_paths] matrices -> {cost: uint64[pairs], deficit:
        uint8[n_reads, n_paths], n_scored, n_paths}, from a table of its own; needs no index and touches no accumulator"""
        b, e = (np.ascontiguousarray(x, dtype=np.uint32) for x in (bases, edges))
        assert b.ndim == 2 and b.shape == e.shape
        if not (0 <= int(lam) < 1 << 32 and 0 <= int(cap) < 1 << 32):
            raise VgaError(-1, "genotype_likelihood_pairs: lam %r, cap %r" % (lam, cap))
        n_reads, n_paths = b.shape
        n = pair_count(n_paths)
        c = np.zeros(max(1, n), dtype=np.uint64)
        d = np.zeros(max(1, b.size), dtype=np.uint8)
        scored = C.c_uint64(0)
        self._check(self.L.vga_genotype_lik_pairs(self.h, n_reads, n_paths, _u32p(b) if b.size else None, _u32p(e) if e.size else None,
                                                  int(lam), int(cap), d.ctypes.data_as(_P(C.c_uint8)), _u64p(c), C.byref(scored)))
        return {"cost": c[:n], "deficit": d[:b.size].reshape(b.shape), "n_scored": int(scored.value), "n_paths": n_paths}

    def path_abundance_begin(self, cap: int = PATH_ABUNDANCE_CAP, source: str = "support") -> None:
        """vga_path_abundance_begin: from now on every align() of this context keeps a row of deficit bytes per reported alignment
        against every path (needs path_support_begin; source "edit" reads the edit distance and needs path_edit_begin).  cap: 1 .. 255."""
        if source not in PATH_ABUNDANCE_SOURCES:
            raise VgaError(-1, "path_abundance_begin: source %r (support or edit)" % (source,))
        if not 0 <= int(cap) < 1 << 32:
            raise VgaError(-1, "path_abundance_begin: cap %r" % (cap,))
        self._check(self.L.vga_path_abundance_begin(self.h, int(cap), PATH_ABUNDANCE_SOURCES[source]))

    def path_abundance_reset(self) -> None:
        """vga_path_abundance_reset: empty the store, keep keeping"""
        self._check(self.L.vga_path_abundance_reset(self.h))

    def path_abundance_end(self) -> None:
        """vga_path_abundance_end: free the store, stop keeping"""
        self._check(self.L.vga_path_abundance_end(self.h))

    def path_abundance_store(self):
        """vga_path_abundance_store -> (deficits uint8[n, n_paths], scored uint8[n]): the rows of the reported alignments in the order
        they were reported; does not reset"""
        n = C.c_uint64(0)
        self._check(self.L.vga_path_abundance_store(self.h, 0, None, None, C.byref(n)))
        rows = n.value
        d, sc = np.zeros((max(1, rows), max(1, self._n_paths)), dtype=np.uint8), np.zeros(max(1, rows), dtype=np.uint8)
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8))
        self._check(self.L.vga_path_abundance_store(self.h, rows, u8(d), u8(sc), C.byref(n)))
        return d.ravel()[:rows * self._n_paths].reshape(rows, self._n_paths), sc[:rows]

    def _path_abundance(self, call, n_paths, lam, iters, tol, who):
        if not all(0 <= int(v) < 1 << 32 for v in (lam, iters, tol)):
            raise VgaError(-1, "%s: lam %r, iters %r, tol %r" % (who, lam, iters, tol))
        theta = np.zeros(max(1, n_paths), dtype=np.uint32)
        reads, best = np.zeros(max(1, n_paths), dtype=np.uint64), np.zeros(max(1, n_paths), dtype=np.uint64)
        n, it, conv = C.c_uint64(0), C.c_uint32(0), C.c_uint32(0)
        self._check(call(int(lam), int(iters), int(tol), _u32p(theta), _u64p(reads), _u64p(best), C.byref(n), C.byref(it), C.byref(conv)))
        return {"theta": theta[:n_paths], "reads_q16": reads[:n_paths], "best": best[:n_paths], "n_scored": int(n.value), "iterations": int(it.value),
                "converged": bool(conv.value), "n_paths": n_paths}

    def path_abundance(self, lam: int = PATH_ABUNDANCE_LAMBDA, iters: int = PATH_ABUNDANCE_ITERS, tol: int = PATH_ABUNDANCE_TOL) -> dict:
        """vga_path_abundance: the EM estimate from this context's own store -> {theta: uint32[n_paths] in units of 2^-24, reads_q16:
        uint64[n_paths] (expected reads x 65 536), best: uint64[n_paths] (scored rows with deficit 0), n_scored, iterations, converged,
        n_paths}; does not reset the store"""
        return self._path_abundance(lambda *a: self.L.vga_path_abundance(self.h, *a), self._n_paths, lam, iters, tol, "path_abundance")

    def path_abundance_rows(self, deficits, scored, lam: int = PATH_ABUNDANCE_LAMBDA, iters: int = PATH_ABUNDANCE_ITERS, tol: int = PATH_ABUNDANCE_TOL) -> dict:
        """vga_path_abundance_rows, the kernel seam: the same from explicit rows, deficits uint8[n_rows, n_paths] and scored
        uint8[n_rows]; needs no index and touches no store"""
        d, sc = np.ascontiguousarray(deficits, dtype=np.uint8), np.ascontiguousarray(scored, dtype=np.uint8).reshape(-1)
        assert d.ndim == 2 and d.shape[0] == len(sc)
        n_rows, n_paths = d.shape
        u8 = lambda a: a.ctypes.data_as(_P(C.c_uint8)) if a.size else None
        return self._path_abundance(lambda *a: self.L.vga_path_abundance_rows(self.h, n_rows, n_paths, u8(d), u8(sc), *a), n_paths, lam, iters, tol,
                                    "path_abundance_rows")

    def path_edit_begin(self) -> None:
        """vga_path_edit_begin: needs path_support_begin; from now on every align() of this context scores the read of every
        reported alignment against every path by edit distance"""
        self._check(self.L.vga_path_edit_begin(self.h))

    def path_edit(self) -> dict:
        """vga_path_edit_read -> {n_scored, sum_edit, best, best_alone: uint64[n_paths], n_alignments, n_too_long}; does not reset"""
        a = [np.zeros(max(1, self._n_paths), dtype=np.uint64) for _ in range(4)]
        n, long_ = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.vga_path_edit_read(self.h, _u64p(a[0]), _u64p(a[1]), _u64p(a[2]), _u64p(a[3]), C.byref(n), C.byref(long_)))
        out = {k: v[:self._n_paths] for k, v in zip(PATH_EDIT_FIELDS, a)}
        out.update(n_alignments=int(n.value), n_too_long=int(long_.value))
        return out

    def path_edit_last(self, n_reads: Optional[int] = None):
        """vga_path_edit_last -> uint32[n_reads, n_paths] of the most recent align() of this context; PATH_EDIT_NONE: not scored"""
        n = self._last_reads if n_reads is None else int(n_reads)
        e = np.zeros(max(1, n * self._n_paths), dtype=np.uint32)
        self._check(self.L.vga_path_edit_last(self.h, n, _u32p(e)))
        return e[:n * self._n_paths].reshape((n, self._n_paths))

    def path_edit_reset(self) -> None:
        """vga_path_edit_reset: zero the accumulators, keep scoring"""
        self._check(self.L.vga_path_edit_reset(self.h))

    def path_edit_end(self) -> None:
        """vga_path_edit_end: free the state, stop scoring"""
        self._check(self.L.vga_path_edit_end(self.h))

    def path_edit_pairs(self, queries, texts) -> np.ndarray:
        """vga_path_edit_pairs, the kernel seam: the infix edit distance of queries[i] in texts[i] (str or bytes) through the
        distance kernel -> uint32[n]; PATH_EDIT_NONE for a query of more than PATH_EDIT_MAX_QUERY letters.  Needs no index and
        touches no accumulator"""
        assert len(queries) == len(texts)
        n = len(queries)
        enc = lambda x: x if isinstance(x, bytes) else x.encode()
        qs, ts = [enc(x) for x in queries], [enc(x) for x in texts]
        q_off, t_off = (np.zeros(n + 1, dtype=np.uint64) for _ in range(2))
        q_off[1:] = np.cumsum([len(x) for x in qs], dtype=np.uint64)
        t_off[1:] = np.cumsum([len(x) for x in ts], dtype=np.uint64)
        out = np.zeros(max(1, n), dtype=np.uint32)
        self._check(self.L.vga_path_edit_pairs(self.h, n, _u64p(q_off), b"".join(qs), _u64p(t_off), b"".join(ts), _u32p(out)))
        return out[:n]

    def chain_paths_text(self, chains: "MapOut") -> List[bytes]:
        """the path column of every chain's GAF record (vga_chain_paths_text), one bytes object per chain"""
        out = _P(ChainText)()
        self._check(self.L.vga_chain_paths_text(self.h, chains._ptr, C.byref(out)))
        try:
            t = out.contents
            n = int(t.n_chains)
            off = [int(t.text_off[i]) for i in range(n + 1)]
            raw = C.string_at(t.text, off[n]) if off[n] else b""
            return [raw[off[i]:off[i + 1]] for i in range(n)]
        finally:
            self.L.vga_chain_text_free(out)

    def kernel_times(self):
        arr = (KernelTime * 32)()
        n = self.L.vga_last_kernel_times(self.h, arr, 32)
        return [{"name": arr[i].name.decode(), "ms": float(arr[i].ms), "launches": int(arr[i].launches),
                 "algorithmic_bytes": int(arr[i].algorithmic_bytes), "busy_ms": float(arr[i].busy_ms)} for i in range(min(n, 32))]

    def synchronize(self):
        self._check(self.L.vga_ctx_synchronize(self.h))

    def close(self):
        if self.h:
            self.L.vga_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def deletion_state(reads: int, depth: int, error: int = VARIANT_ERROR):
    """vga_deletion_state: the rule of the deletion call alone -> (state: 0 none, 1 het, 2 hom; qual)"""
    q = C.c_uint32(0)
    state = load_library().vga_deletion_state(int(reads), int(depth), int(error), C.byref(q))
    return int(state), int(q.value)
