"""The pileup, the parts that need no GPU: the reference walker (tests/pileup_ref.py) checked on the oracle's alignments GAF and
on hand-written records, the four vga_pileup_* calls in the ABI, the command line's refusal of --pileup without --also-align,
and the scratch budget of k_pu_events / k_pu_add / k_pu_finish from a cross-compile for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

import coverage_ref
import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_pileup_begin", "vga_pileup_read", "vga_pileup_reset", "vga_pileup_end"]


# ---- the walker on the oracle's text
def test_walker_on_the_oracle_gaf(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    reads = pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)
    _, ag, _ = oracle.map_reads(ix, [r.name for r in reads], [r.seq for r in reads])
    a = oracle_index_arrays(ix)
    # (walk asserts per record: it ends at path_end on the last path node, covers block_length bases, and meets the graph base
    # every *gq and -g.. names)
    counts, n_al, leading = pileup_ref.walk(ag, a["node_seq_idx"], a["seq_fwd"])
    assert n_al == len(reads) and counts.shape == (len(a["seq_fwd"]), 7) and counts.dtype == np.uint32
    base, _, _, n_cov = coverage_ref.walk(ag, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    assert n_cov == n_al
    assert np.array_equal(counts[:, :5].sum(1), base), "A + C + G + T + N is the depth"
    n_del, n_ins = pileup_ref.cs_totals(ag)
    assert int(counts[:, pileup_ref.DEL].sum()) == n_del > 0
    assert int(counts[:, pileup_ref.INS].sum()) + leading == n_ins > 0
    # most of what the reads say is what the graph holds
    seq = a["seq_fwd"].decode()
    own = np.array([pileup_ref.column(c) for c in seq])
    assert int(counts[np.arange(len(seq)), own].sum()) > 0.9 * int(base.sum())


# ---- hand-written records
# nodes 1 "ACGT" (positions 0..3), 2 "GGCAT" (4..8), 3 "TTA" (9..11)
IDX3, SEQ3 = [0, 4, 9, 12], "ACGTGGCATTTA"


def _record(name, strand, path, start, end, block, cs):
    return "\t".join([name, "20", "0", "20", strand, path, "12", str(start), str(end), str(block), str(block), "255", "as:i:-30 cs:Z:" + cs + ",cg:Z:1M"])


def test_walker_token_effects():
    """a leading insertion, a match run over a node boundary, *gq, an insertion after a covered base, *gn, a deletion over a node
    boundary, an insertion after a deleted base, a closing match run; a '-' record walks the same way; a placeholder adds nothing"""
    a = _record("a", "+", ">1>2>3", 1, 3, 8, "+ac:4*ga+t*cn-att+g:2")
    b = _record("b", "-", ">2", 0, 4, 4, ":3*at")
    ph = "\t".join(["q", "5", "0", "5", "+", "*", "0", "0", "0", "0", "0", "255", "x"])
    counts, n, leading = pileup_ref.walk("\n".join([a, ph, b]) + "\n", IDX3, SEQ3)
    want = np.zeros((12, 7), dtype=np.uint32)
    A, C, G, T, N, DEL, INS = range(7)
    for pos, col, v in [(1, C, 1), (2, G, 1), (3, T, 1), (4, G, 2),      # a's :4 crosses from node 1 into node 2; b's :3 starts at 4
                        (5, A, 1), (5, INS, 1), (5, G, 1),               # a: *ga and the +t behind it; b: match
                        (6, N, 1), (6, C, 1),                            # a: *cn; b: match
                        (7, DEL, 1), (7, T, 1),                          # a: -att starts; b: *at
                        (8, DEL, 1), (9, DEL, 1), (9, INS, 1),           # ... crosses into node 3; +g belongs to the deleted base
                        (10, T, 1), (11, A, 1)]:
        want[pos, col] += v
    assert n == 2 and leading == 1
    assert np.array_equal(counts, want), (counts.tolist(), want.tolist())


@pytest.mark.parametrize("cs,start,end,block", [("*ca:2", 0, 3, 3),     # the graph holds a at 0, not c
                                                 ("-c:2", 0, 3, 2),      # likewise for a deletion
                                                 (":3", 0, 4, 3),        # ends short of path_end
                                                 (":3", 0, 3, 4)])       # covers fewer bases than block_length
def test_walker_checks_itself(cs, start, end, block):
    with pytest.raises(AssertionError):
        pileup_ref.walk(_record("x", "+", ">1", start, end, block, cs) + "\n", IDX3, SEQ3)


# ---- the ABI
def test_abi_lists_and_exports_the_four_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    # the header as C99, with the four calls taken by address under their documented types
    src = tmp_path / "pu.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*b)(vga_ctx *) = vga_pileup_begin;\n"
                   "int (*r)(vga_ctx *, uint32_t *, uint64_t *, uint64_t *) = vga_pileup_read;\n"
                   "int (*z)(vga_ctx *) = vga_pileup_reset;\n"
                   "int (*e)(vga_ctx *) = vga_pileup_end;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "pu.o")])
    assert p.binding.PILEUP_COLUMNS == pileup_ref.COLUMNS


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    assert L.vga_pileup_begin(None) == -1 and L.vga_pileup_read(None, None, None, None) == -1
    assert L.vga_pileup_reset(None) == -1 and L.vga_pileup_end(None) == -1


# ---- the command line
def test_cli_pileup_needs_also_align(tmp_path):
    pkg()
    pr = subprocess.run([EXE, "map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--pileup"],
                        cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and "--pileup" in pr.stderr, pr.stderr
    # refused while the arguments are read: no index is looked for (the files do not exist) and no device is opened
    assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "--pileup" in usage.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def pu_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("puisa") / "pu.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_pileup.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel", ["k_pu_events", "k_pu_add", "k_pu_finish"])
def test_pileup_kernels_without_scratch(pu_isa, kernel):
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"E\w*)\n", pu_isa):
        a = pu_isa.rfind("\n  - ", 0, m.start())
        b = pu_isa.find("\n  - ", m.end())
        entries.append(pu_isa[a:b if b >= 0 else len(pu_isa)])
    assert len(entries) == 1, kernel
    field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))
    print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("wavefront_size") == 64
    if kernel != "k_pu_finish":
        assert field("group_segment_fixed_size") == 0 and field("max_flat_workgroup_size") == 64  # one wave per problem / alignment
