"""The variant call, the parts that need no GPU: the reference (tests/variant_ref.py) on hand-made rows -- every tie the
definition names, N as a base's own letter, the depth threshold --, a planted substitution found again on the oracle's alignments
GAF, the two vga_variant_* calls in the ABI, the command line's refusals, and the scratch budget of the three kernels from a
cross-compile for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_variant_call", "vga_variant_call_table"]
A, C, G, T, D = range(5)


def row(a=0, c=0, g=0, t=0, n=0, dele=0, ins=0):
    return [a, c, g, t, n, dele, ins]


def gt(s):
    return (s["x"], s["y"])


# ---- the reference on hand-made rows
def test_the_order_of_the_pairs():
    assert variant_ref.pair_order(G) == [(G, G), (A, G), (C, G), (G, T), (G, D),
                                         (A, A), (A, C), (A, T), (A, D), (C, C), (C, T), (C, D), (T, T), (T, D), (D, D)]
    for r in range(4):
        o = variant_ref.pair_order(r)
        assert len(o) == 15 == len(set(o)) and all(x <= y for x, y in o)


def test_plain_calls():
    s = variant_ref.site(row(a=10), "A")
    assert s["tested"] and not s["reported"] and gt(s) == (A, A) and s["ins"] == 0
    assert s["qual"] == 10 * 256          # the next pair is a heterozygous one that holds A
    s = variant_ref.site(row(a=5, g=5), "a")   # lower case is the same letter
    assert s["reported"] and gt(s) == (A, G) and s["depth"] == 10
    assert s["qual"] == 5 * 1280 - 10 * 256    # (A, A) and (G, G) cost 5 E, (A, G) 10 * 256
    s = variant_ref.site(row(t=9), "C")
    assert s["reported"] and gt(s) == (T, T) and s["qual"] == 9 * 256
    s = variant_ref.site(row(c=4, dele=4), "C")
    assert s["reported"] and gt(s) == (C, D)
    s = variant_ref.site(row(dele=6), "G")
    assert s["reported"] and gt(s) == (D, D)


def test_the_reference_genotype_wins_its_tie():
    """E = 1280 and n_r = 4 n_a: (r, r) costs 1280 n_a, (r, a) 256 * 5 n_a, the same"""
    for n_a in (1, 3, 1000):
        s = variant_ref.site(row(c=4 * n_a, t=n_a), "C", error=1280, min_depth=1, min_qual=0)
        assert gt(s) == (C, C) and s["qual"] == 0 and not s["reported"]
    s = variant_ref.site(row(c=4 * 3 - 1, t=3), "C", error=1280, min_depth=1, min_qual=0)   # one observation fewer: the pair wins
    assert gt(s) == (C, T) and s["qual"] == 256 and s["reported"]


def test_the_pair_that_holds_r_wins_against_the_homozygous_other():
    """n_a = 4 n_r: (a, a) costs 1280 n_r, (r, a) 256 * 5 n_r; the pair that holds r comes first"""
    s = variant_ref.site(row(g=2, a=8), "G", min_qual=0)
    assert gt(s) == (A, G) and s["qual"] == 0 and s["reported"]
    assert not variant_ref.site(row(g=2, a=8), "G", min_qual=1)["reported"]


def test_ties_among_the_pairs_follow_the_order():
    # three pairs tie at 7168 with r = A: (A, C), (A, G) hold r, (C, G) does not; the other allele ascending picks (A, C)
    s = variant_ref.site(row(a=4, c=4, g=4), "A", min_qual=0)
    assert gt(s) == (A, C) and s["qual"] == 0
    # the same row seen from T: none of the three holds r, (x, y) ascending picks (A, C) again; from G it is (A, G)
    assert gt(variant_ref.site(row(a=4, c=4, g=4), "T", min_qual=0)) == (A, C)
    assert gt(variant_ref.site(row(a=4, c=4, g=4), "G", min_qual=0)) == (A, G)
    # two pairs without r: (C, G) = 256 * 20 and (G, G) = 4 * 1280 tie, (1, 2) comes before (2, 2)
    s = variant_ref.site(row(c=4, g=16), "A", min_qual=0)
    assert gt(s) == (C, G) and s["qual"] == 0
    # a deleted base is the last allele
    assert gt(variant_ref.site(row(t=4, dele=4, c=4), "A", min_qual=0)) == (C, T)


def test_the_three_insertion_ties():
    # none against het: ins E = 256 depth
    s = variant_ref.site(row(a=5, ins=1), "A", error=1280)
    assert s["ins"] == 0 and s["ins_qual"] == 0
    # het against hom: 256 depth = (depth - k) E, none far above
    s = variant_ref.site(row(a=5, ins=4), "A", error=1280, min_qual=0)
    assert s["ins"] == 1 and s["ins_qual"] == 0 and s["reported"]
    # none against hom: ins = depth - ins, het above both with E below 512
    s = variant_ref.site(row(a=4, ins=2), "A", error=400)
    assert s["ins"] == 0 and s["ins_qual"] == 0
    # all three: E = 512
    s = variant_ref.site(row(a=4, ins=2), "A", error=512)
    assert s["ins"] == 0 and s["ins_qual"] == 0
    # and the plain cases: every read inserts, more insertions than reads, half of them
    assert variant_ref.site(row(a=6, ins=6), "A")["ins"] == 2
    s = variant_ref.site(row(a=6, ins=9), "A")
    assert s["ins"] == 2 and s["ins_qual"] == 6 * 256 and s["reported"] and gt(s) == (A, A)
    assert variant_ref.site(row(a=6, ins=3), "A")["ins"] == 1


def test_n_counts_towards_depth_only_and_is_never_tested():
    s = variant_ref.site(row(a=2, n=2), "A", min_depth=4)
    assert s["tested"] and s["depth"] == 4 and gt(s) == (A, A) and s["qual"] == 2 * 256   # the two N cost no pair anything
    for letter in "NnRx-":
        s = variant_ref.site(row(c=50), letter)
        assert not s["tested"] and not s["reported"] and s["depth"] == 50
    c = variant_ref.call_table([row(c=50), row(c=50)], "NA")
    assert c["n_tested"] == 1 and c["pos"].tolist() == [1]


def test_depth_below_and_at_the_threshold():
    below, at = variant_ref.site(row(g=3), "A", min_depth=4), variant_ref.site(row(g=3, n=1), "A", min_depth=4)
    assert not below["tested"] and not below["reported"] and gt(below) == (G, G)
    assert at["tested"] and at["reported"] and at["depth"] == 4
    c = variant_ref.call_table([row(g=3), row(g=4), row(a=7), row(g=2, n=2)], "AAAA", min_depth=4)
    assert (c["n_tested"], c["n_calls"]) == (3, 2) and c["pos"].tolist() == [1, 3] and c["depth"].tolist() == [4, 4]


def test_wide_counters_and_saturation():
    m = 2**32 - 1
    s = variant_ref.site([m] * 7, "A", error=8192)
    assert s["depth"] == 6 * m and s["tested"]
    assert s["qual"] == 0                                  # every allele as often as every other: all heterozygous pairs tie
    assert gt(s) == (A, C) and s["ins"] == 1 and s["ins_qual"] == m * 8192 - 256 * 6 * m
    s = variant_ref.site(row(t=2**40 - 1), "A", error=8192)
    assert gt(s) == (T, T) and s["qual"] == variant_ref.QUAL_MAX   # 256 (2^40 - 1) saturates


def test_table_and_tsv():
    idx, seq = [0, 4, 9, 12], "ACGTGGCATTTA"
    tab = np.zeros((12, 7), dtype=np.uint64)
    tab[np.arange(12), [variant_ref.pileup_ref.column(c) for c in seq]] = 8
    tab[4] = row(g=4, t=4)             # first base of node 2
    tab[11] = row(a=8, ins=8)          # last base of node 3
    c = variant_ref.call_table(tab, seq)
    assert c["n_tested"] == 12 and c["pos"].tolist() == [4, 11]
    assert variant_ref.tsv(c, idx, seq) == (variant_ref.HEADER + "\n"
                                            "2\t0\tG\tG/T\t3072\t.\t2048\t8\t0\t0\t4\t4\t0\t0\t0\n"
                                            "3\t2\tA\tA/A\t2048\thom\t2048\t8\t8\t0\t0\t0\t0\t0\t8\n")
    assert variant_ref.same(c, c) is None
    d = dict(c, qual=c["qual"] + 1)
    assert variant_ref.same(c, d) == "qual"


# ---- a planted variant on the oracle's text
def test_planted_substitution_is_reported(oracle):
    """A sample from one path of DRB1 whose sequence carries one substitution no path has: 12 reads of 1000 bases with 1 % of
    each error, tiled so that the site moves through the read.  The reference reports that graph base, homozygous for the planted
    letter; the calls it reports beside it on this sample (the reads' own errors: mostly two deletions that met at depth 6 to 9)
    are recorded in DESIGN.md section 20, and printed here."""
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    idx = [int(x) for x in a["node_seq_idx"]]
    segs, paths = rs.parse_gfa_paths(DRB1)
    name, steps = paths[3]
    assert not any(rev for _, rev in steps)
    # the site: the middle of the first node of 50 bases or more behind offset 2000 of the path
    off = 0
    for nid, _ in steps:
        if off >= 2000 and len(segs[nid]) >= 50:
            break
        off += len(segs[nid])
    site_path, site_graph = off + len(segs[nid]) // 2, idx[nid - 1] + len(segs[nid]) // 2
    seq = rs.path_sequence(segs, steps)
    old = seq[site_path].upper()
    assert a["seq_fwd"].decode()[site_graph].upper() == old
    new = "ACGT"[("ACGT".index(old) + 1) % 4]
    mut = seq[:site_path] + new + seq[site_path + 1:]
    n_reads, length = 12, 1000
    rng = np.random.Generator(np.random.PCG64(11))
    reads = []
    for r in range(n_reads):
        o = site_path - length + (r + 1) * length // (n_reads + 1)
        tpl = np.frombuffer(mut[o:o + length].encode(), dtype=np.uint8)
        reads.append(("planted%d" % r, rs._mutate(tpl, rng, 0.01, 0.01, 0.01).decode()))
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    c = variant_ref.call_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    print("tested", c["n_tested"], "calls", c["n_calls"], "\n" + variant_ref.tsv(c, a["node_seq_idx"], a["seq_fwd"]))
    at = c["pos"].tolist().index(site_graph)
    planted = "ACGT".index(new)
    assert (int(c["x"][at]), int(c["y"][at])) == (planted, planted)
    assert int(c["depth"][at]) == n_reads and int(c["counts"][at][planted]) == n_reads and int(c["qual"][at]) == n_reads * 256
    # without the substitution the same reads do not report the base
    plain = []
    rng = np.random.Generator(np.random.PCG64(11))
    for r in range(n_reads):
        o = site_path - length + (r + 1) * length // (n_reads + 1)
        plain.append(("plain%d" % r, rs._mutate(np.frombuffer(seq[o:o + length].encode(), dtype=np.uint8), rng, 0.01, 0.01, 0.01).decode()))
    _, ag0, _ = oracle.map_reads(ix, [n for n, _ in plain], [s for _, s in plain])
    c0 = variant_ref.call_gaf(ag0, a["node_seq_idx"], a["seq_fwd"])
    assert site_graph not in c0["pos"].tolist()
    assert sorted(set(c["pos"].tolist()) - {site_graph}) == sorted(c0["pos"].tolist())   # the other calls are the reads' errors


# ---- the ABI
def test_abi_lists_and_exports_the_two_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    assert not re.search(r"typedef\s+struct[^;]*variant", header)   # scalars and parallel arrays: no new struct
    src = tmp_path / "vc.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*c)(vga_ctx *, uint32_t, uint64_t, uint64_t, uint64_t, uint32_t *, uint8_t *, uint32_t *, uint64_t *, uint64_t *, uint64_t *,\n"
                   "         uint64_t *, uint64_t *) = vga_variant_call;\n"
                   "int (*t)(vga_ctx *, uint64_t, const uint64_t *, const char *, uint32_t, uint64_t, uint64_t, uint64_t, uint32_t *, uint8_t *,\n"
                   "         uint32_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t *) = vga_variant_call_table;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "vc.o")])
    b = p.binding
    assert (b.VARIANT_ERROR, b.VARIANT_MIN_DEPTH, b.VARIANT_MIN_QUAL) == (variant_ref.ERROR, variant_ref.MIN_DEPTH, variant_ref.MIN_QUAL) == (1280, 4, 512)
    assert b.VARIANT_ALLELES == variant_ref.ALLELES and b.VARIANT_INS_STATES == variant_ref.INS_STATES
    hpp = open(os.path.join(CSRC, "vga_variant.hpp")).read()
    for macro, value in [("VC_BLOCK", b.VARIANT_BLOCK), ("VC_MIN_ERROR", b.VARIANT_MIN_ERROR), ("VC_MAX_ERROR", b.VARIANT_MAX_ERROR)]:
        assert int(re.search(r"#define " + macro + r" (\d+)u", hpp).group(1)) == value
    assert hasattr(b.Context, "variant_call") and hasattr(b.Context, "variant_call_table")


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    none = [None] * 8
    assert L.vga_variant_call(None, 1280, 4, 512, 0, *none) == -1
    assert L.vga_variant_call_table(None, 0, None, None, 1280, 4, 512, 0, *none) == -1


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa"] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300, env=env)


def refused(pr, *words):
    assert pr.returncode != 0
    for w in words:
        assert w in pr.stderr, pr.stderr
    # refused while the arguments are read: no index is looked for (the files do not exist) and no device is opened
    assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr


def test_cli_call_variants_needs_also_align(tmp_path):
    pkg()
    refused(run_cli(["--call-variants"], tmp_path), "--call-variants", "--also-align")


@pytest.mark.parametrize("option", ["--call-error", "--call-min-depth", "--call-min-qual"])
def test_cli_value_options_need_the_switch(tmp_path, option):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", option, "600"], tmp_path), option, "--call-variants")


@pytest.mark.parametrize("option,value", [("--call-error", "256"), ("--call-error", "8193"), ("--call-error", "x"), ("--call-error", "-5"),
                                          ("--call-min-depth", "0"), ("--call-min-depth", "3.5"), ("--call-min-qual", "-1"), ("--call-min-qual", "")])
def test_cli_refuses_values_out_of_range(tmp_path, option, value):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--call-variants", option, value], tmp_path), option)


def test_usage_names_the_switch():
    pkg()
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    for w in ("--call-variants", "--call-error 1280", "--call-min-depth 4", "--call-min-qual 512"):
        assert w in usage.stderr, usage.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def vc_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vcisa") / "vc.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_variant.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel,copies,lds", [("k_vc_count", 2, 32), ("k_vc_scan", 1, 8192), ("k_vc_emit", 2, 16)])
def test_variant_kernels_without_scratch(vc_isa, kernel, copies, lds):
    """one copy per counter type (32-bit for the context's own counters, 64-bit for the seam); no scratch, no spill, and no LDS
    beyond the wave counts and the scan"""
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"I?\w*)\n", vc_isa):
        a = vc_isa.rfind("\n  - ", 0, m.start())
        b = vc_isa.find("\n  - ", m.end())
        entries.append(vc_isa[a:b if b >= 0 else len(vc_isa)])
    assert len(entries) == copies, (kernel, len(entries))
    for e in entries:
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("wavefront_size") == 64 and field("group_segment_fixed_size") == lds
