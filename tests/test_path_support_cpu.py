"""Path support, the parts that need no GPU: the reference walker (tests/path_support_ref.py) on a hand-written graph and on the
oracle's alignments GAF, the host library's view of the P lines, the six vga_path_support_* calls in the ABI, the command line's
refusals, and the scratch budget of k_ps_build / k_ps_score from a cross-compile for gfx950."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import path_support_ref
from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_path_support_begin", "vga_path_support_read", "vga_path_support_last", "vga_path_support_reset", "vga_path_support_end",
         "vga_path_support_lists"]

# a diamond 1 -> {2, 3} -> 4 and a node 5 no path visits.  Path b visits node 3 twice and steps 4+,3+ without an L line, path c is
# all '-', path d shares the arm 2 -> 4 with a.
DIAMOND = "\n".join(["H\tVN:Z:1.0", "S\t1\tACGT", "S\t2\tCCA", "S\t3\tGG", "S\t4\tTTTTT", "S\t5\tAAA",
                     "L\t1\t+\t2\t+\t0M", "L\t1\t+\t3\t+\t0M", "L\t2\t+\t4\t+\t0M", "L\t3\t+\t4\t+\t0M",
                     "P\ta\t1+,2+,4+\t*", "P\tb\t1+,3+,4+,3+\t*", "P\tc\t4-,2-,1-\t*", "P\td\t2+,4+\t*"]) + "\n"


def gaf_line(name, path, start, end, block, cs):
    return "\t".join([name, "9", "0", "9", "+", path, "9", str(start), str(end), str(block), str(block), "255", "as:i:-30 cs:Z:" + cs + ",cg:Z:1M"])


# ---- the walker on a hand-written graph
def test_walker_token_effects(tmp_path):
    gfa = tmp_path / "diamond.gfa"
    gfa.write_text(DIAMOND)
    node_len, paths = path_support_ref.parse_gfa(str(gfa))
    assert node_len == {1: 4, 2: 3, 3: 2, 4: 5, 5: 3} and [p[0] for p in paths] == ["a", "b", "c", "d"]
    gaf = "\n".join([
        # node 1 from offset 1: 3 matches; node 2: a mismatch, a deletion of its other two bases; an insertion; node 4: 2 matches
        gaf_line("r0", ">1>2>4", 1, 2, 6, ":3*ag-cc+tt:2"),
        gaf_line("r1", ">1>3>4", 0, 5, 11, ":11"),
        "\t".join(["r2", "5", "0", "5", "+", "*", "0", "0", "0", "0", "0", "255", "x"]),
        gaf_line("r3", ">2>4", 0, 5, 8, ":3:5"),
        gaf_line("r4", ">5", 0, 3, 3, ":3"),
    ]) + "\n"
    w = path_support_ref.walk(gaf, node_len, paths)
    #                                    a  b   c  d
    assert w["bases"].tolist() == [[6, 5, 0, 3],    # r0: b has nodes 1 and 4 only, d nodes 2 (1 covered base) and 4
                                   [9, 11, 0, 5],   # r1: node 3 of b counts once though b visits it twice
                                   [0, 0, 0, 0],    # r2: a placeholder
                                   [8, 5, 0, 8],
                                   [0, 0, 0, 0]]    # r4: node 5 is on no path
    assert w["edges"].tolist() == [[2, 0, 0, 1], [0, 2, 0, 0], [0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0]]
    assert w["top_paths"] == [[0], [1], [], [0, 3], []]
    assert w["top"].tolist() == [2, 1, 0, 1] and w["top_alone"].tolist() == [1, 1, 0, 0]
    assert w["sum_bases"].tolist() == [23, 21, 0, 16] and w["sum_edges"].tolist() == [3, 2, 0, 2]
    assert w["n_alignments"] == 4 and w["n_unplaced"] == 1
    # the all-'-' path scores nothing although the records cross its nodes; 4+,3+ of b is a pair no record can hold
    off, steps = path_support_ref.packed_steps(paths)
    assert off.tolist() == [0, 3, 7, 10, 12] and steps.tolist() == [2, 4, 8, 2, 6, 8, 6, 9, 5, 3, 4, 8]
    # the self-checks: a walk that ends at offset 2 of node 2 and covers 6 bases passes, a wrong path_end or block_length does not
    path_support_ref.walk(gaf_line("ok", ">1>2", 0, 2, 6, ":6") + "\n", node_len, paths)
    for end, block in ((3, 6), (2, 5)):
        with pytest.raises(AssertionError):
            path_support_ref.walk(gaf_line("bad", ">1>2", 0, end, block, ":6") + "\n", node_len, paths)


# ---- the walker on the oracle's text
def test_walker_on_the_oracle_gaf(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    reads = pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)
    _, ag, _ = oracle.map_reads(ix, [r.name for r in reads], [r.seq for r in reads])
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    assert len(paths) == 12
    w = path_support_ref.walk(ag, node_len, paths)
    assert w["n_alignments"] == len(reads) and w["n_unplaced"] == 0
    names = [p[0] for p in paths]
    reverse = [i for i, (_, st) in enumerate(paths) if all(rev for _, rev in st)]
    assert [names[i] for i in reverse] == ["gi|345525392:5000-18402"]
    nonzero = (w["bases"] > 0) | (w["edges"] > 0)
    assert nonzero.sum(axis=1).tolist() == [11] * len(reads)
    assert not nonzero[:, reverse[0]].any()
    hits = sum(1 for r, rd in enumerate(reads) if names.index(rd.path) in w["top_paths"][r])
    print("true path among the top paths:", hits, "of", len(reads))
    assert hits >= 22


# ---- the host library's view of the P lines
@pytest.mark.parametrize("gfa", sorted(glob.glob(os.path.join(DATA, "*.gfa")) + glob.glob(os.path.join(DATA, "hla", "*.gfa"))),
                         ids=lambda g: os.path.basename(g))
def test_hostlib_paths_equal_a_plain_parse(gfa):
    node_len, paths = path_support_ref.parse_gfa(gfa)
    got = pkg().hostlib.gfa_paths(gfa)
    off, steps = path_support_ref.packed_steps(paths)
    assert got["names"] == [p[0] for p in paths]
    assert got["step_off"].dtype == np.uint64 and got["step_off"].tolist() == off.tolist()
    assert got["steps"].dtype == np.uint64 and got["steps"].tolist() == steps.tolist()
    assert got["length"].tolist() == [sum(node_len[n] for n, rev in st if not rev) for _, st in paths]


def test_golden_graphs_hold_the_cases_the_paths_test_names():
    repeats = lambda g: any(len({n for n, _ in st}) < len(st) for _, st in path_support_ref.parse_gfa(os.path.join(DATA, "hla", g))[1])
    assert repeats("5-B3106.gfa") and repeats("7-MICB-4277.gfa")
    assert any(all(rev for _, rev in st) for _, st in path_support_ref.parse_gfa(DRB1)[1])


# ---- the ABI
def test_abi_lists_and_exports_the_six_calls():
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6


def test_null_context():
    L = pkg().binding.load_library()
    assert L.vga_path_support_begin(None, 0, None, None, None) in (-1, -6)  # VGA_ERR_ARG or VGA_ERR_NO_DEVICE
    assert L.vga_path_support_read(None, None, None, None, None, None, None) == -1
    assert L.vga_path_support_last(None, 0, None, None) == -1 and L.vga_path_support_lists(None, 0, None, None, None, None, None) == -1
    assert L.vga_path_support_reset(None) == -1 and L.vga_path_support_end(None) == -1


# ---- the command line: refusals before any device is opened
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300, env=env)


def test_cli_path_support_needs_also_align(tmp_path):
    pkg()
    pr = run_cli(["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--path-support"], tmp_path)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and "--path-support" in pr.stderr, pr.stderr


@pytest.fixture(scope="module")
def test_index(tmp_path_factory):
    pkg()
    d = tmp_path_factory.mktemp("psidx")
    gfa = os.path.join(DATA, "test.gfa")
    pr = subprocess.run([EXE, "index", "-i", gfa, "-k", "11", "-o", str(d / "t")], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    (d / "r.fa").write_text(">r\nACGTACGTACGT\n")
    return d, gfa


def test_cli_refuses_a_graph_without_paths(test_index):
    d, gfa = test_index
    bare = d / "bare.gfa"
    bare.write_text("".join(ln for ln in open(gfa) if not ln.startswith("P")))
    pr = run_cli(["map", "-i", str(d / "t"), "-f", str(d / "r.fa"), "-p", "abpoa", "--also-align", "-G", str(bare), "--path-support", "-o", str(d / "o1")], d)
    assert pr.returncode != 0 and "no P line" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr  # (refused before a context was asked for)
    assert not glob.glob(str(d / "o1*"))


def test_cli_refuses_a_graph_that_is_not_the_index_s(test_index):
    d, _ = test_index
    pr = run_cli(["map", "-i", str(d / "t"), "-f", str(d / "r.fa"), "-p", "abpoa", "--also-align", "-G", DRB1, "--path-support", "-o", str(d / "o2")], d)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    # ... node lengths too: the same graph with one base more on its first node
    longer = d / "longer.gfa"
    lines = open(os.path.join(DATA, "test.gfa")).read().splitlines()
    k = next(i for i, ln in enumerate(lines) if ln.startswith("S\t"))
    f = lines[k].split("\t")
    f[2] += "A"
    lines[k] = "\t".join(f)
    longer.write_text("\n".join(lines) + "\n")
    pr = run_cli(["map", "-i", str(d / "t"), "-f", str(d / "r.fa"), "-p", "abpoa", "--also-align", "-G", str(longer), "--path-support", "-o", str(d / "o3")], d)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert not glob.glob(str(d / "o2*")) and not glob.glob(str(d / "o3*"))


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def ps_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("psisa") / "ps.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_path_support.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel", ["k_ps_build", "k_ps_score"])
def test_path_support_kernels_without_scratch(ps_isa, kernel):
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"E\w*)\n", ps_isa):
        a = ps_isa.rfind("\n  - ", 0, m.start())
        b = ps_isa.find("\n  - ", m.end())
        entries.append(ps_isa[a:b if b >= 0 else len(ps_isa)])
    assert len(entries) == 1, kernel
    field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))
    print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("wavefront_size") == 64
    if kernel == "k_ps_score":  # one wave per alignment; two 32-bit sums per path in LDS
        assert field("max_flat_workgroup_size") == 64 and field("group_segment_fixed_size") == 2 * 4 * 4096
