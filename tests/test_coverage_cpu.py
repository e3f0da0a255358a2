"""Read coverage, the parts that need no GPU: the reference walker (tests/coverage_ref.py) checked on the oracle's alignments
GAF, the four vga_coverage_* calls in the ABI, the command line's refusal of --coverage without --also-align, and the register
and scratch budget of k_cov_runs / k_cov_add from a cross-compile for gfx950."""
import os
import re
import subprocess

import pytest

import coverage_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_coverage_begin", "vga_coverage_read", "vga_coverage_reset", "vga_coverage_end"]


# ---- the walker on the oracle's text
@pytest.mark.parametrize("k", [11, 19])
def test_walker_on_the_oracle_gaf(oracle, k):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), k)
    reads = pkg().readsim.simulate_reads(DRB1, 12, 3000, 0.03, 0.03, 0.04, seed=7)
    _, ag, _ = oracle.map_reads(ix, [r.name for r in reads], [r.seq for r in reads])
    a = oracle_index_arrays(ix)
    # (walk asserts per record: it ends at path_end on the last path node, and covers block_length bases)
    base, node, edge, n_al = coverage_ref.walk(ag, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])
    recs = coverage_ref.records(ag)
    assert n_al == len(recs) == len(reads)
    assert len(base) == len(a["seq_fwd"]) and len(node) == len(a["node_seq_idx"]) - 1 and len(edge) == len(a["edges"])
    assert int(base.sum()) == sum(int(ln.split("\t")[10]) for ln in ag.splitlines() if ln.split("\t")[5] != "*") > 0
    assert int(node.max()) <= n_al and int(base.max()) <= n_al
    assert int(node.sum()) == sum(len(r[0]) for r in recs)
    assert int(edge.sum()) == sum(len(r[0]) - 1 for r in recs)
    out = coverage_ref.outgoing_slots(a["node_edge_idx"], a["node_edges_to"], len(a["edges"]))
    assert not edge[~out].any(), "only outgoing slots count"


def test_walker_token_effects():
    """one hand-made record on a two-node graph: a match run over the node boundary, a mismatch, a deletion, an insertion"""
    # nodes 1 (4 bases) and 2 (5 bases); edges: node 1 has one outgoing slot (-> 2), node 2 one incoming (<- 1)
    node_seq_idx, node_edge_idx, node_edges_to, edges = [0, 4, 9], [0, 1, 2], [0, 1, 0], [4, 2]
    cs = ":3*ag-cc+tt:2"  # 3 matches (node 1: 1..3), mismatch (node 2: 0), deletion (node 2: 1..2), insertion, 2 matches (node 2: 3..4)
    line = "\t".join(["r", "9", "0", "9", "+", ">1>2", "8", "1", "5", "6", "6", "255", "as:i:-30 cs:Z:" + cs + ",cg:Z:4M2D2I2M"])
    base, node, edge, n = coverage_ref.walk(line + "\n" + "\t".join(["q", "5", "0", "5", "+", "*", "0", "0", "0", "0", "0", "255", "x"]) + "\n",
                                            node_seq_idx, node_edge_idx, node_edges_to, edges)
    assert base.tolist() == [0, 1, 1, 1, 1, 0, 0, 1, 1] and node.tolist() == [1, 1] and edge.tolist() == [1, 0] and n == 1


# ---- the ABI
def test_abi_lists_and_exports_the_four_calls():
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    assert L.vga_coverage_begin(None) == -1 and L.vga_coverage_read(None, None, None, None, None) == -1
    assert L.vga_coverage_reset(None) == -1 and L.vga_coverage_end(None) == -1


def test_no_device_no_context():
    import sys

    # asked in a child process: the GPU runtime is not initialised inside the test process
    probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.is_available())"], capture_output=True, text=True,
                           timeout=300, check=True)
    if probe.stdout.strip().splitlines()[-1] == "True":
        pytest.skip("GPU present")
    with pytest.raises(pkg().VgaError) as e:
        pkg().Context(0)
    assert e.value.code == -6  # VGA_ERR_NO_DEVICE: the coverage calls brought no CPU path with them


# ---- the command line
@pytest.mark.parametrize("flag", ["--coverage", "--coverage-only"])
def test_cli_coverage_needs_also_align(tmp_path, flag):
    pkg()
    pr = subprocess.run([EXE, "map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", flag],
                        cwd=str(tmp_path), capture_output=True, text=True, timeout=120)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and flag in pr.stderr, pr.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def cov_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("covisa") / "cov.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_coverage.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel", ["k_cov_runs", "k_cov_add", "k_cov_depth"])
def test_coverage_kernels_without_scratch(cov_isa, kernel):
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"E\w*)\n", cov_isa):
        a = cov_isa.rfind("\n  - ", 0, m.start())
        b = cov_isa.find("\n  - ", m.end())
        entries.append(cov_isa[a:b if b >= 0 else len(cov_isa)])
    assert len(entries) == 1, kernel
    field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))
    print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("wavefront_size") == 64
    if kernel != "k_cov_depth":
        assert field("group_segment_fixed_size") == 0 and field("max_flat_workgroup_size") == 64  # one wave per problem / alignment
