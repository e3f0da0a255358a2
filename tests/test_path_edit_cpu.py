"""Path edit, the parts that need no GPU: the reference's two distances against each other and against the definition, the window
arithmetic of csrc/vga_path_edit.hpp compiled with a host compiler, the calls in the ABI, the binding's methods and constants, the
command line's refusals, the measure on the oracle's alignments GAF of three DRB1 samples, and the register budget of k_pe_dist from
a cross-compile for gfx950."""
import glob
import os
import random
import re
import subprocess

import numpy as np
import pytest

import genotype_lik_ref
import path_edit_ref as ref
from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_path_edit_begin", "vga_path_edit_read", "vga_path_edit_last", "vga_path_edit_reset", "vga_path_edit_end", "vga_path_edit_pairs",
         "vga_genotype_lik_source"]


# ---- the reference
def test_reference_distances_agree_with_the_definition_on_tiny_inputs():
    rng = random.Random(1)
    for _ in range(400):
        q = "".join(rng.choice("ACGTNa") for _ in range(rng.randrange(0, 7)))
        t = "".join(rng.choice("ACGTNc") for _ in range(rng.randrange(0, 9)))
        assert ref.brute_distance(q, t) == ref.dp_distance(q, t) == ref.myers_distance(q, t), (q, t)
    assert ref.brute_distance("ACGT", "") == 4 and ref.brute_distance("", "ACGT") == 0 and ref.brute_distance("N", "N") == 1
    assert ref.brute_distance("acg", "TTACGTT") == 0 and ref.brute_distance("GGA", "ACC") == 2


@pytest.mark.parametrize("m,n", [(1, 1), (63, 64), (64, 63), (65, 300), (129, 5), (200, 700), (700, 200)])
def test_reference_distances_agree_with_each_other(m, n):
    rng = random.Random(m * 1000 + n)
    for alphabet in ("ACGT", "ACGTNacgtn", "AC"):
        q = "".join(rng.choice(alphabet) for _ in range(m))
        t = "".join(rng.choice(alphabet) for _ in range(n))
        if n > m:
            at = rng.randrange(0, n - m)
            t = t[:at] + "".join(c for c in q if rng.random() > 0.08) + t[at + m:]
        e = ref.myers_distance(q, t)
        assert e == ref.dp_distance(q, t) and 0 <= e <= m, (m, n, alphabet)


def test_reference_window_rule():
    node_seq = {1: "AAAA", 2: "CC", 3: "GGG", 4: "T"}
    steps = [(1, False), (2, False), (3, True), (2, False), (4, False)]
    seq, pos = ref.path_sequence(steps, node_seq)
    assert seq == "AAAACCCCCCCT" and pos == [0, 4, 6, 9, 11]
    win = lambda nodes, m: ref.window(nodes, steps, pos, node_seq, m, len(seq))
    assert win([3], 5) is None                        # only an "id-" step
    assert win([9, 3], 5) is None
    assert win([2], 1) == (3, 12)                     # i: the first step of node 2, j: its last; hi = 9 + 2 + 1
    assert win([1, 2], 2) == (0, 12)                  # lo clamps at 0, hi at |seq_p|
    assert win([4, 1], 1) is None                     # a = 4 (step 4), b = 1 (step 0): j < i
    assert win([3, 2, 4], 3) == (1, 12)               # node 3 is skipped: a = 2 (step 1), b = 4


# ---- the header host and device share
def test_header_arithmetic_with_a_host_compiler(tmp_path):
    rng = random.Random(5)
    cases = [(0, 0, 1, 1, 1), (5, 5, 3, 9, 8), (0xFFFFFF00, 0xFFFFFFF0, 15, 0xFFFFFFFF, 0xFFFFFFFF)]
    for _ in range(200):
        seq_len = rng.randrange(1, 1 << rng.randrange(1, 32))
        pos_i = rng.randrange(0, seq_len)
        pos_j = rng.randrange(pos_i, seq_len)
        cases.append((pos_i, pos_j, rng.randrange(1, seq_len - pos_j + 1), rng.randrange(1, 1 << rng.randrange(1, 20)), seq_len))
    ms = [0, 1, 63, 64, 65, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384, 16385, 100000]
    src = tmp_path / "pe.cpp"
    src.write_text('#include "vga_path_edit.hpp"\n#include <cstdio>\nint main() {\n'
                   + "".join('  { pe_window w = pe_window_of(%uu, %uu, %uu, %uu, %uu); printf("W %%u %%u\\n", w.lo, w.hi); }\n' % c for c in cases)
                   + "".join('  printf("M %%u %%u %%u %%llu\\n", pe_blocks(%uu), pe_blocks_per_lane(%uu), pe_blocks_per_lane(%uu) ? pe_lanes(%uu, pe_blocks_per_lane(%uu)) : 0u, '
                             'pe_blocks_per_lane(%uu) ? (unsigned long long)pe_steps(%uu, pe_blocks_per_lane(%uu), 1000u) : 0ull);\n' % ((m,) * 8) for m in ms)
                   + '  for (int c = 0; c < 256; c++) printf("C %u %u\\n", pe_code((unsigned char)c), pe_code_complement(pe_code((unsigned char)c)));\n'
                   + '  printf("K %u %u %u %u\\n", PE_NONE, PE_MAX_R, PE_MAX_QUERY, PE_CODE_OTHER);\n  return 0;\n}\n')
    exe = str(tmp_path / "pe")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    W = [tuple(int(x) for x in l.split()[1:]) for l in out if l[0] == "W"]
    assert W == [(max(0, i - m), min(s, j + lb + m)) for i, j, lb, m, s in cases]
    M = [tuple(int(x) for x in l.split()[1:]) for l in out if l[0] == "M"]
    for m, (nb, R, lanes, steps) in zip(ms, M):
        assert nb == (m + 63) // 64
        assert R == (1 if nb <= 64 else 2 if nb <= 128 else 4 if nb <= 256 else 0), m
        if R:
            assert lanes == (nb + R - 1) // R <= 64 and steps == 1000 + lanes - 1, m
    Cc = [tuple(int(x) for x in l.split()[1:]) for l in out if l[0] == "C"]
    for c, (code, comp) in enumerate(Cc):
        want = ref.code(chr(c))
        assert code == (want if want >= 0 else 4), c
        assert comp == (3 - want if want >= 0 else 4), c
    b = pkg().binding
    assert [int(x) for x in [l for l in out if l[0] == "K"][0].split()[1:]] == [b.PATH_EDIT_NONE, b.PATH_EDIT_MAX_R, b.PATH_EDIT_MAX_QUERY, 4]
    assert b.PATH_EDIT_NONE == ref.NONE and b.PATH_EDIT_MAX_QUERY == ref.LIMIT == 16384


# ---- the ABI and the binding
def test_abi_lists_and_exports_the_calls():
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert re.search(r"#define\s+VGA_GL_FROM_SUPPORT\s+0u", header) and re.search(r"#define\s+VGA_GL_FROM_EDIT\s+1u", header)
    assert L.vga_abi_version() == 6


def test_null_context():
    L = pkg().binding.load_library()
    assert L.vga_path_edit_begin(None) == -1 and L.vga_path_edit_reset(None) == -1 and L.vga_path_edit_end(None) == -1
    assert L.vga_path_edit_read(None, None, None, None, None, None, None) == -1
    assert L.vga_path_edit_last(None, 0, None) == -1
    assert L.vga_path_edit_pairs(None, 0, None, None, None, None, None) == -1
    assert L.vga_genotype_lik_source(None, 0) == -1


def test_binding_has_the_methods_and_the_kernel_s_constants():
    b = pkg().binding
    for name in ("path_edit_begin", "path_edit", "path_edit_last", "path_edit_reset", "path_edit_end", "path_edit_pairs"):
        assert callable(getattr(b.Context, name)), name
    import inspect
    assert inspect.signature(b.Context.genotype_likelihood_begin).parameters["source"].default == "support"
    assert (b.VGA_GL_FROM_SUPPORT, b.VGA_GL_FROM_EDIT) == (0, 1) and b.GENOTYPE_LIK_SOURCES == {"support": 0, "edit": 1}
    hpp = open(os.path.join(CSRC, "vga_path_edit.hpp")).read()
    assert int(re.search(r"#define\s+PE_MAX_R\s+(\d+)u", hpp).group(1)) == b.PATH_EDIT_MAX_R
    assert re.search(r"#define\s+PE_MAX_QUERY\s+\(64u \* 64u \* PE_MAX_R\)", hpp) and b.PATH_EDIT_MAX_QUERY == 64 * 64 * b.PATH_EDIT_MAX_R
    assert re.search(r"#define\s+PE_NONE\s+0xFFFFFFFFu", hpp)


# ---- the measure on the oracle's text
@pytest.fixture(scope="module")
def drb1_reads(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    _, paths = ref.parse_gfa(DRB1)
    reads = pkg().readsim.simulate_reads(DRB1, 120, 3000, 0.03, 0.03, 0.04, seed=7)
    names = [p[0] for p in paths]
    return ix, [(names.index(r.path), r) for r in reads]


# (sample, reads, the rank-1 pair and its cost, the runner-up and its cost) under the rule as include/vga_hip.h words it, from
# tests/path_edit_ref.py through tests/genotype_lik_ref.py at lambda 512, cap 64
SAMPLES = [((2, 5), 26, (2, 5, 6656), (3, 5, 7680)), ((4, 9), 19, (4, 9, 5376), (1, 9, 9472)), ((3,), 13, (3, 3, 0), (2, 3, 234))]


@pytest.mark.parametrize("keep,n_reads,first,second", SAMPLES, ids=["paths 2 and 5", "paths 4 and 9", "path 3"])
def test_sample_is_called_from_the_edit_distance(oracle, drb1_reads, keep, n_reads, first, second):
    ix, reads = drb1_reads
    sel = [r for p, r in reads if p in keep]
    assert len(sel) == n_reads
    _, ag, _ = oracle.map_reads(ix, [r.name for r in sel], [r.seq for r in sel])
    w = ref.walk(ag, [r.seq for r in sel], DRB1)
    assert w["n_alignments"] == n_reads and w["n_too_long"] == 0
    assert (w["edit"][:, 6] == ref.NONE).all()  # path 6 has only "id-" steps
    T = pkg().binding.genotype_likelihood_table(512, 64)
    t = genotype_lik_ref.pairs(*ref.likelihood_matrices(w), 512, 64, T)
    ranked = genotype_lik_ref.rank(t["cost"], 12)
    print(keep, n_reads, "reads; best", ranked[0], "then", ranked[1], "residual min e / m per read:",
          ["%.3f" % (w["edit"][r][w["edit"][r] != ref.NONE].min() / w["lengths"][r]) for r in range(n_reads)][:6])
    assert ranked[0][:3] == first and ranked[1][:3] == second, (ranked[0], ranked[1])
    # a few cells through the second distance
    rng = random.Random(7)
    wins, seqs = ref.windows(ag, [r.seq for r in sel], DRB1)
    for _ in range(3):
        r, p = rng.randrange(n_reads), rng.choice([x for x in range(12) if x != 6])
        if wins[r][1][p] is not None:
            lo, hi = wins[r][1][p]
            assert ref.dp_distance(wins[r][0], seqs[p][lo:hi]) == w["edit"][r, p]


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300, env=env)


def test_cli_path_edit_needs_also_align(tmp_path):
    pkg()
    pr = run_cli(["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--path-edit", "-o", str(tmp_path / "o")], tmp_path)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and "--path-edit" in pr.stderr, pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


@pytest.mark.parametrize("extra,says", [(["--genotype-from", "edit"], "--genotype-likelihood"),
                                        (["--genotype-likelihood", "--genotype-from", "bases"], "edit or support"),
                                        (["--genotype-likelihood", "--genotype-from", ""], "edit or support"),
                                        (["--genotype", "--genotype-from", "support"], "--genotype-likelihood")])
def test_cli_refuses_a_genotype_from_without_meaning(tmp_path, extra, says):
    pkg()
    pr = run_cli(["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--also-align", "-G", DRB1, "-o", str(tmp_path / "o")] + extra,
                 tmp_path)
    assert pr.returncode != 0 and "--genotype-from" in pr.stderr and says in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


def test_cli_refuses_a_graph_without_paths_or_of_another_index(tmp_path):
    pkg()
    gfa = os.path.join(DATA, "test.gfa")
    pr = subprocess.run([EXE, "index", "-i", gfa, "-k", "11", "-o", str(tmp_path / "t")], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    (tmp_path / "r.fa").write_text(">r\nACGTACGTACGT\n")
    bare = tmp_path / "bare.gfa"
    bare.write_text("".join(ln for ln in open(gfa) if not ln.startswith("P")))
    common = ["map", "-i", str(tmp_path / "t"), "-f", str(tmp_path / "r.fa"), "-p", "abpoa", "--also-align", "--path-edit"]
    pr = run_cli(common + ["-G", str(bare), "-o", str(tmp_path / "o1")], tmp_path)
    assert pr.returncode != 0 and "no P line" in pr.stderr and "--path-edit" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr  # (refused before a context was asked for)
    pr = run_cli(common + ["-G", DRB1, "-o", str(tmp_path / "o2")], tmp_path)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o1*")) and not glob.glob(str(tmp_path / "o2*"))


def test_usage_names_the_switches():
    pkg()
    pr = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--path-edit" in pr.stderr and "--genotype-from" in pr.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def pe_build(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("peisa") / "pe.s")
    pr = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "vga_path_edit.hip"), "-o", out], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-2000:]
    return pr.stderr, open(out).read()


def test_distance_kernel_without_scratch_or_spills(pe_build):
    remarks, isa = pe_build
    usage = {}
    name = None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if m and name:
            usage[name][m.group(1).strip()] = int(m.group(2))
    dist = {n: u for n, u in usage.items() if "k_pe_dist" in n}
    assert len(dist) == 3 and len([n for n in usage if "k_pe_" in n]) == 7, sorted(usage)
    for n, u in usage.items():
        print(n, u)
        assert u["ScratchSize"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (n, u)
    # Pv, Mv and four masks per block are 12 registers per block: R = 4 stays well inside the 128 that keep 4 waves on a SIMD
    assert max(u["VGPRs"] for u in dist.values()) <= 96
    # the hand-over between lanes is a wave shift, not a trip through LDS
    assert isa.count("wave_shr:1") == 3
