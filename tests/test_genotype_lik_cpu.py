"""The diploid read likelihood, the parts that need no GPU: the six vga_genotype_lik_* calls in the ABI, the binding's methods and
constants, the library's table T against numpy's float evaluation, the reference (tests/genotype_lik_ref.py) and the ranking on
hand-made matrices and on the oracle's alignments GAF (the four DRB1 samples of tests/test_genotype_cpu.py, where this model calls
the homozygous sample without a tie rule), the command line's refusals, and the scratch budget of k_gl_deficit and k_gl_pairs
from a cross-compile for gfx950."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import genotype_lik_ref as ref
import path_support_ref
from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CTX_CALLS = ["vga_genotype_lik_begin", "vga_genotype_lik_read", "vga_genotype_lik_reset", "vga_genotype_lik_end", "vga_genotype_lik_pairs"]
LAM, CAP = 512, 64


# ---- the ABI and the binding
def test_abi_lists_and_exports_the_six_calls():
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CTX_CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert "vga_genotype_lik_table" in p.binding.ABI_SYMBOLS and L.vga_genotype_lik_table is not None
    assert re.search(r"\bint\s+vga_genotype_lik_table\s*\(\s*uint32_t\s+lambda\s*,\s*uint32_t\s+cap\s*,\s*uint32_t\s*\*", header)
    assert L.vga_abi_version() == 6
    for name in ("vga_genotype_begin", "vga_genotype_read", "vga_genotype_reset", "vga_genotype_end", "vga_genotype_pairs"):
        assert name in p.binding.ABI_SYMBOLS, name  # (the five calls of --genotype stay)


def test_null_context():
    L = pkg().binding.load_library()
    assert L.vga_genotype_lik_begin(None, LAM, CAP) == -1 and L.vga_genotype_lik_reset(None) == -1 and L.vga_genotype_lik_end(None) == -1
    assert L.vga_genotype_lik_read(None, 0, None, None) == -1
    assert L.vga_genotype_lik_pairs(None, 0, 1, None, None, LAM, CAP, None, None, None) == -1


def test_binding_has_the_methods_and_the_kernel_s_constants():
    b = pkg().binding
    for name in ("genotype_likelihood_begin", "genotype_likelihood", "genotype_likelihood_reset", "genotype_likelihood_end", "genotype_likelihood_pairs"):
        assert callable(getattr(b.Context, name)), name
    assert callable(b.genotype_likelihood_table) and callable(b.genotype_likelihood_rank)
    hpp = open(os.path.join(CSRC, "vga_genotype_lik.hpp")).read()
    define = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u", hpp).group(1))
    assert (b.GENOTYPE_LIK_TILE, b.GENOTYPE_LIK_READS, b.GENOTYPE_LIK_MIN_CHUNKS, b.GENOTYPE_LIK_MAX_GROUP_READS, b.GENOTYPE_LIK_MAX_PATHS,
            b.GENOTYPE_LIK_MAX_LAMBDA, b.GENOTYPE_LIK_MAX_CAP) == (
        define("GL_TILE"), define("GL_READS"), define("GL_MIN_CHUNKS"), define("GL_MAX_GROUP_READS"), define("GL_MAX_PATHS"), define("GL_MAX_LAMBDA"),
        define("GL_MAX_CAP"))
    assert (b.GENOTYPE_LIK_LAMBDA, b.GENOTYPE_LIK_CAP) == (LAM, CAP)
    # the flush interval of the 32-bit accumulators, from the largest cost of one read (they hold twice the cost)
    per_read = 4096 * 255 + 256
    assert b.GENOTYPE_LIK_MAX_GROUP_READS * 2 * per_read < 1 << 32 and b.GENOTYPE_LIK_MAX_GROUP_READS % b.GENOTYPE_LIK_READS == 0


# ---- the table
@pytest.mark.parametrize("lam", [1, 128, 256, 512, 1024, 4096])
def test_table_against_numpy(lam):
    b = pkg().binding
    T = b.genotype_likelihood_table(lam, 255)
    assert T.dtype == np.uint32 and T.shape == (256,)
    assert T[0] == 0 and np.all(np.diff(T.astype(np.int64)) >= 0) and T.max() <= 256
    want = ref.table_float(lam, 255)
    off = np.abs(T.astype(np.int64) - want)
    print("lambda", lam, "T[1..4]", T[1:5].tolist(), "T[255]", int(T[255]), "largest |library - numpy|", int(off.max()))
    assert off.max() <= 1
    # a shorter table is the head of the longer one
    assert np.array_equal(b.genotype_likelihood_table(lam, 64), T[:65]) and np.array_equal(b.genotype_likelihood_table(lam, 1), T[:2])


def test_table_header_with_a_host_compiler(tmp_path):
    """csrc/vga_genotype_lik.hpp is the one definition: compiled alone by a host compiler it prints the library's table"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "vga_genotype_lik.hpp"\n#include <cstdio>\nint main() { uint32_t t[256]; vga_gl_table(512, 64, t); '
                   'for (int x = 0; x <= 64; x++) printf("%u\\n", t[x]); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out] == pkg().binding.genotype_likelihood_table(512, 64).tolist()


def test_table_refuses_bad_arguments():
    p = pkg()
    L = p.binding.load_library()
    buf = (ctypes.c_uint32 * 300)()
    for lam, cap in ((0, 64), (4097, 64), (512, 0), (512, 256), (1 << 31, 64)):
        assert L.vga_genotype_lik_table(lam, cap, buf) == -1, (lam, cap)
        with pytest.raises(p.VgaError) as e:
            p.binding.genotype_likelihood_table(lam, cap)
        assert e.value.code == -1
    assert L.vga_genotype_lik_table(512, 64, None) == -1
    assert L.vga_genotype_lik_table(4096, 255, buf) == 0 and L.vga_genotype_lik_table(1, 1, buf) == 0


# ---- the reference and the ranking on hand-made matrices
def test_reference_on_hand_made_matrices():
    b = pkg().binding
    lam, cap = 256, 4
    T = b.genotype_likelihood_table(lam, cap)
    t = [int(x) for x in T]
    #         path 0  1  2  3
    bases = [[7, 3, 10, 0],     # r0: s = 10 everywhere, a full tie: d = 0, costs nothing
             [0, 0, 0, 0],      # r1: all zero: d = 0, costs nothing, is not scored
             [15, 9, 16, 5]]    # r2: s = 20, 17, 16, 15: deficits cap - 1, cap, and cap + 1 capped to cap
    edges = [[3, 7, 0, 10],
             [0, 0, 0, 0],
             [5, 8, 0, 10]]
    got = ref.pairs(bases, edges, lam, cap, T)
    assert got["deficit"].tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 3, 4, 4]] and got["n_scored"] == 2 and got["n_paths"] == 4
    at = lambda p, q: ref.pair_index(4, p, q)
    cost = lambda p, q: int(got["cost"][at(p, q)])
    assert [at(0, 0), at(0, 1), at(0, 2), at(0, 3), at(1, 1), at(1, 2), at(1, 3), at(2, 2), at(2, 3), at(3, 3)] == list(range(10))
    assert cost(0, 0) == 0 and cost(0, 1) == t[3] and cost(0, 2) == t[4] == cost(0, 3)
    assert cost(1, 1) == 3 * lam and cost(1, 2) == 3 * lam + t[1] == cost(1, 3)
    assert cost(2, 2) == 4 * lam == cost(2, 3) == cost(3, 3)  # (T[0] = 0: two alleles that fit equally badly cost what one does)
    assert 0 < t[1] <= t[3] <= t[4] <= 256 < 3 * lam
    ranked = ref.rank(got["cost"], 4)
    # cost, then the homozygous pair first -- (2, 2) and (3, 3) before (2, 3) --, then p, then q
    assert [(p, q) for p, q, _, _ in ranked] == [(0, 0), (0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (1, 3), (2, 2), (3, 3), (2, 3)]
    assert [m for _, _, _, m in ranked] == [c for _, _, c, _ in ranked] and ranked[1][2] == t[3]
    assert b.genotype_likelihood_rank(got["cost"], 4) == ranked and b.genotype_likelihood_rank(got["cost"], 4, 3) == ranked[:3] == ref.rank(got["cost"], 4, 3)
    # a full tie: every pair costs 0, the homozygous pairs come first
    tie = ref.pairs([[4, 4, 4]], [[1, 1, 1]], lam, cap, T)
    assert not tie["cost"].any() and tie["n_scored"] == 1
    assert [(p, q) for p, q, _, _ in ref.rank(tie["cost"], 3)] == [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
    assert b.genotype_likelihood_rank(tie["cost"], 3) == ref.rank(tie["cost"], 3)
    # the margin is over the first pair, whatever its cost
    c = np.array([9, 7, 8], dtype=np.uint64)
    assert ref.rank(c, 2) == [(0, 1, 7, 0), (1, 1, 8, 1), (0, 0, 9, 2)] == b.genotype_likelihood_rank(c, 2)
    # s above 32 bits, and no read at all
    big = ref.pairs([[0xFFFFFFFF, 0, 0xFFFFFFFE]], [[0xFFFFFFFF, 0, 0xFFFFFFFF]], lam, cap, T)
    assert big["deficit"].tolist() == [[0, 4, 1]] and int(big["cost"][ref.pair_index(3, 1, 2)]) == lam + t[3]
    none = ref.pairs(np.zeros((0, 3)), np.zeros((0, 3)), lam, cap, T)
    assert none["cost"].tolist() == [0] * 6 and none["n_scored"] == 0


def test_rank_keeps_64_bits():
    big = 1 << 63
    c = np.array([big + 1, big, 5], dtype=np.uint64)
    want = [(1, 1, 5, 0), (0, 1, big, big - 5), (0, 0, big + 1, big - 4)]
    assert ref.rank(c, 2) == want == pkg().binding.genotype_likelihood_rank(c, 2)


# ---- the model on the oracle's text
@pytest.fixture(scope="module")
def drb1_reads(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    reads = pkg().readsim.simulate_reads(DRB1, 120, 3000, 0.03, 0.03, 0.04, seed=7)
    names = [p[0] for p in paths]
    return ix, node_len, paths, [(names.index(r.path), r) for r in reads]


def ranked_of(oracle, drb1_reads, keep):
    """the reads of the paths in `keep`, ranked with the library's table and with numpy's"""
    ix, node_len, paths, reads = drb1_reads
    sel = [r for p, r in reads if p in keep]
    _, ag, _ = oracle.map_reads(ix, [r.name for r in sel], [r.seq for r in sel])
    w = path_support_ref.walk(ag, node_len, paths)
    lib = ref.pairs(w["bases"], w["edges"], LAM, CAP, pkg().binding.genotype_likelihood_table(LAM, CAP))
    flt = ref.pairs(w["bases"], w["edges"], LAM, CAP, ref.table_float(LAM, CAP))
    assert lib["n_scored"] == len(sel) == flt["n_scored"]
    return len(sel), ref.rank(lib["cost"], 12), ref.rank(flt["cost"], 12)


@pytest.mark.parametrize("pair,n_reads,best,second", [((2, 5), 26, 7680, 11264), ((4, 9), 19, 5888, 22784)], ids=["paths 2 and 5", "paths 4 and 9"])
def test_heterozygous_sample_is_called(oracle, drb1_reads, pair, n_reads, best, second):
    n, lib, flt = ranked_of(oracle, drb1_reads, set(pair))
    print(n, "reads; library's table:", lib[:4], "numpy's table:", flt[:4])
    assert n == n_reads
    assert lib[0] == (pair[0], pair[1], best, 0)
    assert lib[1][2] == second == lib[2][2] and lib[3][2] > second  # (two pairs share the second place)
    assert lib[1][3] == second - best
    assert pkg().binding.genotype_likelihood_rank(np.array([c for _, _, c, _ in sorted(lib)], dtype=np.uint64), 12, 5) == lib[:5]


def test_homozygous_sample_is_called_without_a_tie_rule(oracle, drb1_reads):
    n, lib, flt = ranked_of(oracle, drb1_reads, {3})
    print(n, "reads; library's table:", lib[:4], "numpy's table:", flt[:4])
    assert n == 13
    assert lib[0] == (3, 3, 0, 0)
    assert lib[1] == (2, 3, 174, 174) and lib[2] == (2, 2, 512, 512)
    assert lib[1][2] > lib[0][2]  # strictly cheaper than rank 2: --genotype's measure ties them


def test_identical_paths_tie(oracle, drb1_reads):
    n, lib, flt = ranked_of(oracle, drb1_reads, {0, 1})
    print(n, "reads; library's table:", lib[:6], "numpy's table:", flt[:6])
    assert n == 20
    assert [(p, q) for p, q, _, _ in lib[:4]] == [(0, 1), (0, 7), (1, 8), (7, 8)]
    assert [c for _, _, c, _ in lib[:4]] == [37632] * 4 and lib[4][2] > 37632


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300, env=env)


def base_args(tmp_path):
    return ["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "-o", str(tmp_path / "o")]


def test_cli_needs_also_align(tmp_path):
    pkg()
    pr = run_cli(base_args(tmp_path) + ["--genotype-likelihood"], tmp_path)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and "--genotype-likelihood" in pr.stderr, pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


@pytest.mark.parametrize("flag", ["--genotype-lambda", "--genotype-cap"])
def test_cli_refuses_a_parameter_without_the_switch(tmp_path, flag):
    pkg()
    for extra in ([], ["--genotype"]):
        pr = run_cli(base_args(tmp_path) + ["--also-align", "-G", DRB1, flag, "32"] + extra, tmp_path)
        assert pr.returncode != 0 and flag in pr.stderr and "--genotype-likelihood" in pr.stderr, pr.stderr
        assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


@pytest.mark.parametrize("flag,value", [("--genotype-lambda", "0"), ("--genotype-lambda", "4097"), ("--genotype-lambda", "-1"), ("--genotype-lambda", "many"),
                                        ("--genotype-lambda", ""), ("--genotype-cap", "0"), ("--genotype-cap", "256"), ("--genotype-cap", "6.5"),
                                        ("--genotype-top", "-1")])
def test_cli_refuses_a_value_out_of_range(tmp_path, flag, value):
    pkg()
    pr = run_cli(base_args(tmp_path) + ["--also-align", "-G", DRB1, "--genotype-likelihood", flag, value], tmp_path)
    assert pr.returncode != 0 and flag in pr.stderr, pr.stderr
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
    common = ["map", "-i", str(tmp_path / "t"), "-f", str(tmp_path / "r.fa"), "-p", "abpoa", "--also-align", "--genotype-likelihood"]
    pr = run_cli(common + ["-G", str(bare), "-o", str(tmp_path / "o1")], tmp_path)
    assert pr.returncode != 0 and "no P line" in pr.stderr and "--genotype-likelihood" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr  # (refused before a context was asked for)
    pr = run_cli(common + ["-G", DRB1, "-o", str(tmp_path / "o2")], tmp_path)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o1*")) and not glob.glob(str(tmp_path / "o2*"))


def test_usage_names_the_switches():
    pkg()
    pr = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    for flag in ("--genotype-likelihood", "--genotype-lambda", "--genotype-cap"):
        assert flag in pr.stderr, flag


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def gl_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("glisa") / "gl.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_genotype_lik.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_entry(isa, kernel):
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"E\w*)\n", isa):
        a = isa.rfind("\n  - ", 0, m.start())
        z = isa.find("\n  - ", m.end())
        entries.append(isa[a:z if z >= 0 else len(isa)])
    assert len(entries) == 1, kernel
    return lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))


def test_kernels_without_scratch(gl_isa):
    b = pkg().binding
    for kernel in ("k_gl_deficit", "k_gl_pairs"):
        field = kernel_entry(gl_isa, kernel)
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0, kernel
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0, kernel
        assert field("wavefront_size") == 64 and field("max_flat_workgroup_size") == 256, kernel
    # k_gl_pairs: two staged arrays of one 16-bit doubled deficit per read and path, and the 256 16-bit entries of the table;
    # at most 128 registers would be a fourth wave per SIMD, 168 is what k_gt_pairs takes
    field = kernel_entry(gl_isa, "k_gl_pairs")
    assert field("group_segment_fixed_size") == 2 * b.GENOTYPE_LIK_READS * b.GENOTYPE_LIK_TILE * 2 + 256 * 2
    assert field("vgpr_count") <= 168
    assert kernel_entry(gl_isa, "k_gl_deficit")("group_segment_fixed_size") == 0
    # the costs are combined with 64-bit vector atomics
    assert "global_atomic_add_x2" in gl_isa
