"""The path abundance, the parts that need no GPU: the seven vga_path_abundance* calls in the ABI and the header, the binding's
constants against the #defines of csrc/vga_abundance.hpp, the table W (its properties, numpy's float evaluation, the header compiled
alone with a host compiler, the refusals), the reference (tests/path_abundance_ref.py) on hand-made rows and against the header's own
host iteration in a stand-alone program (once more under the host sanitizers), the four DRB1 samples of tests/test_genotype_lik_cpu.py
on the oracle's alignments GAF, the command line's refusals and usage text, and the resource fields of the kernels from a
cross-compile for gfx950.  Without the feature every test here stops at the missing header, binding call, symbol, switch or kernel."""
import ctypes
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import path_abundance_ref as ref
import path_support_ref
from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_path_abundance_table", "vga_path_abundance_begin", "vga_path_abundance_reset", "vga_path_abundance_end", "vga_path_abundance_store",
         "vga_path_abundance", "vga_path_abundance_rows"]
LAM, CAP = 512, 64


def binding():
    b = pkg().binding
    assert hasattr(b, "path_abundance_table"), "the binding has no path abundance"
    return b


# ---- 1. the ABI, the header and the binding
def test_abi_lists_and_exports_the_calls():
    p = pkg()
    b = binding()
    L = b.load_library()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    for name in CALLS:
        assert name in b.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    for name in ("path_abundance_begin", "path_abundance_reset", "path_abundance_end", "path_abundance_store", "path_abundance", "path_abundance_rows"):
        assert callable(getattr(p.Context, name)), name
    assert callable(b.path_abundance_table) and callable(b.path_abundance_ppm)


def test_header_declares_the_calls(tmp_path):
    src = tmp_path / "decl.c"
    outs = "uint32_t *, uint64_t *, uint64_t *, uint64_t *, uint32_t *, uint32_t *"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*a)(uint32_t, uint32_t, uint32_t *) = vga_path_abundance_table;\n"
                   "int (*b)(vga_ctx *, uint32_t, uint32_t) = vga_path_abundance_begin;\n"
                   "int (*c)(vga_ctx *) = vga_path_abundance_reset;\n"
                   "int (*d)(vga_ctx *) = vga_path_abundance_end;\n"
                   "int (*e)(vga_ctx *, uint64_t, uint8_t *, uint8_t *, uint64_t *) = vga_path_abundance_store;\n"
                   "int (*f)(vga_ctx *, uint32_t, uint32_t, uint32_t, " + outs + ") = vga_path_abundance;\n"
                   "int (*g)(vga_ctx *, uint64_t, uint32_t, const uint8_t *, const uint8_t *, uint32_t, uint32_t, uint32_t, " + outs + ") = vga_path_abundance_rows;\n"
                   "int s = VGA_AB_FROM_SUPPORT + VGA_AB_FROM_EDIT;\n")
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "decl.o")])


def test_null_context():
    L = binding().load_library()
    assert L.vga_path_abundance_begin(None, CAP, 0) == -1 and L.vga_path_abundance_reset(None) == -1 and L.vga_path_abundance_end(None) == -1
    assert L.vga_path_abundance_store(None, 0, None, None, None) == -1
    assert L.vga_path_abundance(None, LAM, 1000, 16, None, None, None, None, None, None) == -1
    assert L.vga_path_abundance_rows(None, 0, 1, None, None, LAM, 1000, 16, None, None, None, None, None, None) == -1


def test_binding_constants_equal_the_header_s():
    b = binding()
    hpp = open(os.path.join(CSRC, "vga_abundance.hpp")).read()
    define = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u(?:ll)?\s", hpp).group(1))
    assert (b.PATH_ABUNDANCE_LAMBDA, b.PATH_ABUNDANCE_MAX_LAMBDA, b.PATH_ABUNDANCE_CAP, b.PATH_ABUNDANCE_MAX_CAP, b.PATH_ABUNDANCE_ITERS, b.PATH_ABUNDANCE_MAX_ITERS,
            b.PATH_ABUNDANCE_TOL, b.PATH_ABUNDANCE_MAX_PATHS, b.PATH_ABUNDANCE_THETA_BITS, b.PATH_ABUNDANCE_RESP_BITS, b.PATH_ABUNDANCE_GROUP_ROWS,
            b.PATH_ABUNDANCE_MAX_GROUPS, b.PATH_ABUNDANCE_MAX_ROW_FACTOR, b.PATH_ABUNDANCE_BLOCK_ITERS) == (
        define("AB_LAMBDA_DEFAULT"), define("AB_LAMBDA_MAX"), define("AB_CAP_DEFAULT"), define("AB_CAP_MAX"), define("AB_ITERS_DEFAULT"), define("AB_ITERS_MAX"),
        define("AB_TOL_DEFAULT"), define("AB_MAX_PATHS"), define("AB_THETA_BITS"), define("AB_RESP_BITS"), define("AB_GROUP_ROWS"), define("AB_MAX_GROUPS"),
        define("AB_MAX_ROW_FACTOR"), define("AB_BLOCK_ITERS"))
    assert (b.PATH_ABUNDANCE_LAMBDA, b.PATH_ABUNDANCE_CAP, b.PATH_ABUNDANCE_ITERS, b.PATH_ABUNDANCE_TOL) == (512, 64, 1000, 16)
    assert b.PATH_ABUNDANCE_MAX_TOL == 1 << 24 and "#define AB_TOL_MAX (1u << 24)" in hpp
    assert b.PATH_ABUNDANCE_MAX_ROWS == 1 << 23 and "#define AB_MAX_ROWS (1ull << 23)" in hpp
    assert b.PATH_ABUNDANCE_CHUNK == 1024 and "#define AB_CHUNK_PATHS (64u * AB_LANE_PATHS)" in hpp and define("AB_LANE_PATHS") == 16
    assert b.PATH_ABUNDANCE_SOURCES == {"support": define("AB_FROM_SUPPORT"), "edit": define("AB_FROM_EDIT")} == {"support": 0, "edit": 1}
    # the flush bound of k_ab_estep's 32-bit partial sums: a responsibility is at most 2^16
    assert (1 << b.PATH_ABUNDANCE_RESP_BITS) * b.PATH_ABUNDANCE_GROUP_ROWS * b.PATH_ABUNDANCE_MAX_ROW_FACTOR < 1 << 32
    assert b.path_abundance_ppm(1 << 24) == 1000000 and b.path_abundance_ppm(0) == 0 and b.path_abundance_ppm((1 << 24) // 12) == 83333
    assert b.path_abundance_ppm(np.array([1 << 23, 16], dtype=np.uint32)).tolist() == [500000, 0] and ref.ppm(1 << 23) == 500000


# ---- 2. the table
@pytest.mark.parametrize("lam", [1, 128, 512, 4096])
def test_table_against_numpy(lam):
    b = binding()
    W = b.path_abundance_table(lam, 255)
    assert W.dtype == np.uint32 and W.shape == (256,)
    assert W[0] == 65536 and np.all(np.diff(W.astype(np.int64)) <= 0) and W.min() >= 1
    off = np.abs(W.astype(np.int64) - ref.table_float(lam, 255))
    print("lambda", lam, "W[1..4]", W[1:5].tolist(), "W[255]", int(W[255]), "largest |library - numpy|", int(off.max()))
    assert off.max() <= 1
    # a shorter table is the head of a longer one, and repeats its last entry
    for cap in (64, 1):
        S = b.path_abundance_table(lam, cap)
        assert np.array_equal(S[:cap + 1], W[:cap + 1]) and np.all(S[cap:] == W[cap])
    assert np.abs(b.path_abundance_table(lam, 64).astype(np.int64) - ref.table_float(lam, 64)).max() <= 1


def test_table_header_with_a_host_compiler(tmp_path):
    """csrc/vga_abundance.hpp is the one definition: compiled alone by a host compiler it prints the library's table"""
    src = tmp_path / "t.cpp"
    src.write_text('#include "vga_abundance.hpp"\n#include <cstdio>\nint main() { uint32_t t[256]; vga_ab_table(512, 64, t); '
                   'for (int x = 0; x < 256; x++) printf("%u\\n", t[x]); printf("%u %u %u\\n", vga_ab_ppm(1u << 24), vga_ab_ppm(8388608u), vga_ab_ppm(16u)); return 0; }\n')
    exe = str(tmp_path / "t")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(x) for x in out[:256]] == binding().path_abundance_table(512, 64).tolist()
    assert [int(x) for x in out[256:]] == [1000000, 500000, 0]


def test_table_refuses_bad_arguments():
    p = pkg()
    b = binding()
    L = b.load_library()
    buf = (ctypes.c_uint32 * 300)()
    for lam, cap in ((0, 64), (4097, 64), (512, 0), (512, 256), (1 << 31, 64)):
        assert L.vga_path_abundance_table(lam, cap, buf) == -1, (lam, cap)
        with pytest.raises(p.VgaError) as e:
            b.path_abundance_table(lam, cap)
        assert e.value.code == -1
    assert L.vga_path_abundance_table(512, 64, None) == -1
    assert L.vga_path_abundance_table(4096, 255, buf) == 0 and L.vga_path_abundance_table(1, 1, buf) == 0


# ---- 3. the reference on hand-made rows
def W_of(lam=LAM, cap=255):
    return binding().path_abundance_table(lam, cap)


def test_reference_one_path():
    res = ref.estimate([[0], [3], [0]], [1, 1, 0], W_of())
    assert res["theta"].tolist() == [1 << 24] and res["reads_q16"].tolist() == [2 << 16] and res["best"].tolist() == [1]
    assert (res["n_scored"], res["iterations"], res["converged"]) == (2, 1, True)


def test_reference_all_zero_matrix_is_uniform_at_once():
    trace = []
    res = ref.estimate(np.zeros((5, 3), dtype=np.uint8), [1] * 5, W_of(), trace=trace)
    assert res["theta"].tolist() == [(1 << 24) // 3] * 3 and res["iterations"] == 1 and res["converged"] and trace[0][2] == 0
    assert res["best"].tolist() == [5, 5, 5] and len(set(res["reads_q16"].tolist())) == 1
    # no row, or no scored row: no call
    for d, sc in ((np.zeros((0, 3), dtype=np.uint8), []), (np.zeros((2, 3), dtype=np.uint8), [0, 0])):
        none = ref.estimate(d, sc, W_of())
        assert not none["theta"].any() and not none["reads_q16"].any() and (none["n_scored"], none["iterations"], none["converged"]) == (0, 0, False)
        assert ref.tsv(none, ["a", "b", "c"]) == ref.HEADER + "\n" and ref.stderr_line(none, 2) == "path-abundance: no call"


def test_reference_identical_columns_stay_identical():
    rng = np.random.default_rng(3)
    d = rng.integers(0, 6, size=(40, 5)).astype(np.uint8)
    d[:, 3] = d[:, 1]
    trace = []
    ref.estimate(d, [1] * 40, W_of(128), iters=30, tol=0, trace=trace)
    assert len(trace) > 3 and all(t[0][1] == t[0][3] and t[1][1] == t[1][3] for t in trace)


def test_reference_unscored_row_changes_nothing():
    rng = np.random.default_rng(4)
    d = rng.integers(0, 4, size=(20, 4)).astype(np.uint8)
    base = ref.estimate(d, [1] * 20, W_of(), iters=50)
    more = ref.estimate(np.vstack([d[:7], [[9, 0, 0, 200]], d[7:]]), [1] * 7 + [0] + [1] * 13, W_of(), iters=50)
    ref.same(more, base)


def test_reference_iteration_limits():
    rng = np.random.default_rng(5)
    d = rng.integers(0, 4, size=(20, 4)).astype(np.uint8)
    one = ref.estimate(d, [1] * 20, W_of(), iters=1, tol=0)
    assert one["iterations"] == 1 and not one["converged"]
    loose = ref.estimate(d, [1] * 20, W_of(), iters=1000, tol=1 << 24)
    assert loose["iterations"] == 1 and loose["converged"]
    ref.same(dict(loose, converged=False), one)  # (the same single iteration)
    short = ref.estimate(d, [1] * 20, W_of(), iters=3, tol=0)
    assert short["iterations"] == 3 and not short["converged"]


def test_reference_a_row_with_one_zero_drives_the_others_down():
    # every row fits path 1 alone: its share rises and every other share falls, monotonically, to exactly 0
    d = np.full((6, 4), 2, dtype=np.uint8)
    d[:, 1] = 0
    trace = []
    res = ref.estimate(d, [1] * 6, W_of(), trace=trace)
    th = np.array([t[0] for t in trace], dtype=np.int64)
    assert np.all(np.diff(th[:, 1]) >= 0) and all(np.all(np.diff(th[:, p]) <= 0) for p in (0, 2, 3))
    assert res["converged"] and res["theta"][1] > (1 << 24) - 8 and res["theta"][[0, 2, 3]].tolist() == [0, 0, 0]
    assert res["best"].tolist() == [0, 6, 0, 0]


def test_reference_bounds_at_4096_paths():
    """the bounds of the definition (asserted inside the reference) with theta concentrated on one path: W[0] everywhere on it"""
    d = np.full((3, 4096), 255, dtype=np.uint8)
    d[:, 77] = 0
    trace = []
    res = ref.estimate(d, [1, 1, 1], W_of(1), iters=4, tol=0, trace=trace)
    assert res["iterations"] == 4
    d[:] = 0  # ... and spread evenly: every z is 4096 * 4096 * 65536 = 2^40
    even = ref.estimate(d, [1, 1, 1], W_of(1), iters=2, tol=0)
    assert even["theta"].tolist() == [4096] * 4096 and int(even["reads_q16"].sum()) == 3 << 16
    peak = ref.estimate(np.where(np.arange(4096)[None, :] == 5, 0, 255).astype(np.uint8).repeat(2, axis=0), [1, 1], W_of(4096), iters=50)
    assert peak["theta"][5] == 1 << 24 and peak["converged"] and int(peak["theta"].astype(np.int64).sum()) == 1 << 24


HARNESS = r"""
#include "vga_abundance.hpp"
#include <cstdio>
#include <vector>
static_assert(AB_MAX_PATHS == 4096u && AB_MAX_ROWS == (1ull << 23) && AB_THETA_BITS == 24u && AB_RESP_BITS == 16u, "the limits");
int main()
{
    unsigned long long n, np, lam, iters, tol;
    if (scanf("%llu %llu %llu %llu %llu", &n, &np, &lam, &iters, &tol) != 5) return 2;
    std::vector<uint8_t> d(n * np + 1), sc(n + 1);
    for (size_t i = 0; i < n; i++) { unsigned v; if (scanf("%u", &v) != 1) return 2; sc[i] = (uint8_t)v; }
    for (size_t i = 0; i < n * np; i++) { unsigned v; if (scanf("%u", &v) != 1) return 2; d[i] = (uint8_t)v; }
    uint32_t W[256];
    vga_ab_table((uint32_t)lam, 255, W);
    std::vector<uint32_t> theta(np, (1u << AB_THETA_BITS) / (uint32_t)np);
    std::vector<uint64_t> S(np);
    unsigned long long it = 0, conv = 0;
    while (it < iters) {
        const uint32_t diff = vga_ab_iterate_host(n, (uint32_t)np, d.data(), sc.data(), W, theta.data(), S.data());
        it++;
        if (diff <= tol) { conv = 1; break; }
    }
    printf("%llu %llu %u %u", it, conv, vga_ab_row_lanes((uint32_t)np), vga_ab_group_rows(n));
    for (size_t p = 0; p < np; p++) printf(" %u %llu", theta[p], (unsigned long long)S[p]);
    printf("\n");
    return 0;
}
"""


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "host sanitizers"])
def test_reference_equals_the_header_s_host_iteration(tmp_path, flags):
    """a stand-alone program with its own main: the header's iteration and nothing of the library"""
    src = tmp_path / "ab.cpp"
    src.write_text(HARNESS)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror"] + flags + ["-I", CSRC, str(src), "-o", str(tmp_path / "ab")])
    rng = np.random.default_rng(11)
    for n, npaths, lam, iters, tol in ((1, 1, 512, 5, 0), (9, 3, 512, 40, 16), (33, 17, 128, 25, 0), (5, 65, 4096, 10, 16), (70, 12, 1, 30, 4)):
        d = rng.integers(0, 7, size=(n, npaths)).astype(np.uint8)
        d[rng.integers(0, n), :] = 255
        sc = (rng.random(n) < 0.8).astype(np.uint8)
        sc[0] = 1
        text = "%d %d %d %d %d\n%s\n%s\n" % (n, npaths, lam, iters, tol, " ".join(map(str, sc.tolist())), " ".join(map(str, d.ravel().tolist())))
        pr = subprocess.run([str(tmp_path / "ab")], input=text, capture_output=True, text=True, timeout=120)
        assert pr.returncode == 0, pr.stderr
        f = [int(x) for x in pr.stdout.split()]
        want = ref.estimate(d, sc, W_of(lam), iters=iters, tol=tol)
        assert (f[0], bool(f[1])) == (want["iterations"], want["converged"]), (n, npaths)
        assert f[2] == min(64, 1 << (npaths - 1).bit_length()) and f[3] == 256
        assert f[4::2] == want["theta"].tolist() and f[5::2] == want["reads_q16"].tolist(), (n, npaths)


# ---- 4. the four DRB1 samples on the oracle's text
@pytest.fixture(scope="module")
def drb1_reads(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    _, paths = path_support_ref.parse_gfa(DRB1)
    names = [p[0] for p in paths]
    reads = pkg().readsim.simulate_reads(DRB1, 120, 3000, 0.03, 0.03, 0.04, seed=7)
    return ix, names, [(names.index(r.path), r) for r in reads]


def estimate_of(oracle, drb1_reads, keep, lam=LAM, iters=1000):
    ix, names, reads = drb1_reads
    sel = [r for p, r in reads if p in keep]
    _, ag, _ = oracle.map_reads(ix, [r.name for r in sel], [r.seq for r in sel])
    d, sc, _ = ref.gaf_rows(ag, DRB1, CAP)
    assert len(d) == len(sel)
    res = ref.estimate(d, sc, binding().path_abundance_table(lam, CAP), iters=iters)
    return res, {p: ref.ppm(res["theta"][p]) for p in range(12) if res["theta"][p]}


# what the committed reference gives: README.md quotes these.  They equal the figures of the prototype the feature was specified with.
@pytest.mark.parametrize("keep,n,iterations,ppm", [
    ({2, 5}, 26, 131, {2: 307686, 5: 692309, 9: 3}),
    ({4, 9}, 19, 34, {4: 505275, 9: 368417, 1: 63153, 7: 63153}),
    ({3}, 13, 143, {3: 1000000}),
], ids=["paths 2 and 5", "paths 4 and 9", "path 3"])
def test_drb1_sample(oracle, drb1_reads, keep, n, iterations, ppm):
    res, got = estimate_of(oracle, drb1_reads, keep)
    print(res["iterations"], got)
    assert (res["n_scored"], res["iterations"], res["converged"]) == (n, iterations, True)
    assert {p: v for p, v in got.items() if v} == ppm
    assert set(ref.order(res["theta"])[:len(keep)]) == keep
    if keep == {4, 9}:
        assert res["theta"][1] == res["theta"][7]  # (identical paths)


def test_drb1_identical_paths_share(oracle, drb1_reads):
    res, got = estimate_of(oracle, drb1_reads, {0, 1})
    print(res["iterations"], got)
    assert (res["n_scored"], res["iterations"], res["converged"]) == (20, 41, True)
    assert set(ref.order(res["theta"])[:4]) == {0, 8, 1, 7}
    assert res["theta"][0] == res["theta"][8] and res["theta"][1] == res["theta"][7] and res["theta"][0] > res["theta"][1]
    assert (got[0], got[8], got[1], got[7]) == (300004, 300004, 175002, 175002)


def test_drb1_small_lambda_does_not_converge_in_200_iterations(oracle, drb1_reads):
    res, _ = estimate_of(oracle, drb1_reads, {3}, lam=128, iters=200)
    assert res["iterations"] == 200 and not res["converged"] and ref.order(res["theta"])[0] == 3


def test_reference_text_by_hand():
    res = dict(theta=np.array([1 << 23, 0, 1 << 23, 100], dtype=np.uint32), reads_q16=np.array([7, 0, 7, 1], dtype=np.uint64),
               best=np.array([2, 0, 3, 0], dtype=np.uint64), n_scored=5, iterations=9, converged=True, n_paths=4)
    names = ["p0", "p1", "p2", "p3"]
    assert ref.tsv(res, names) == ref.HEADER + "\n1\tp0\t500000\t8388608\t7\t2\n2\tp2\t500000\t8388608\t7\t3\n"
    assert ref.tsv(res, names, 0).count("\n") == 5 and ref.tsv(res, names, 0).splitlines()[3:] == ["3\tp3\t5\t100\t1\t0", "4\tp1\t0\t0\t0\t0"]
    assert ref.stderr_line(res, 6) == "path-abundance: 5 reads scored of 6 kept, 9 iterations (converged), 2 paths at or above 10000 ppm: 500000 ppm, 500000 ppm"
    assert ref.stderr_line(dict(res, converged=False), 6, 600000) == "path-abundance: 5 reads scored of 6 kept, 9 iterations (not converged), 0 paths at or above 600000 ppm"


# ---- 5. the command line: the refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa", "-o", str(cwd / "o")] + args, cwd=str(cwd),
                          capture_output=True, text=True, timeout=300, env=env)


def test_cli_argument_errors(tmp_path):
    pkg()
    on = ["-D", "-G", DRB1, "--path-abundance"]
    off = ["-D", "-G", DRB1]
    cases = [(["--path-abundance"], ("--path-abundance", "--also-align"))]
    for flag, value in (("--abundance-lambda", "512"), ("--abundance-cap", "64"), ("--abundance-iters", "10"), ("--abundance-tol", "1"), ("--abundance-min", "0"),
                        ("--abundance-from", "edit")):
        cases.append((off + [flag, value], (flag, "without --path-abundance")))
        cases.append((off + ["--path-support", flag, value], (flag, "without --path-abundance")))
    for flag, value, words in (("--abundance-lambda", "0", "1 to 4096"), ("--abundance-lambda", "4097", "1 to 4096"), ("--abundance-lambda", "many", "1 to 4096"),
                               ("--abundance-cap", "0", "1 to 255"), ("--abundance-cap", "256", "1 to 255"), ("--abundance-cap", "6.5", "1 to 255"),
                               ("--abundance-iters", "0", "1 to 100000"), ("--abundance-iters", "100001", "1 to 100000"), ("--abundance-iters", "-1", "1 to 100000"),
                               ("--abundance-tol", "16777217", "0 to 16777216"), ("--abundance-tol", "", "0 to 16777216"), ("--abundance-min", "-1", "at least 0"),
                               ("--abundance-min", "1e4", "at least 0"), ("--abundance-from", "both", "edit or support"), ("--abundance-from", "Edit", "edit or support")):
        cases.append((on + [flag, value], (flag, words)))
    for args, words in cases:
        pr = run_cli(args, tmp_path)
        assert pr.returncode != 0 and all(w in pr.stderr for w in words), (args, pr.stderr)
        assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
        assert not os.listdir(str(tmp_path))
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--path-abundance [--abundance-lambda 512] [--abundance-cap 64] [--abundance-iters 1000] [--abundance-tol 16]" in usage.stderr, usage.stderr
    assert "[--abundance-min 10000] [--abundance-from support|edit]]" in usage.stderr


def test_cli_refuses_a_graph_without_paths_or_of_another_index(tmp_path):
    """the checks of --path-support: the switch reads the P lines of --graph, and holds the graph against the index, before any
    device is opened"""
    pkg()
    gfa = os.path.join(DATA, "test.gfa")
    pr = subprocess.run([EXE, "index", "-i", gfa, "-k", "11", "-o", str(tmp_path / "t")], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    (tmp_path / "r.fa").write_text(">r\nACGTACGTACGT\n")
    bare = tmp_path / "bare.gfa"
    bare.write_text("".join(ln for ln in open(gfa) if not ln.startswith("P")))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    common = [EXE, "map", "-i", str(tmp_path / "t"), "-f", str(tmp_path / "r.fa"), "-p", "abpoa", "--also-align", "--path-abundance"]
    pr = subprocess.run(common + ["-G", str(bare), "-o", str(tmp_path / "o1")], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode != 0 and "no P line" in pr.stderr and "--path-abundance" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr  # (refused before a context was asked for)
    pr = subprocess.run(common + ["-G", DRB1, "-o", str(tmp_path / "o2")], capture_output=True, text=True, timeout=300, env=env)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o1*")) and not glob.glob(str(tmp_path / "o2*"))


# ---- 6. the kernels from a cross-compile for gfx950: the resource fields
@pytest.fixture(scope="module")
def ab_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("abisa") / "ab.s")
    src = os.path.join(CSRC, "vga_abundance.hip")
    assert os.path.exists(src), "no csrc/vga_abundance.hip"
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only", "-I", CSRC, src, "-o", out],
                          stderr=subprocess.DEVNULL)
    return open(out).read()


def kernel_entry(isa, kernel):
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"E\w*)\n", isa):
        a = isa.rfind("\n  - ", 0, m.start())
        z = isa.find("\n  - ", m.end())
        entries.append(isa[a:z if z >= 0 else len(isa)])
    assert len(entries) == 1, kernel
    return lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))


@pytest.mark.parametrize("kernel", ["k_ab_keep", "k_ab_count", "k_ab_estep", "k_ab_mstep"])
def test_kernels_without_scratch_or_spills(ab_isa, kernel):
    field = kernel_entry(ab_isa, kernel)
    print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("wavefront_size") == 64
    assert field("max_flat_workgroup_size") == (64 if kernel == "k_ab_keep" else 256)
