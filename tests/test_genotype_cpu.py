"""Genotyping, the parts that need no GPU: the reference (tests/genotype_ref.py) on hand-made matrices and on the oracle's alignments
GAF, the pair index (Python and the header host and device share), the five vga_genotype_* calls in the ABI, the binding's methods and
constants, the command line's refusals, and the scratch budget of k_gt_pairs from a cross-compile for gfx950."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import genotype_ref
import path_support_ref
from helpers import DATA, ROOT, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_genotype_begin", "vga_genotype_read", "vga_genotype_reset", "vga_genotype_end", "vga_genotype_pairs"]


# ---- the ABI and the binding
def test_abi_lists_and_exports_the_five_calls():
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
    assert L.vga_genotype_begin(None) == -1 and L.vga_genotype_reset(None) == -1 and L.vga_genotype_end(None) == -1
    assert L.vga_genotype_read(None, 0, None, None, None, None) == -1
    assert L.vga_genotype_pairs(None, 0, 1, None, None, None, None, None, None) == -1


def test_binding_has_the_methods_and_the_kernel_s_constants():
    b = pkg().binding
    for name in ("genotype_begin", "genotype", "genotype_reset", "genotype_end", "genotype_pairs"):
        assert callable(getattr(b.Context, name)), name
    assert callable(b.pair_index) and callable(b.genotype_rank)
    hpp = open(os.path.join(CSRC, "vga_genotype.hpp")).read()
    define = lambda name: int(re.search(r"#define\s+" + name + r"\s+(\d+)u", hpp).group(1))
    assert (b.GENOTYPE_TILE, b.GENOTYPE_READS, b.GENOTYPE_MIN_CHUNKS, b.GENOTYPE_MAX_PATHS) == (
        define("GT_TILE"), define("GT_READS"), define("GT_MIN_CHUNKS"), define("GT_MAX_PATHS"))


# ---- the pair index
@pytest.mark.parametrize("n_paths", [1, 2, 3, 64, 65, 4096])
def test_pair_index_is_a_bijection(n_paths):
    b = pkg().binding
    p, q = np.triu_indices(n_paths)
    at = b.pair_index(n_paths, p, q)
    assert at.dtype == np.int64 and np.array_equal(at, np.arange(n_paths * (n_paths + 1) // 2))
    assert b.pair_count(n_paths) == len(at)
    assert np.array_equal(genotype_ref.pair_index(n_paths, p.astype(np.int64), q.astype(np.int64)), at)
    assert b.pair_index(n_paths, 0, 0) == 0 and b.pair_index(n_paths, n_paths - 1, n_paths - 1) == len(at) - 1


def test_pair_index_header_with_a_host_compiler(tmp_path):
    src = tmp_path / "pi.cpp"
    src.write_text('#include "vga_pair_index.hpp"\n#include <cstdio>\n#include <initializer_list>\nint main() { for (unsigned long long n : {1ull, 5ull, 65ull, 4096ull}) { '
                   'unsigned long long want = 0; for (unsigned long long p = 0; p < n; p++) for (unsigned long long q = p; q < n; q++, want++) '
                   'if (vga_pair_index(n, p, q) != want) { printf("bad %llu %llu %llu\\n", n, p, q); return 1; } '
                   'if (vga_pair_count(n) != want) return 2; } puts("ok"); return 0; }\n')
    exe = str(tmp_path / "pi")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", CSRC, str(src), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout == "ok\n"


# ---- the split of a call's reads over workgroups (vga_split_reads, shared by k_gt_pairs and k_gl_pairs)
SPLIT_MAIN = """#include "vga_pair_index.hpp"
#include <cstdio>
#include <cstdlib>
// argv: reads_per_chunk min_chunks max_group_reads, then n_reads n_tiles n_cu per case
int main(int argc, char **argv)
{
    const uint32_t chunk = (uint32_t)strtoul(argv[1], 0, 10), min_chunks = (uint32_t)strtoul(argv[2], 0, 10), limit = (uint32_t)strtoul(argv[3], 0, 10);
    for (int i = 4; i + 2 < argc; i += 3) {
        const vga_read_split s = vga_split_reads((uint32_t)strtoul(argv[i], 0, 10), (uint32_t)strtoul(argv[i + 1], 0, 10), atoi(argv[i + 2]), chunk, min_chunks, limit);
        printf("%u %u\\n", s.groups, s.reads_per_group);
    }
    return 0;
}
"""
SPLIT_READS = [1, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049, 65536]
SPLIT_NO_LIMIT = 0xFFFFFFFF


def gt_groups_of_the_parent(n_reads, n_tiles, n_cu):
    b = pkg().binding
    chunks = (n_reads + b.GENOTYPE_READS - 1) // b.GENOTYPE_READS
    want = (4 * max(n_cu, 1) + n_tiles - 1) // n_tiles
    most = max(1, chunks // b.GENOTYPE_MIN_CHUNKS)
    groups = max(1, min(want, most, 65535))
    per = (chunks + groups - 1) // groups
    return (chunks + per - 1) // per, per * b.GENOTYPE_READS


def gl_groups_of_the_parent(n_reads, n_tiles, n_cu):
    b = pkg().binding
    chunks = (n_reads + b.GENOTYPE_LIK_READS - 1) // b.GENOTYPE_LIK_READS
    want = (4 * max(n_cu, 1) + n_tiles - 1) // n_tiles
    most = max(1, chunks // b.GENOTYPE_LIK_MIN_CHUNKS)
    groups = max(1, min(want, most, 65535))
    per = min((chunks + groups - 1) // groups, b.GENOTYPE_LIK_MAX_GROUP_READS // b.GENOTYPE_LIK_READS)
    return (chunks + per - 1) // per, per * b.GENOTYPE_LIK_READS


def split_cases():
    b = pkg().binding
    shape = [(t, cu) for t in (1, 2, 3, 528, 2080) for cu in (0, 1, 256)]
    gt = (b.GENOTYPE_READS, b.GENOTYPE_MIN_CHUNKS, SPLIT_NO_LIMIT, gt_groups_of_the_parent,
          [(n, t, cu) for n in SPLIT_READS + [(1 << 31) - 1] for t, cu in shape])
    gl = (b.GENOTYPE_LIK_READS, b.GENOTYPE_LIK_MIN_CHUNKS, b.GENOTYPE_LIK_MAX_GROUP_READS, gl_groups_of_the_parent,
          [(n, t, cu) for n in SPLIT_READS + [65535 * b.GENOTYPE_LIK_MAX_GROUP_READS] for t, cu in shape])
    return {"genotype": gt, "likelihood": gl}


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]],
                         ids=["plain", "sanitized"])
def test_split_rule_is_the_parent_s_two_rules(tmp_path, flags):
    src = tmp_path / "split.cpp"
    src.write_text(SPLIT_MAIN)
    exe = str(tmp_path / "split")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", CSRC, str(src), "-o", exe])
    for stage, (chunk, min_chunks, limit, parent, cases) in split_cases().items():
        assert len(cases) == 12 * 5 * 3
        pr = subprocess.run([exe, str(chunk), str(min_chunks), str(limit)] + [str(x) for c in cases for x in c], capture_output=True, text=True, timeout=60)
        assert pr.returncode == 0 and not pr.stderr, pr.stderr
        got = [tuple(int(x) for x in ln.split()) for ln in pr.stdout.splitlines()]
        assert len(got) == len(cases)
        for (n_reads, n_tiles, n_cu), (groups, per_group) in zip(cases, got):
            what = (stage, n_reads, n_tiles, n_cu, groups, per_group)
            assert (groups, per_group) == parent(n_reads, n_tiles, n_cu), what
            assert 1 <= groups <= 65535, what
            assert per_group % chunk == 0 and per_group > 0, what
            assert limit == SPLIT_NO_LIMIT or per_group <= limit, what
            assert groups * per_group >= n_reads, what
            assert (groups - 1) * per_group < n_reads, what  # (no workgroup without a read)


# ---- the owner of the states and workspaces (vga_owned, vga_common.hpp)
OWNER_MAIN = """#include "vga_common.hpp"
#include <type_traits>
struct payload {
    static int live, made;
    int *p;
    payload() : p(new int(7)) { live++; made++; }
    ~payload() { delete p; live--; }
};
int payload::live = 0, payload::made = 0;
int main()
{
    static_assert(!std::is_copy_constructible<vga_owned<payload>>::value && !std::is_copy_assignable<vga_owned<payload>>::value, "one owner");
    {
        vga_owned<payload> a{nullptr, nullptr};
        if (a || a.get()) return 1;
        a.reset();  // (empty: harmless)
        a = vga_make_owned<payload>();
        if (!a || *a->p != 7 || payload::live != 1) return 2;
        a.reset();
        if (a || payload::live != 0) return 3;
        a.reset();  // (again)
        a = vga_make_owned<payload>();
        a = vga_make_owned<payload>();  // (reassignment releases the first)
        if (payload::live != 1 || payload::made != 3) return 4;
        vga_owned<void> v = vga_make_owned<void, payload>();  // (held without its type: the deleter knows it)
        if (!v || payload::live != 2) return 5;
        vga_owned<payload> b = std::move(a);
        if (a || !b || payload::live != 2) return 6;
    }  // (b and v are destroyed holding their payloads)
    if (payload::live != 0 || payload::made != 4) return 7;
    puts("ok");
    return 0;
}
"""


def test_owner_type_under_the_host_sanitizers(tmp_path):
    """a stand-alone host program: no HIP call, no device code"""
    src = tmp_path / "owner.hip"
    src.write_text(OWNER_MAIN)
    exe = str(tmp_path / "owner")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                           "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", exe], stderr=subprocess.DEVNULL)
    assert b"__asan_init" in open(exe, "rb").read()
    pr = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert (pr.returncode, pr.stdout, pr.stderr) == (0, "ok\n", ""), (pr.returncode, pr.stderr)


# ---- the reference on hand-made matrices
def test_reference_on_hand_made_matrices():
    #         path 0  1  2
    bases = [[10, 10, 9],    # r0: 0 and 1 tie in bases, edges decide for 1
             [5, 4, 5],      # r1: 1 has fewer bases and more edges: lexicographic, not the sum -- 0 and 2 win over it
             [7, 7, 7],      # r2: a full tie everywhere
             [0, 0, 0]]      # r3: an unplaced row
    edges = [[1, 2, 9],
             [1, 9, 1],
             [3, 3, 3],
             [0, 0, 0]]
    t = genotype_ref.pairs(bases, edges)
    at = lambda p, q: genotype_ref.pair_index(3, p, q)
    row = lambda p, q: tuple(int(t[k][at(p, q)]) for k in genotype_ref.FIELDS)
    assert [at(0, 0), at(0, 1), at(0, 2), at(1, 1), at(1, 2), at(2, 2)] == list(range(6))
    assert row(0, 0) == (22, 5, 0, 0) and row(1, 1) == (21, 14, 0, 0) and row(2, 2) == (21, 13, 0, 0)
    # (0, 1): r0 takes 1 on the edges (10, 2), r1 takes 0 (5, 1) though 4 + 9 > 5 + 1, r2 and r3 tie and take 0
    assert row(0, 1) == (10 + 5 + 7, 2 + 1 + 3, 1, 1)
    # (0, 2): r0 takes 0 (10 > 9 whatever the edges), r1 is a full tie (5, 1) = (5, 1): neither prefers
    assert row(0, 2) == (10 + 5 + 7, 1 + 1 + 3, 1, 0)
    # (1, 2): r0 takes 1, r1 takes 2
    assert row(1, 2) == (10 + 5 + 7, 2 + 1 + 3, 1, 1)
    # ranking: 22 bases everywhere but the diagonal of 1 and 2; then edges; then the homozygous pair first; then p, q
    assert genotype_ref.rank(t) == [(0, 1), (1, 2), (0, 0), (0, 2), (1, 1), (2, 2)]
    assert genotype_ref.rank(t, 2) == [(0, 1), (1, 2)]
    assert pkg().binding.genotype_rank(t) == genotype_ref.rank(t) and pkg().binding.genotype_rank(t, 3) == genotype_ref.rank(t, 3)
    # the homozygous pair goes first on a tie, and pairs with sums (0, 0) are not ranked
    t = genotype_ref.pairs([[4, 0, 0]], [[1, 0, 0]])
    assert genotype_ref.rank(t) == [(0, 0), (0, 1), (0, 2)] == pkg().binding.genotype_rank(t)
    t = genotype_ref.pairs(np.zeros((3, 4)), np.zeros((3, 4)))
    assert genotype_ref.rank(t) == [] == pkg().binding.genotype_rank(t)
    t = genotype_ref.pairs(np.zeros((0, 2)), np.zeros((0, 2)))
    assert t["sum_bases"].tolist() == [0, 0, 0]


def test_rank_keeps_64_bits():
    big = 1 << 63
    t = {"n_paths": 2, "sum_bases": np.array([big, big + 1, 5], dtype=np.uint64), "sum_edges": np.array([0, 0, big], dtype=np.uint64)}
    assert genotype_ref.rank(t) == [(0, 1), (0, 0), (1, 1)] == pkg().binding.genotype_rank(t)


# ---- the measure on the oracle's text
@pytest.fixture(scope="module")
def drb1_reads(oracle):
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    reads = pkg().readsim.simulate_reads(DRB1, 120, 3000, 0.03, 0.03, 0.04, seed=7)
    names = [p[0] for p in paths]
    return ix, node_len, paths, [(names.index(r.path), r) for r in reads]


def table_of(oracle, drb1_reads, keep):
    ix, node_len, paths, reads = drb1_reads
    sel = [r for p, r in reads if p in keep]
    _, ag, _ = oracle.map_reads(ix, [r.name for r in sel], [r.seq for r in sel])
    w = path_support_ref.walk(ag, node_len, paths)
    return len(sel), genotype_ref.pairs(w["bases"], w["edges"])


@pytest.mark.parametrize("pair,n_reads,best,second", [((2, 5), 26, (73566, 13638), (73563, 13634)), ((4, 9), 19, (53816, 11826), (53801, 11795))],
                         ids=["paths 2 and 5", "paths 4 and 9"])
def test_heterozygous_sample_is_called(oracle, drb1_reads, pair, n_reads, best, second):
    n, t = table_of(oracle, drb1_reads, set(pair))
    ranked = genotype_ref.rank(t)
    sums = lambda pq: (int(t["sum_bases"][genotype_ref.pair_index(12, *pq)]), int(t["sum_edges"][genotype_ref.pair_index(12, *pq)]))
    print(n, "reads; best", ranked[0], sums(ranked[0]), "then", ranked[1], sums(ranked[1]))
    assert n == n_reads
    assert ranked[0] == pair and sums(ranked[0]) == best and sums(ranked[1]) == second
    assert pkg().binding.genotype_rank(t, 5) == ranked[:5]


def test_homozygous_sample_is_called_through_the_homozygous_first_rule(oracle, drb1_reads):
    n, t = table_of(oracle, drb1_reads, {3})
    ranked = genotype_ref.rank(t)
    at = lambda pq: genotype_ref.pair_index(12, *pq)
    assert n > 0 and ranked[0] == (3, 3)
    assert (int(t["sum_bases"][at((3, 3))]), int(t["sum_edges"][at((3, 3))])) == (36409, 5981)
    # it ties with the heterozygous pairs that hold 3: sum[p, q] >= sum[p, p] always
    assert (t["sum_bases"][at(ranked[1])], t["sum_edges"][at(ranked[1])]) == (t["sum_bases"][at((3, 3))], t["sum_edges"][at((3, 3))])
    assert 3 in ranked[1] and ranked[1][0] != ranked[1][1]


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE] + args, cwd=str(cwd), capture_output=True, text=True, timeout=300, env=env)


def test_cli_genotype_needs_also_align(tmp_path):
    pkg()
    pr = run_cli(["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--genotype", "-o", str(tmp_path / "o")], tmp_path)
    assert pr.returncode != 0
    assert "--also-align" in pr.stderr and "--genotype" in pr.stderr, pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


@pytest.mark.parametrize("top", ["-1", "many", "3.5", ""])
def test_cli_refuses_a_genotype_top_that_is_no_count(tmp_path, top):
    pkg()
    pr = run_cli(["map", "-i", str(tmp_path / "none"), "-f", str(tmp_path / "none.fa"), "-p", "abpoa", "--also-align", "-G", DRB1, "--genotype",
                  "--genotype-top", top, "-o", str(tmp_path / "o")], tmp_path)
    assert pr.returncode != 0 and "--genotype-top" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o*"))


def test_cli_refuses_a_graph_without_paths(tmp_path):
    pkg()
    gfa = os.path.join(DATA, "test.gfa")
    pr = subprocess.run([EXE, "index", "-i", gfa, "-k", "11", "-o", str(tmp_path / "t")], capture_output=True, text=True, timeout=300)
    assert pr.returncode == 0, pr.stderr
    (tmp_path / "r.fa").write_text(">r\nACGTACGTACGT\n")
    bare = tmp_path / "bare.gfa"
    bare.write_text("".join(ln for ln in open(gfa) if not ln.startswith("P")))
    common = ["map", "-i", str(tmp_path / "t"), "-f", str(tmp_path / "r.fa"), "-p", "abpoa", "--also-align", "--genotype"]
    pr = run_cli(common + ["-G", str(bare), "-o", str(tmp_path / "o1")], tmp_path)
    assert pr.returncode != 0 and "no P line" in pr.stderr and "--genotype" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr  # (refused before a context was asked for)
    pr = run_cli(common + ["-G", DRB1, "-o", str(tmp_path / "o2")], tmp_path)
    assert pr.returncode != 0 and "not the graph the index was built from" in pr.stderr, pr.stderr
    assert "device" not in pr.stderr.lower(), pr.stderr
    assert not glob.glob(str(tmp_path / "o1*")) and not glob.glob(str(tmp_path / "o2*"))


def test_usage_names_the_switch():
    pkg()
    pr = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert "--genotype" in pr.stderr and "--genotype-top" in pr.stderr


# ---- the kernel, cross-compiled
@pytest.fixture(scope="module")
def gt_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gtisa") / "gt.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_genotype.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


def test_pair_kernel_without_scratch(gt_isa):
    b = pkg().binding
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+k_gt_pairsE\w*)\n", gt_isa):
        a = gt_isa.rfind("\n  - ", 0, m.start())
        z = gt_isa.find("\n  - ", m.end())
        entries.append(gt_isa[a:z if z >= 0 else len(gt_isa)])
    assert len(entries) == 1
    field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", entries[0]).group(1))
    print("k_gt_pairs vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("wavefront_size") == 64 and field("max_flat_workgroup_size") == 256
    # two staged key arrays, one 64-bit key per read and path
    assert field("group_segment_fixed_size") == 2 * b.GENOTYPE_READS * b.GENOTYPE_TILE * 8
    # the sums are combined with 64-bit vector atomics
    assert "global_atomic_add_x2" in gt_isa
