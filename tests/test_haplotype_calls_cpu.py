"""The haplotype counts and calls, the parts that need no GPU: the reference (tests/haplotype_calls_ref.py) against jobs, rows and
calls computed by hand, vga_haplotype_jobs and vga_haplotype_call of the built library against the reference, the calls in the ABI,
the command line's refusal, the scratch budget of the three kernels from a cross-compile for gfx950, and the planted sample with a
homozygous substitution and a heterozygous insertion added, on the oracle's alignments GAF.  Without the feature every test here
stops at the missing binding call (haplotype_jobs, haplotype_call: asked for first, also by the tests of the reference alone), the
missing symbols or kernels, or the unknown switch; checked once against the parent commit, where all eleven fail."""
import os
import re
import subprocess

import numpy as np
import pytest

import hapcall_cases as H
import haplotype_calls_ref as ref
import phase_cases as P
import phase_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_haplotype_counts", "vga_haplotype_counts_lists", "vga_haplotype_jobs", "vga_haplotype_call"]


def binding():
    b = pkg().binding
    assert hasattr(b, "haplotype_jobs") and hasattr(b, "haplotype_call"), "the binding has no haplotype calls"
    return b


def reference_rows(case):
    recs, words = P.pack(case.reads)
    obs = phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)
    shows = ref.shows_lists(recs, words, case.cpos, case.cref)
    return ref.counts(shows, ref.tags(obs, case.ps, case.flip), ref.jobs(case.cpos, case.pos, case.ps))


# ---- the reference on cases written out by hand
def test_jobs_by_hand():
    binding()
    h = H.HAND
    assert ref.jobs(h.cpos, h.pos, h.ps) == H.HAND_JOBS and len(H.HAND_JOBS) == 10
    # every site its own set: a job where the site's own base is a call, and nowhere else
    assert ref.jobs(h.cpos, h.pos, [1, 2, 3, 4]) == [(1, 1), (3, 2), (5, 3), (7, 4)]
    assert ref.jobs([6, 11], h.pos, [1, 2, 3, 4]) == []
    # nested: set 1 = sites 0 and 3 (bases 5 .. 30), set 2 = sites 1 and 2 (bases 10 .. 20)
    assert ref.jobs(h.cpos, h.pos, [1, 2, 2, 1]) == [(1, 1), (2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (5, 1), (5, 2), (6, 1), (7, 1)]
    # two sets behind each other: base 15 lies strictly between their spans
    assert ref.jobs(h.cpos, h.pos, [1, 1, 3, 3]) == [(1, 1), (2, 1), (3, 1), (5, 3), (6, 3), (7, 3)]
    assert ref.jobs([], h.pos, h.ps) == [] and ref.jobs(h.cpos, [], []) == []


def test_counts_by_hand():
    binding()
    assert reference_rows(H.HAND) == H.HAND_ROWS
    case, rows = H.columns_case()
    assert reference_rows(case) == rows
    case, rows = H.columns_case(copies=3)
    assert reference_rows(case) == rows and rows[0][2:9] == [6, 0, 0, 3, 0, 0, 0]
    text, n_jobs, n_lines, differ = ref.tsv(H.HAND_ROWS, H.HAND.cpos, [0, 10, 40], "ACGTACGTAC" * 4)
    assert (n_jobs, n_lines) == (10, 10) and text.splitlines()[0] == ref.HEADER
    # base 5 is offset 5 of node 1; base 15 offset 5 of node 2: "other" decides nothing, a carries an insertion in half of its reads
    assert text.splitlines()[1] == "1\t5\tC\t1\tA\tC\t2\t1\t2\t0\t0\t0\t0\t0\t0\t0\t1\t0\t0\t0\t0\t0"
    assert text.splitlines()[5] == "2\t5\tC\t1\t?\t.\t2\t0\t0\t0\t0\t0\t2\t0\t1\t0\t0\t0\t0\t0\t0\t1"
    assert differ == 4   # base 5, base 10 in set 1 and in set 2: A against C; base 20 in set 1: C against A (in set 2 a is undecided)


def test_call_rule_by_hand():
    b = binding()
    cases = {(3, 0, 0, 0, 0, 0, 0): "A", (0, 0, 0, 0, 0, 4, 0): "-", (0, 0, 0, 0, 0, 0, 0): ".", (0, 0, 0, 0, 0, 0, 5): ".",   # obs = 0 with insertions
             (2, 2, 0, 0, 0, 0, 0): "?", (2, 0, 0, 0, 1, 1, 0): "?",      # a tie between A and C; exactly half
             (3, 0, 0, 0, 1, 1, 0): "A", (0, 0, 0, 5, 0, 0, 3): "T+", (0, 0, 0, 5, 0, 0, 2): "T", (1, 1, 0, 0, 0, 0, 2): "?+",
             (0, 0, 0, 0, 3, 0, 0): "?", (0, 1, 0, 0, 3, 0, 0): "?", (0, 0, 1, 0, 0, 0, 0): "G", (0, 2, 0, 0, 0, 1, 0): "C",
             (0, 0, 0, 0xFFFFFFFF, 0, 0xFFFFFFFF, 0): "?", (0xFFFFFFFF, 0xFFFFFFFE, 0, 0, 0, 0, 0xFFFFFFFF): "A+"}
    for n, want in cases.items():
        assert ref.call(n) == want, n
        assert b.haplotype_call(n) == want, n
    rng = np.random.default_rng(5)
    for _ in range(2000):
        n = [int(v) for v in rng.integers(0, 4, size=7) * rng.integers(0, 3, size=7)]
        assert b.haplotype_call(n) == ref.call(n), n


def test_library_jobs_equal_the_reference():
    b = binding()
    h = H.HAND
    assert b.haplotype_jobs(h.cpos, h.pos, h.ps).tolist() == [list(j) for j in H.HAND_JOBS]
    assert b.haplotype_jobs([], h.pos, h.ps).shape == (0, 2) and b.haplotype_jobs(h.cpos, [], []).shape == (0, 2)
    rng = np.random.default_rng(9)
    for n_sites, n_calls in ((1, 1), (8, 5), (9, 30), (65, 65), (300, 200)):
        n_bases = 4 * n_sites + n_calls + 8
        pos = np.sort(rng.choice(n_bases, size=n_sites, replace=False))
        cpos = np.sort(rng.choice(n_bases, size=n_calls, replace=False))
        for k in range(4):
            ps = []
            for s in range(n_sites):   # a site opens a set or joins the set of an earlier one
                ps.append(s + 1 if s == 0 or rng.integers(0, 3) == 0 else ps[int(rng.integers(0, s))])
            got = b.haplotype_jobs(cpos, pos, ps)
            assert got.dtype == np.uint32 and got.tolist() == [list(j) for j in ref.jobs(cpos, pos, ps)], (n_sites, n_calls, k)
    for bad in (dict(cpos=[5, 5]), dict(cpos=[7, 5]), dict(pos=[5, 5, 20, 30]), dict(ps=[0, 2, 1, 2]), dict(ps=[1, 3, 3, 2]), dict(ps=[1, 2, 1, 5])):
        with pytest.raises(pkg().VgaError):
            b.haplotype_jobs(bad.get("cpos", h.cpos), bad.get("pos", h.pos), bad.get("ps", h.ps))


# ---- the ABI
def test_abi_lists_and_exports_the_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(L, name) is not None and getattr(L, name).argtypes is not None
    src = tmp_path / "hc.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*c)(vga_ctx *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *,\n"
                   "         uint64_t, uint32_t *, uint64_t *, uint64_t *) = vga_haplotype_counts;\n"
                   "int (*l)(vga_ctx *, uint64_t, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint8_t *, uint64_t,\n"
                   "         const uint32_t *, const uint8_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *, uint64_t, uint32_t *,\n"
                   "         uint64_t *) = vga_haplotype_counts_lists;\n"
                   "int (*j)(uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint32_t *, uint64_t, uint32_t *, uint64_t *) = vga_haplotype_jobs;\n"
                   "int (*k)(const uint32_t *, char *) = vga_haplotype_call;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "hc.o")])
    hpp = open(os.path.join(CSRC, "vga_hapcall.hpp")).read()
    assert p.binding.HAPLOTYPE_ROW == 16 == int(re.search(r"#define HC_ROW (\d+)u", hpp).group(1))
    assert p.binding.HAPLOTYPE_MAX_JOBS == 1 << 24 and "#define HC_MAX_JOBS (1ull << 24)" in hpp and "#define HC_MAX_CALLS (1ull << 24)" in hpp
    for name in ("haplotype_counts", "haplotype_counts_lists"):
        assert hasattr(p.binding.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    assert L.vga_haplotype_counts(None, 0, None, 0, None, None, None, None, None, 0, None, None, None) == -1
    assert L.vga_haplotype_counts_lists(None, 0, 0, None, 0, None, 0, None, None, 0, None, None, None, None, None, None, 0, None, None) == -1
    assert L.vga_haplotype_jobs(0, None, 0, None, None, 0, None, None) == -1
    assert L.vga_haplotype_call(None, None) == -1


# ---- the command line: the refusal before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa"] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300, env=env)


def test_cli_haplotype_calls_needs_haplotag(tmp_path):
    pkg()
    for args in (["--call-variants", "--phase", "--haplotype-calls"], ["--call-variants", "--haplotype-calls"], ["--haplotype-calls"]):
        pr = run_cli(["-D", "-G", "none.gfa"] + args, tmp_path)
        assert pr.returncode != 0 and "--haplotype-calls" in pr.stderr and "--haplotag" in pr.stderr, pr.stderr
        assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
        assert not os.listdir(str(tmp_path))
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--haplotype-calls]" in usage.stderr, usage.stderr


# ---- the planted sample on the oracle's text
def test_planted_haplotypes_are_called(oracle):
    """The planted sample of test_phase_cpu.py (haplotype A carries substitutions at s1 and s3, B at s2; 12 reads of 1000 bases each)
    extended in the same node, between the planted sites: a substitution on both haplotypes at five eighths of the node and three
    inserted letters behind the base at three eighths of it on haplotype A alone.  In the rows of the planted set the three heterozygous bases carry the planted
    letters as the phase chain arranges them, the homozygous base has a = b = the planted letter, and exactly one of the two calls
    has "+" at the insertion base."""
    binding()
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    idx = [int(v) for v in a["node_seq_idx"]]
    base_reads, at, new, old = P.planted_sample(rs, DRB1, a["node_seq_idx"], n_reads=1)   # (only for the sites and the letters)
    # the same construction with the two additions: rebuild the haplotypes as planted_sample does
    segs, paths = rs.parse_gfa_paths(DRB1)
    _, steps = paths[3]
    off = 0
    for nid, _ in steps:
        if off >= 2000 and len(segs[nid]) >= 50:
            break
        off += len(segs[nid])
    ln = len(segs[nid])
    assert [idx[nid - 1] + o for o in (ln // 4, ln // 2, 3 * ln // 4)] == at
    seq = rs.path_sequence(segs, steps)
    hom_o, ins_o = 5 * ln // 8, 3 * ln // 8
    hom_at, ins_at = idx[nid - 1] + hom_o, idx[nid - 1] + ins_o
    hom_new = "ACGT"[("ACGT".index(seq[off + hom_o].upper()) + 1) % 4]
    # three letters that cannot be placed one base to the left or right: none equals the base before or the base behind
    free = [c for c in "ACGT" if c not in (seq[off + ins_o].upper(), seq[off + ins_o + 1].upper())]
    ins_letters = free[0] + free[1] + free[0]
    hap_a, hap_b = list(seq), list(seq)
    hap_a[off + ln // 4], hap_a[off + 3 * ln // 4], hap_b[off + ln // 2] = new[0], new[2], new[1]
    hap_a[off + hom_o] = hap_b[off + hom_o] = hom_new
    hap_a[off + ins_o] = seq[off + ins_o] + ins_letters
    rng = np.random.Generator(np.random.PCG64(11))
    reads, length, n_reads = [], 1000, 12
    first, last = off + ln // 4, off + 3 * ln // 4
    for name, hap, shift in (("a", "".join(hap_a), 3), ("b", "".join(hap_b), 0)):
        for r in range(n_reads):
            o = last - length + 1 + (r + 1) * (length - (last - first) - 1 - 3) // (n_reads + 1)
            assert o <= first and o + length > last + shift
            tpl = np.frombuffer(hap[o:o + length].encode(), dtype=np.uint8)
            reads.append(("%s%d" % (name, r), rs._mutate(tpl, rng, 0.01, 0.01, 0.01).decode()))
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    g = ref.gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    text, n_jobs, n_lines, differ = ref.tsv(g["rows"], g["cpos"], a["node_seq_idx"], a["seq_fwd"])
    print(text, n_jobs, n_lines, differ)
    assert len(g["shows"]) == 24
    h = [g["pos"].index(p) for p in at]
    planted = g["ps"][h[0]]
    assert g["ps"][h[1]] == planted and g["ps"][h[2]] == planted
    mine = {g["cpos"][row[0]]: (ref.call(row[2:9]), ref.call(row[9:16]), row) for row in g["rows"] if row[1] == planted}
    assert set(at) | {hom_at, ins_at} <= set(mine), (sorted(mine), at, hom_at, ins_at)
    # the heterozygous bases: the letters as <out>-phase.tsv arranges them (haplotype a carries flip ? y : x)
    for k in range(3):
        i = h[k]
        want = ("ACGT-"[g["y"][i] if g["flip"][i] else g["x"][i]], "ACGT-"[g["x"][i] if g["flip"][i] else g["y"][i]])
        assert sorted(want) == sorted((old[k], new[k])), k
        assert tuple(c.rstrip("+") for c in mine[at[k]][:2]) == want, (k, mine[at[k]])
    assert mine[hom_at][0] == mine[hom_at][1] == hom_new, mine[hom_at]
    assert sorted(c.endswith("+") for c in mine[ins_at][:2]) == [False, True], mine[ins_at]
    # the haplotype with the insertion is the one that carries the planted letters of s1 and s3
    assert mine[ins_at][0].endswith("+") == (mine[at[0]][0] == new[0]), (mine[ins_at], mine[at[0]])
    assert text == ref.tsv_gaf(ag, a["node_seq_idx"], a["seq_fwd"])[0] and n_lines <= n_jobs == len(g["rows"])


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def hc_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hcisa") / "ph.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_phase.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel,lds", [("k_hc_tags", 0), ("k_hc_cols", 0), ("k_hc_count", 4 * 14 * 4)])
def test_kernels_without_scratch(hc_isa, kernel, lds):
    """no scratch, no spill, and no LDS beyond the four waves' fourteen counters.  The fields of the code-object metadata only."""
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"\w*)\n", hc_isa):
        a = hc_isa.rfind("\n  - ", 0, m.start())
        b = hc_isa.find("\n  - ", m.end())
        entries.append(hc_isa[a:b if b >= 0 else len(hc_isa)])
    assert len(entries) == 1, (kernel, len(entries))
    for e in entries:
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("wavefront_size") == 64 and field("group_segment_fixed_size") == lds
