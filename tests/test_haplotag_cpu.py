"""The haplotype tags, the parts that need no GPU: the reference (tests/haplotag_ref.py) against rows computed by hand, the
vga_phase_tags* calls in the ABI, the command line's refusal, the scratch budget of k_ph_tag and k_ph_tag_scan from a cross-compile
for gfx950, and the two planted haplotypes told apart on the oracle's alignments GAF.  Without the feature every test here stops
at the missing reference, symbols, switch or kernels."""
import os
import re
import subprocess

import numpy as np
import pytest

import haplotag_ref
import phase_cases as P
import phase_ref
import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_phase_tags", "vga_phase_tags_lists"]


# ---- the reference on observations written out by hand (phase_cases.TINY_OBS, EDGE_OBS)
def test_rows_by_hand_one_set_with_a_flipped_site():
    """site 1 flipped: its y is haplotype a.  Reads 1 and 2 tie 1 : 1, read 3 votes at site 1 alone (site 0 shows a deletion that
    is no allele), reads 4 and 5 consume no site and have no row"""
    rows = haplotag_ref.rows(P.TINY_OBS, [1, 1], [0, 1])
    assert rows == [(0, 1, 2, 0), (1, 1, 1, 1), (2, 1, 1, 1), (3, 1, 1, 0)]
    text, n, a, b, tied = haplotag_ref.tsv(rows)
    assert text == haplotag_ref.HEADER + "\n0\t1\ta\t2\t0\n1\t1\t.\t1\t1\n2\t1\t.\t1\t1\n3\t1\ta\t1\t0\n" and (n, a, b, tied) == (4, 2, 0, 2)
    assert haplotag_ref.HEADER == "read\tps\thap\tvotes_a\tvotes_b"
    # the input file's numbers: records 0 .. 3 are reads 7, 2, 9, 4 -- the text comes in read order
    text = haplotag_ref.tsv(rows, [7, 2, 9, 4, 5, 6])[0]
    assert text == haplotag_ref.HEADER + "\n2\t1\t.\t1\t1\n4\t1\ta\t1\t0\n7\t1\ta\t2\t0\n9\t1\t.\t1\t1\n"


def test_rows_by_hand_every_site_its_own_set():
    rows = haplotag_ref.rows(P.TINY_OBS, [1, 2], [0, 0])
    assert rows == [(0, 1, 1, 0), (0, 2, 0, 1), (1, 1, 0, 1), (1, 2, 0, 1), (2, 1, 1, 0), (2, 2, 1, 0), (3, 2, 0, 1)]
    assert haplotag_ref.table(P.TINY_OBS, [1, 2], [0, 0]).shape == (7, 4)


def test_rows_by_hand_interleaved_sets():
    """sites 0, 2, 4 in set 1 (flips 0, 1, 1) and sites 1, 3 in set 2 (flips 1, 0): ps is not monotone in h.  Read 3 has two votes
    for b in set 2, read 4 no row, read 5 rows in both sets though it skips sites 1 and 2"""
    rows = haplotag_ref.rows(P.EDGE_OBS, [1, 2, 1, 2, 1], [0, 1, 1, 0, 1])
    assert rows == [(0, 1, 2, 0), (0, 2, 0, 1), (1, 1, 1, 0), (1, 2, 1, 0), (2, 1, 0, 1), (2, 2, 0, 1), (3, 1, 1, 0), (3, 2, 0, 2), (5, 1, 2, 0), (5, 2, 1, 0)]
    text, n, a, b, tied = haplotag_ref.tsv(rows)
    assert (n, a, b, tied) == (10, 6, 4, 0) and text.splitlines()[8] == "3\t2\tb\t0\t2"
    assert haplotag_ref.rows([], [1], [0]) == [] and haplotag_ref.rows([[3, 2]], [1, 1], [0, 1]) == []
    assert haplotag_ref.tsv([]) == (haplotag_ref.HEADER + "\n", 0, 0, 0, 0)
    assert haplotag_ref.table([], [], []).shape == (0, 4)


def test_rows_from_the_lists_of_the_cases():
    """the observations of the stored lists give the same rows as the ones written out by hand"""
    for case, obs in ((P.TINY, P.TINY_OBS), (P.EDGE, P.EDGE_OBS)):
        recs, words = P.pack(case.reads)
        got = phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref)
        ps, flip = [1] * len(case.pos), [h & 1 for h in range(len(case.pos))]
        assert haplotag_ref.rows(got, ps, flip) == haplotag_ref.rows(obs, ps, flip), case.name


# ---- the ABI
def test_abi_lists_and_exports_the_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(L, name) is not None and getattr(L, name).argtypes is not None
    src = tmp_path / "tag.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*t)(vga_ctx *, uint64_t, const uint32_t *, const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *, uint64_t, uint32_t *,\n"
                   "         uint64_t *, uint64_t *) = vga_phase_tags;\n"
                   "int (*s)(vga_ctx *, uint64_t, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint8_t *,\n"
                   "         const uint8_t *, const uint8_t *, const uint32_t *, const uint8_t *, uint64_t, uint32_t *, uint64_t *) = vga_phase_tags_lists;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "tag.o")])
    assert p.binding.PHASE_TAG_COLS == 4
    hpp = open(os.path.join(CSRC, "vga_phase.hpp")).read()
    assert int(re.search(r"#define PH_TAG_COLS (\d+)u", hpp).group(1)) == 4
    for name in ("phase_tags", "phase_tags_lists"):
        assert hasattr(p.binding.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    assert L.vga_phase_tags(None, 0, None, None, None, None, None, 0, None, None, None) == -1
    assert L.vga_phase_tags_lists(None, 0, 0, None, 0, None, 0, None, None, None, None, None, None, 0, None, None) == -1


# ---- the command line: the refusal before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa"] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300, env=env)


def test_cli_haplotag_needs_phase(tmp_path):
    pkg()
    for args in (["--call-variants", "--haplotag"], ["--pileup", "--call-variants", "--call-insertions", "--haplotag"], ["--haplotag"]):
        pr = run_cli(["-D", "-G", "none.gfa"] + args, tmp_path)
        assert pr.returncode != 0 and "--haplotag" in pr.stderr and "--phase" in pr.stderr, pr.stderr
        assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
        assert not os.listdir(str(tmp_path))


def test_usage_names_the_switch():
    pkg()
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "[--phase [--phase-min-links 2] [--haplotag]]" in usage.stderr, usage.stderr


# ---- the planted sample on the oracle's text
def test_planted_haplotypes_are_told_apart(oracle):
    """Two haplotypes of one DRB1 path (phase_cases.planted_sample): reads a0 .. a11 carry the substitutions at s1 and s3, reads
    b0 .. b11 the one at s2; 1000 bases each with 1 % of each error.  In the set of the three planted sites every read has a row,
    no read goes with the other group's haplotype, and at most one read per group is undecided.  (Seen with the reference's
    defaults: 28 heterozygous sites in 3 sets; the 12 a reads on one haplotype, 11 b reads on the other, one b read tied 3 : 3.  The
    other two sets are the noisy calls at the reads' ends; they collect 16 votes per read, which is why no set is chosen per read.)"""
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    reads, at, new, old = P.planted_sample(rs, DRB1, a["node_seq_idx"])
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    calls = variant_ref.call_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    pos, x, y = phase_ref.sites_of(calls)
    obs = phase_ref.observations(ag, a["node_seq_idx"], a["seq_fwd"], pos, x, y)
    assert len(obs) == len(reads) == 24       # every read has a record: record r is read r
    ps, flip, _ = phase_ref.chain(phase_ref.tables(obs, len(pos))[0])
    rows = haplotag_ref.rows(obs, ps, flip)
    h = [pos.index(p) for p in at]
    planted = ps[h[0]]
    assert ps[h[1]] == planted and ps[h[2]] == planted
    print(len(pos), "sites in", len(set(ps)), "sets; the planted set is", planted)
    # haplotype a of the set carries flip ? y : x: the group whose reads carry the planted letter at s1 is the a reads' haplotype
    carries = "ACGT-"[y[h[0]] if flip[h[0]] else x[h[0]]]
    assert carries in (new[0], old[0])
    hap_of = {"a": "a" if carries == new[0] else "b"}
    hap_of["b"] = "b" if hap_of["a"] == "a" else "a"
    mine = {r: (va, vb) for r, p, va, vb in rows if p == planted}
    assert sorted(mine) == list(range(24)), sorted(mine)
    undecided = {"a": 0, "b": 0}
    for r, (name, _) in enumerate(reads):
        hap = haplotag_ref.hap(*mine[r])
        print(name, mine[r], hap)
        assert hap in (hap_of[name[0]], "."), (name, mine[r])
        undecided[name[0]] += hap == "."
    assert undecided["a"] <= 1 and undecided["b"] <= 1, undecided
    # the text from the GAF alone is the text of these rows
    text = haplotag_ref.tsv_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    assert text[0] == haplotag_ref.tsv(rows)[0] and text[1] == len(rows) and text[5] == 24


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def ph_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tagisa") / "ph.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_phase.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel,count,lds", [("k_ph_tagILb", 2, 0), ("k_ph_tag_scan", 1, 4 * 16)])
def test_tag_kernels_without_scratch(ph_isa, kernel, count, lds):
    """both passes of k_ph_tag and the scan: no scratch, no spill, no LDS beyond the scan's sixteen wave sums.  The fields of the
    code-object metadata only."""
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"\w*)\n", ph_isa):
        a = ph_isa.rfind("\n  - ", 0, m.start())
        b = ph_isa.find("\n  - ", m.end())
        entries.append(ph_isa[a:b if b >= 0 else len(ph_isa)])
    assert len(entries) == count, (kernel, len(entries))
    for e in entries:
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("wavefront_size") == 64 and field("group_segment_fixed_size") == lds
