"""The insertion table and the insertion call, the parts that need no GPU: the reference (tests/insertion_ref.py) on hand-made
rows -- every tie the definition names --, a planted insertion found again on the oracle's alignments GAF, the constants of
csrc/vga_insertion.hpp against the binding's and the reference's, the six vga_insertion_* calls in the ABI, the command line's
refusals, and the scratch budget of the three kernels from a cross-compile for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

import insertion_ref
import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_insertion_begin", "vga_insertion_read", "vga_insertion_reset", "vga_insertion_end", "vga_insertion_call", "vga_insertion_call_table"]
A, C, G, T, N = range(5)


def row(bins=(), letters=()):
    """a row from {length: reads} (9 for more) and {(position, letter code): reads}"""
    r = [0] * insertion_ref.COLS
    for length, v in dict(bins).items():
        r[length - 1] = v
    for (j, c), v in dict(letters).items():
        r[insertion_ref.BINS + 5 * j + c] = v
    return r


# ---- the constants
def test_constants_agree():
    hpp = open(os.path.join(CSRC, "vga_insertion.hpp")).read()
    macro = lambda name: int(re.search(r"#define " + name + r" (\d+)u", hpp).group(1))
    b = pkg().binding
    assert macro("IA_MAX_LEN") == b.INSERTION_MAX_LEN == insertion_ref.MAX_LEN == 8
    assert macro("IA_COLS") == b.INSERTION_COLS == insertion_ref.COLS == 9 + 8 * 5 == 49
    assert macro("IA_BINS") == insertion_ref.BINS == 9 and macro("IA_LETTERS") == len(insertion_ref.LETTERS) == len(b.INSERTION_LETTERS) == 5
    assert b.INSERTION_LETTERS == insertion_ref.LETTERS
    assert re.search(r"#define IA_MAX_SEQ \(1ull << 26\)", hpp) and b.INSERTION_MAX_SEQ == 1 << 26
    assert re.search(r"#define IA_MAX_COUNT \(1ull << 40\)", hpp) and b.INSERTION_MAX_COUNT == 1 << 40
    assert insertion_ref.INS_STATES == variant_ref.INS_STATES == b.VARIANT_INS_STATES


# ---- the reference on hand-made rows
def test_an_empty_row_gives_length_zero():
    assert insertion_ref.call_row(row()) == (0, 0, "", [])
    # letters without a bin cannot come from the walker; the call reads the bins first and reports nothing
    assert insertion_ref.call_row(row(letters={(0, A): 3})) == (0, 0, "", [])


def test_equal_bins_give_the_shorter_length():
    r = row({2: 5, 4: 5}, {(0, C): 10, (1, G): 10, (2, T): 5, (3, T): 5})
    assert insertion_ref.call_row(r) == (2, 5, "CG", [10, 10])
    r = row({1: 1, 2: 1, 3: 1, 8: 1}, {(0, T): 4})
    assert insertion_ref.call_row(r)[:3] == (1, 1, "T")
    r = row({3: 4, 2: 5}, {(0, A): 9, (1, A): 9, (2, A): 4})
    assert insertion_ref.call_row(r) == (2, 5, "AA", [9, 9])


def test_more_wins_only_when_strictly_larger():
    letters = {(j, G): 6 for j in range(8)}
    assert insertion_ref.call_row(row({8: 3, 9: 3}, letters)) == (8, 3, "G" * 8, [6] * 8)
    assert insertion_ref.call_row(row({1: 3, 9: 3}, {(0, G): 6, (1, G): 3}))[:3] == (1, 3, "G")
    length, reads, seq, seq_reads = insertion_ref.call_row(row({8: 3, 9: 4}, {(j, G): 7 for j in range(8)}))
    assert (length, reads, seq, seq_reads) == (9, 4, "G" * 8, [7] * 8)   # more: reported as 9, its first eight letters
    assert insertion_ref.MORE == 9


def test_letter_ties_follow_a_c_g_t_n():
    assert insertion_ref.call_row(row({1: 10}, {(0, A): 2, (0, C): 2, (0, G): 2, (0, T): 2, (0, N): 2})) == (1, 10, "A", [2])
    assert insertion_ref.call_row(row({1: 8}, {(0, C): 2, (0, G): 2, (0, T): 2, (0, N): 2})) == (1, 8, "C", [2])
    assert insertion_ref.call_row(row({1: 4}, {(0, T): 2, (0, N): 2})) == (1, 4, "T", [2])
    assert insertion_ref.call_row(row({1: 3}, {(0, T): 1, (0, N): 2})) == (1, 3, "N", [2])
    assert insertion_ref.call_row(row({2: 4}, {(0, G): 2, (0, C): 2, (1, N): 3, (1, A): 1})) == (2, 4, "CN", [2, 3])


def test_call_rows_and_wide_counters():
    m, top = 2**32 - 1, 2**40 - 1
    rows = [row(), row({3: m}, {(0, A): m, (1, C): m, (2, G): m}), row({9: top}, {(j, N): top for j in range(8)})]
    c = insertion_ref.call_rows(rows)
    assert c["length"].tolist() == [0, 3, 9] and c["length_reads"].tolist() == [0, m, top]
    assert bytes(c["seq"][1]) == b"ACG\0\0\0\0\0" and bytes(c["seq"][2]) == b"N" * 8 and not c["seq"][0].any()
    assert c["seq_reads"][1].tolist() == [m, m, m, 0, 0, 0, 0, 0] and c["seq_reads"][2].tolist() == [top] * 8
    assert insertion_ref.same(c, c) is None
    assert insertion_ref.same(c, dict(c, length=c["length"] + 1)) == "length"


def test_walker_and_tsv_on_a_hand_made_record():
    """two nodes of 6 and 5 bases; one read that inserts before any base, behind a deleted base, a run of nine with a lower-case
    foreign letter, and one at the last base"""
    idx, seq = [0, 6, 11], "ACGTACGGTCA"
    cs = "+tt:2-g+ac:3+acgtacgtn:1*ga:2+g"
    covered = 2 + 3 + 1 + 1 + 2
    gaf = "\t".join(["r", "30", "0", "30", "+", ">1>2", "11", "0", "4", str(covered), str(covered), "60", "cs:Z:" + cs + ",cg:Z:x"]) + "\n"
    counts, n_al, n_ev, leading = insertion_ref.walk(gaf, idx, seq)
    assert (n_al, n_ev, leading) == (1, 3, 1)
    assert sorted(set(np.argwhere(counts)[:, 0].tolist())) == [2, 5, 9]
    assert insertion_ref.call_row(counts[2]) == (2, 1, "AC", [1, 1])          # behind the deleted base
    assert insertion_ref.call_row(counts[5]) == (9, 1, "ACGTACGT", [1] * 8)   # the ninth letter is not kept
    assert insertion_ref.call_row(counts[9]) == (1, 1, "G", [1])
    calls = {"pos": [2, 4, 5], "ins": [2, 0, 1], "ins_qual": [700, 0, 600], "depth": [1, 1, 1], "counts": [[0] * 6 + [1]] * 3}
    text, sites, n_long = insertion_ref.tsv(calls, counts, idx)
    assert (sites, n_long) == (2, 1)
    assert text == insertion_ref.HEADER + "\n1\t2\thom\t700\t1\t1\t2\t1\tAC\t1,1\n1\t5\thet\t600\t1\t1\t>8\t1\tACGTACGT\t1,1,1,1,1,1,1,1\n"


# ---- a planted insertion on the oracle's text
def test_planted_insertion_is_called(oracle):
    """A sample from one path of DRB1 whose sequence carries three letters no path has, in the middle of a node: 12 reads of
    1000 bases with 1 % of each error, tiled so that the site moves through the read (test_variant_cpu.py's set-up).  The first
    inserted letter differs from the graph base behind the run and the last from the one before it, so the run cannot slide.
    variant_ref reports the base before the run with a homozygous insertion, insertion_ref calls length 3 and the planted letters
    there.  The other sites are the reads' own errors: printed here, recorded in DESIGN.md section 22."""
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    idx = [int(x) for x in a["node_seq_idx"]]
    segs, paths = rs.parse_gfa_paths(DRB1)
    name, steps = paths[3]
    assert not any(rev for _, rev in steps)
    off = 0
    for nid, _ in steps:
        if off >= 2000 and len(segs[nid]) >= 50:
            break
        off += len(segs[nid])
    site_path, site_graph = off + len(segs[nid]) // 2, idx[nid - 1] + len(segs[nid]) // 2   # the run goes in before this base
    seq = rs.path_sequence(segs, steps)
    before, behind = seq[site_path - 1].upper(), seq[site_path].upper()
    assert a["seq_fwd"].decode()[site_graph - 1:site_graph + 1].upper() == before + behind
    first = next(c for c in "ACGT" if c != behind)
    last = next(c for c in "ACGT" if c not in (before, first))
    middle = next(c for c in "ACGT" if c not in (first, last))
    planted = first + middle + last
    assert len(set(planted)) == 3 and planted[0] != behind and planted[-1] != before
    mut = seq[:site_path] + planted + seq[site_path:]
    n_reads, length = 12, 1000
    rng = np.random.Generator(np.random.PCG64(11))
    reads = []
    for r in range(n_reads):
        o = site_path - length + (r + 1) * length // (n_reads + 1)
        tpl = np.frombuffer(mut[o:o + length].encode(), dtype=np.uint8)
        reads.append(("planted%d" % r, rs._mutate(tpl, rng, 0.01, 0.01, 0.01).decode()))
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    calls = variant_ref.call_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    counts, n_al, n_ev, n_leading = insertion_ref.walk(ag, a["node_seq_idx"], a["seq_fwd"])
    text, sites, n_long = insertion_ref.tsv(calls, counts, a["node_seq_idx"])
    print("alignments", n_al, "insertions", n_ev, "leading", n_leading, "sites", sites, "longer than 8", n_long, "\n" + text)
    assert n_al == n_reads
    at = calls["pos"].tolist().index(site_graph - 1)   # the base consumed before the run
    assert int(calls["ins"][at]) == 2, "hom"
    got = insertion_ref.call_row(counts[site_graph - 1])
    assert got[0] == 3 and got[2] == planted, got
    assert got[1] >= n_reads - 2 and min(got[3]) >= n_reads - 2   # (a read's own error may fall on the run)
    line = [ln for ln in text.splitlines() if ln.startswith("%d\t%d\thom\t" % (nid, site_graph - 1 - idx[nid - 1]))]
    assert len(line) == 1 and line[0].split("\t")[6] == "3" and line[0].split("\t")[8] == planted, line


# ---- the ABI
def test_abi_lists_and_exports_the_six_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    assert not re.search(r"typedef\s+struct[^;]*insertion", header)   # scalars and parallel arrays: no new struct
    src = tmp_path / "ia.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*b)(vga_ctx *) = vga_insertion_begin, (*z)(vga_ctx *) = vga_insertion_reset, (*e)(vga_ctx *) = vga_insertion_end;\n"
                   "int (*r)(vga_ctx *, uint32_t *, uint64_t *, uint64_t *, uint64_t *) = vga_insertion_read;\n"
                   "int (*c)(vga_ctx *, uint64_t, const uint32_t *, uint8_t *, uint64_t *, uint8_t *, uint64_t *, uint64_t *) = vga_insertion_call;\n"
                   "int (*t)(vga_ctx *, uint64_t, const uint64_t *, uint8_t *, uint64_t *, uint8_t *, uint64_t *, uint64_t *) = vga_insertion_call_table;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "ia.o")])
    for name in ("insertion_begin", "insertions", "insertion_reset", "insertion_end", "insertion_call", "insertion_call_table"):
        assert hasattr(p.binding.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    for name in ("vga_insertion_begin", "vga_insertion_reset", "vga_insertion_end"):
        assert getattr(L, name)(None) == -1
    assert L.vga_insertion_read(None, None, None, None, None) == -1
    assert L.vga_insertion_call(None, 0, None, None, None, None, None, None) == -1
    assert L.vga_insertion_call_table(None, 0, None, None, None, None, None, None) == -1


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa", "-o", str(cwd / "out")] + args, cwd=str(cwd),
                          capture_output=True, text=True, timeout=300, env=env)


def refused(pr, cwd, *words):
    assert pr.returncode != 0
    for w in words:
        assert w in pr.stderr, pr.stderr
    # refused while the arguments are read: no index is looked for (the files do not exist), no device is opened, nothing written
    assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr
    assert os.listdir(str(cwd)) == []


def test_cli_call_insertions_needs_call_variants(tmp_path):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--call-insertions"], tmp_path), tmp_path, "--call-insertions", "--call-variants")


def test_cli_call_insertions_needs_also_align(tmp_path):
    pkg()
    refused(run_cli(["--call-insertions"], tmp_path), tmp_path, "--call-insertions", "--also-align")
    refused(run_cli(["--call-insertions", "--call-variants"], tmp_path), tmp_path, "--also-align")


def test_usage_names_the_switch():
    pkg()
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "--call-insertions" in usage.stderr, usage.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def ia_remarks():
    pr = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "vga_insertion.hip"), "-o", os.devnull], capture_output=True, text=True,
                        timeout=900)
    assert pr.returncode == 0, pr.stderr
    return pr.stderr


@pytest.mark.parametrize("kernel,copies", [("k_ia_events", 1), ("k_ia_add", 1), ("k_ia_call", 2)])
def test_insertion_kernels_without_scratch(ia_remarks, kernel, copies):
    """the compiler's resource remarks: no scratch, no spill and no LDS for the three kernels (k_ia_call once per counter type:
    32-bit for the context's own counters, 64-bit for the seam).  The VGPR counts are printed; DESIGN.md section 22 records them."""
    blocks = re.split(r"remark: Function Name: ", ia_remarks)[1:]
    mine = [b for b in blocks if re.match(r"_Z\w*?\d+" + kernel + r"[EI]", b)]
    assert len(mine) == copies, (kernel, [b.split()[0] for b in blocks])
    for b in mine:
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", b).group(1))
        print(kernel, "vgprs", field("VGPRs"), "sgprs", field("TotalSGPRs"), "occupancy", field("Occupancy [waves/SIMD]"))
        assert field("ScratchSize [bytes/lane]") == 0
        assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
        assert field("LDS Size [bytes/block]") == 0
