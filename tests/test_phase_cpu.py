"""The phase links and the phase chain, the parts that need no GPU: the reference (tests/phase_ref.py) against observations,
links and chains computed by hand, vga_phase_chain against the reference's chain, a planted phase found again on the oracle's
alignments GAF, the vga_phase_* calls in the ABI, the command line's refusals, and the scratch budget of the three kernels from a
cross-compile for gfx950.  Without the feature every test here stops at the missing symbols, files or switch."""
import os
import re
import subprocess

import numpy as np
import pytest

import phase_cases as P
import phase_ref
import variant_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_phase_begin", "vga_phase_read", "vga_phase_reset", "vga_phase_end", "vga_phase_links", "vga_phase_links_lists", "vga_phase_chain"]
A, C, G, T, D = range(5)


# ---- the reference on hand-made records
# two nodes, ACGT and ACGTAC; site 0 at base 2 (G, alleles G / T), site 1 at base 5 (C, alleles A / C)
GAF_IDX, GAF_SEQ = [0, 4, 10], "ACGTACGTAC"
GAF = "\n".join("\t".join(f) for f in [
    ["a", "10", "0", "10", "+", ">1>2", "10", "0", "6", "10", "10", "60", "as:i:-30 cs:Z::10,cg:Z:10M"],                  # own letters: x, y
    ["b", "7", "0", "7", "+", ">1>2", "10", "1", "4", "5", "7", "60", "as:i:-30 cs:Z::1*gt:2*ca:2,cg:Z:7M"],              # T = y, A = x
    ["c", "3", "0", "3", "+", ">1", "4", "0", "4", "3", "3", "60", "as:i:-30 cs:Z::2-g:1,cg:Z:2M1D1M"],                   # D at site 0: other
    ["d", "5", "0", "5", "+", ">2", "6", "0", "3", "2", "3", "60", "as:i:-30 cs:Z::1+tt*cn:1,cg:Z:1M2I2M"],               # n at site 1: other
    ["e", "5", "0", "5", "+", "*", "0", "0", "0", "0", "0", "255", "as:i:0 cs:Z:,cg:Z:"],                                  # no alignment
]) + "\n"


def test_observations_from_gaf_text():
    obs = phase_ref.observations(GAF, GAF_IDX, GAF_SEQ, [2, 5], [G, A], [T, C])
    assert obs == [[0, 1], [1, 0], [2, 3], [3, 2]]
    links, sr = phase_ref.tables(obs, 2)
    want = np.zeros((2, 8, 4), dtype=np.uint32)
    want[0, 0] = [0, 1, 1, 0]
    assert np.array_equal(links, want) and sr.tolist() == [[1, 1, 1], [1, 1, 1]]


def test_observations_from_lists_by_hand():
    for case, obs in ((P.TINY, P.TINY_OBS), (P.EDGE, P.EDGE_OBS)):
        recs, words = P.pack(case.reads)
        assert phase_ref.obs_lists(recs, words, case.pos, case.x, case.y, case.ref) == obs, case.name
    links, sr = phase_ref.tables(P.TINY_OBS, 2)
    assert np.array_equal(links, P.TINY_LINKS) and np.array_equal(sr, P.TINY_SITE_READS)
    links, sr = phase_ref.tables(P.EDGE_OBS, 5)
    assert sr.tolist() == [[3, 0, 1], [3, 1, 0], [1, 1, 2], [1, 1, 2], [0, 2, 1]]
    assert links[0, 0].tolist() == [1, 1, 0, 0] and links[1, 0].tolist() == [1, 1, 0, 0] and links[0, 3].tolist() == [0, 2, 0, 0]
    assert links[3, 0].tolist() == [0, 1, 0, 0] and not links[4].any() and not links[3, 1:].any()
    far = P.far_case()
    links, sr = phase_ref.tables(phase_ref.obs_lists(*P.pack(far.reads), far.pos, far.x, far.y, far.ref), 10)
    assert links[0, 7].tolist() == [3, 0, 2, 0] and int(links.sum()) == 5 and sr[9].tolist() == [0, 4, 0]   # nine apart: not linked


def table(n, entries):
    t = np.zeros((n, 8, 4), dtype=np.uint32)
    for (h, d), l in entries.items():
        t[h, d - 1] = l
    return t


def test_chain_by_hand():
    # the smallest d wins, though the link two back is stronger
    t = table(3, {(0, 2): [9, 0, 0, 9], (1, 1): [0, 2, 0, 0], (0, 1): [3, 0, 0, 0]})
    assert phase_ref.chain(t) == ([1, 1, 1], [0, 0, 1], [0, 1, 1])
    # cis == trans is skipped: the link two back decides
    t = table(3, {(1, 1): [2, 2, 0, 0], (0, 2): [0, 3, 0, 0]})
    assert phase_ref.chain(t) == ([1, 2, 1], [0, 0, 1], [0, 0, 2])
    # the edge of min_links: one read below it opens a set, at it the link holds
    t = table(2, {(0, 1): [3, 1, 0, 0]})
    assert phase_ref.chain(t, 3) == ([1, 2], [0, 0], [0, 0])
    assert phase_ref.chain(t, 2) == ([1, 1], [0, 0], [0, 1])
    t = table(2, {(0, 1): [0, 1, 0, 0]})
    assert phase_ref.chain(t, 2) == ([1, 2], [0, 0], [0, 0]) and phase_ref.chain(t, 1) == ([1, 1], [0, 1], [0, 1])
    # a flip goes through two links: trans, trans is cis again; trans, cis stays flipped
    t = table(4, {(0, 1): [0, 4, 4, 0], (1, 1): [0, 0, 5, 0], (2, 1): [6, 0, 0, 1]})
    assert phase_ref.chain(t) == ([1, 1, 1, 1], [0, 1, 0, 0], [0, 1, 1, 1])
    # a new set is numbered by its line, and later sites join it
    t = table(4, {(0, 1): [5, 0, 0, 0], (2, 1): [0, 0, 7, 0]})
    assert phase_ref.chain(t) == ([1, 1, 3, 3], [0, 0, 0, 1], [0, 1, 0, 1])
    assert phase_ref.chain(table(0, {})) == ([], [], [])
    # a link nine back does not exist: eight back is the furthest
    t = table(10, {(0, 8): [4, 0, 0, 0]})
    ps, flip, link_d = phase_ref.chain(t)
    assert ps == [1, 2, 3, 4, 5, 6, 7, 8, 1, 10] and link_d[8] == 8


def test_tsv_by_hand():
    links = table(3, {(0, 1): [0, 4, 5, 0], (0, 2): [9, 9, 9, 9]})
    sr = np.array([[5, 4, 1], [5, 4, 0], [2, 2, 2]], dtype=np.uint32)
    text, n, sets = phase_ref.tsv([2, 5, 9], [G, A, C], [T, C, D], links, sr, GAF_IDX)
    assert (n, sets) == (3, 2)
    assert text == (phase_ref.HEADER + "\n1\t2\tG|T\t1\t0\t0\t0\t5\t4\t1\n2\t1\tC|A\t1\t1\t0\t9\t5\t4\t0\n2\t5\tC|-\t3\t0\t0\t0\t2\t2\t2\n")
    assert phase_ref.tsv([], [], [], table(0, {}), np.zeros((0, 3)), GAF_IDX) == (phase_ref.HEADER + "\n", 0, 0)


# ---- the library's chain, without a context
def test_library_chain_equals_the_reference():
    b = pkg().binding
    rng = np.random.default_rng(3)
    for n, hi, min_links in [(0, 2, 2), (1, 2, 2), (2, 3, 1), (9, 3, 2), (10, 4, 2), (300, 3, 2), (300, 6, 3), (300, 2**31, 65535), (64, 2**32, 2)]:
        links = rng.integers(0, hi, size=(n, 8, 4), dtype=np.uint64).astype(np.uint32)
        links[rng.integers(0, 2, size=(n, 8)).astype(bool)] = 0    # and windows where the nearest sites say nothing
        ps, flip, link_d = b.phase_chain(links, min_links)
        assert (ps.tolist(), flip.tolist(), link_d.tolist()) == phase_ref.chain(links, min_links), (n, hi, min_links)
        assert ps.dtype == np.uint32 and flip.dtype == np.uint8 and link_d.dtype == np.uint8
    for bad in (0, 65536, 2**32 - 1):
        with pytest.raises(b.VgaError) as e:
            b.phase_chain(np.zeros((2, 8, 4), dtype=np.uint32), bad)
        assert e.value.code == -1


# ---- the ABI
def test_abi_lists_and_exports_the_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert getattr(L, name) is not None
    assert L.vga_abi_version() == 6
    assert not re.search(r"typedef\s+struct[^;]*phase", header)   # scalars and parallel arrays: no new struct
    src = tmp_path / "ph.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*b)(vga_ctx *) = vga_phase_begin;\nint (*r)(vga_ctx *) = vga_phase_reset;\nint (*e)(vga_ctx *) = vga_phase_end;\n"
                   "int (*d)(vga_ctx *, uint32_t *, uint32_t *, uint64_t *, uint64_t *) = vga_phase_read;\n"
                   "int (*l)(vga_ctx *, uint64_t, const uint32_t *, const uint8_t *, const uint8_t *, uint32_t *, uint32_t *, uint64_t *) = vga_phase_links;\n"
                   "int (*s)(vga_ctx *, uint64_t, uint64_t, const uint32_t *, uint64_t, const uint32_t *, uint64_t, const uint32_t *, const uint8_t *,\n"
                   "         const uint8_t *, const uint8_t *, uint32_t *, uint32_t *) = vga_phase_links_lists;\n"
                   "int (*c)(uint64_t, const uint32_t *, uint32_t, uint32_t *, uint8_t *, uint8_t *) = vga_phase_chain;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "ph.o")])
    b = p.binding
    assert (b.PHASE_WINDOW, b.PHASE_MIN_LINKS, b.PHASE_MAX_MIN_LINKS) == (phase_ref.WINDOW, phase_ref.MIN_LINKS, 65535) == (8, 2, 65535)
    hpp = open(os.path.join(CSRC, "vga_phase.hpp")).read()
    for macro, value in [("PH_WINDOW", 8), ("PH_MIN_LINKS_DEFAULT", 2), ("PH_MIN_LINKS_MAX", 65535), ("PH_COLS", b.PHASE_COLS)]:
        assert int(re.search(r"#define " + macro + r" (\d+)u", hpp).group(1)) == value
    for name in ("phase_begin", "phase_reads", "phase_reset", "phase_end", "phase_links", "phase_links_lists"):
        assert hasattr(b.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    for name in ("vga_phase_begin", "vga_phase_reset", "vga_phase_end"):
        assert getattr(L, name)(None) == -1
    assert L.vga_phase_read(None, None, None, None, None) == -1
    assert L.vga_phase_links(None, 0, None, None, None, None, None, None) == -1
    assert L.vga_phase_links_lists(None, 0, 0, None, 0, None, 0, None, None, None, None, None, None) == -1
    assert L.vga_phase_chain(0, None, 2, None, None, None) == 0    # no context to be null: no sites, nothing to write
    assert L.vga_phase_chain(1, None, 2, None, None, None) == -1
    assert L.vga_phase_chain(0, None, 0, None, None, None) == -1


# ---- the command line: refusals before anything is opened or written
def run_cli(args, cwd):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")  # (no device to open: a refusal cannot depend on one)
    return subprocess.run([EXE, "map", "-i", str(cwd / "none"), "-f", str(cwd / "none.fa"), "-p", "abpoa"] + args, cwd=str(cwd), capture_output=True,
                          text=True, timeout=300, env=env)


def refused(pr, *words):
    assert pr.returncode != 0
    for w in words:
        assert w in pr.stderr, pr.stderr
    assert pr.stderr.strip().count("\n") == 0 and "device" not in pr.stderr.lower() and "hip" not in pr.stderr.lower(), pr.stderr


def test_cli_phase_needs_call_variants(tmp_path):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--phase"], tmp_path), "--phase", "--call-variants")
    refused(run_cli(["-D", "-G", "none.gfa", "--pileup", "--phase"], tmp_path), "--phase", "--call-variants")


def test_cli_min_links_needs_the_switch(tmp_path):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--call-variants", "--phase-min-links", "3"], tmp_path), "--phase-min-links", "--phase")


@pytest.mark.parametrize("value", ["0", "65536", "x", "-1", "2.5", ""])
def test_cli_refuses_min_links_out_of_range(tmp_path, value):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--call-variants", "--phase", "--phase-min-links", value], tmp_path), "--phase-min-links")


def test_usage_names_the_switch():
    pkg()
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    for w in ("--phase", "--phase-min-links 2"):
        assert w in usage.stderr, usage.stderr


# ---- a planted phase on the oracle's text
def test_planted_phase_is_found(oracle):
    """Two haplotypes of one DRB1 path (phase_cases.planted_sample): A carries substitutions at s1 and s3, B at s2, 12 reads of
    1000 bases each with 1 % of each error.  The reference reports the three sites heterozygous, in one phase set, the planted
    letters of s1 and s3 on one haplotype and that of s2 on the other.  The other heterozygous calls of this sample are the
    reads' ends and errors (deletions at depth 4 to 9); none of them lies between the three sites."""
    rs = pkg().readsim
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    reads, at, new, old = P.planted_sample(rs, DRB1, a["node_seq_idx"])
    assert at[0] < at[1] < at[2] < at[0] + 300
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    calls = variant_ref.call_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    pos, x, y = phase_ref.sites_of(calls)
    links, sr = phase_ref.links_gaf(ag, a["node_seq_idx"], a["seq_fwd"], pos, x, y)
    ps, flip, link_d = phase_ref.chain(links)
    text, n_sites, n_sets = phase_ref.tsv(pos, x, y, links, sr, a["node_seq_idx"])
    print(text, n_sites, n_sets)
    h = [pos.index(p) for p in at]
    for k in range(3):
        assert sorted("ACGT"[v] for v in (x[h[k]], y[h[k]])) == sorted((old[k], new[k])), k
    assert ps[h[0]] == ps[h[1]] == ps[h[2]]
    hap_a = ["ACGT-"[y[i] if flip[i] else x[i]] for i in h]
    hap_b = ["ACGT-"[x[i] if flip[i] else y[i]] for i in h]
    assert (hap_a, hap_b) in (([new[0], old[1], new[2]], [old[0], new[1], old[2]]), ([old[0], new[1], old[2]], [new[0], old[1], new[2]]))
    assert h[2] - h[0] - 2 == 0, "spurious heterozygous calls between the planted sites"
    assert h[2] - h[0] - 2 <= 7
    assert [int(v) for v in sr[h[1]]] == [12, 12, 0]
    assert text == phase_ref.tsv_gaf(ag, a["node_seq_idx"], a["seq_fwd"])[0]


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def ph_isa(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("phisa") / "ph.s")
    subprocess.check_call([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                           os.path.join(CSRC, "vga_phase.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return open(out).read()


@pytest.mark.parametrize("kernel,lds", [("k_ph_keep", 0), ("k_ph_obs", 0), ("k_ph_link", 4 * 35 * 4)])
def test_phase_kernels_without_scratch(ph_isa, kernel, lds):
    """no scratch, no spill, and no LDS beyond the four waves' 32 link counts and 3 site counts"""
    entries = []
    for m in re.finditer(r"\.name:\s+(_Z\w*?\d+" + kernel + r"\w*)\n", ph_isa):
        a = ph_isa.rfind("\n  - ", 0, m.start())
        b = ph_isa.find("\n  - ", m.end())
        entries.append(ph_isa[a:b if b >= 0 else len(ph_isa)])
    assert len(entries) == 1, (kernel, len(entries))
    for e in entries:
        field = lambda f: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1))
        print(kernel, "vgprs", field("vgpr_count"), "sgprs", field("sgpr_count"), "lds", field("group_segment_fixed_size"))
        assert field("private_segment_fixed_size") == 0
        assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
        assert field("wavefront_size") == 64 and field("group_segment_fixed_size") == lds
