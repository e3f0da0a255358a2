"""The deletion call, the parts that need no GPU: the reference walker (tests/deletion_ref.py) on a hand-made record, the rule --
every tie, reads above depth, the saturation and the three thresholds -- in the reference and in the library's export, a planted
deletion found again on the oracle's alignments GAF, the conditions tests/deletion_cases.py is there for, the constants of
csrc/vga_deletion.hpp against the binding's, the calls in the ABI, the command line's refusals, and the resources of the k_dl_*
kernels from a cross-compile for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

import deletion_cases
import deletion_ref
import op_cases as M
import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
CSRC = os.path.join(ROOT, "rs-vgaligner_amd", "csrc")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
HIPCC = "/opt/rocm/bin/hipcc"
CALLS = ["vga_deletion_begin", "vga_deletion_read", "vga_deletion_reset", "vga_deletion_end", "vga_deletion_call", "vga_deletion_call_table"]
NONE, HET, HOM = deletion_ref.NONE, deletion_ref.HET, deletion_ref.HOM
E = deletion_ref.ERROR


# ---- the constants
def test_constants_agree():
    hpp = open(os.path.join(CSRC, "vga_deletion.hpp")).read()
    macro = lambda name: int(re.search(r"#define " + name + r" (\d+)u", hpp).group(1))
    b = pkg().binding
    assert macro("DL_EVENT_WORDS") == b.DELETION_EVENT_WORDS == deletion_ref.EVENT_WORDS == 3
    assert int(re.search(r"#define DL_STORE_EVENTS0 (\d+)ull", hpp).group(1)) == b.DELETION_STORE_EVENTS0
    assert re.search(r"#define DL_MAX_EVENTS 0xFFFFFFFFull", hpp) and b.DELETION_MAX_EVENTS == 2**32 - 1
    assert re.search(r"#define DL_MAX_COUNT \(1ull << 40\)", hpp) and b.DELETION_MAX_COUNT == 1 << 40
    assert (macro("DL_NONE"), macro("DL_HET"), macro("DL_HOM")) == (NONE, HET, HOM) == (0, 1, 2)
    assert b.DELETION_STATES == deletion_ref.STATES == ("none", "het", "hom")
    assert (deletion_ref.ERROR, deletion_ref.MIN_DEPTH, deletion_ref.MIN_QUAL) == (b.VARIANT_ERROR, b.VARIANT_MIN_DEPTH, b.VARIANT_MIN_QUAL)


# ---- the reference walker
def test_walker_on_a_hand_made_record():
    """a record over two nodes (1 and 3 of an index of three: 6, 3 and 5 bases).  It opens with a run (an end run), crosses the
    node boundary with a run of four whose bases are not contiguous on the linearised graph, has a run directly behind an
    insertion, and closes with a run behind a trailing insertion (an end run)."""
    idx, seq = [0, 6, 9, 14], "ACGTAC" + "TTT" + "GGTCA"
    #     -a (0) | :2 | -tacg (3 4 5 | 9) | :1 | +gg -t (11) | *ca (12) | +c | -a (13)
    cs = "-a:2-tacg:1+gg-t*ca+c-a"
    covered = 2 + 1 + 1
    gaf = "\t".join(["r", "10", "0", "10", "+", ">1>3", "11", "0", "5", str(covered), str(covered), "60", "cs:Z:" + cs + ",cg:Z:x"]) + "\n"
    events, n_al, n_end = deletion_ref.walk(gaf, idx)
    assert (n_al, n_end) == (1, 2)
    assert events.dtype == np.uint32 and events.tolist() == [[3, 4, 9], [11, 1, 11]]   # last - first = 6 != len - 1 = 3: it crosses
    counts = pileup_ref.walk(gaf, idx, seq)[0]
    assert np.flatnonzero(counts[:, pileup_ref.DEL]).tolist() == [0, 3, 4, 5, 9, 11, 13]   # the end runs count in the pileup
    deletion_ref.check_against_pileup(events, counts)
    with pytest.raises(AssertionError):
        deletion_ref.check_against_pileup(np.array([[3, 4, 9], [3, 1, 3]], dtype=np.uint32), counts)
    # a record without a match: every run is an end run, once
    gaf2 = "\t".join(["q", "2", "0", "2", "+", ">1", "6", "0", "6", "0", "0", "60", "cs:Z:-acg+tt-tac,cg:Z:x"]) + "\n"
    ev2, n_al2, n_end2 = deletion_ref.walk(gaf2, idx)
    assert (len(ev2), n_al2, n_end2) == (0, 1, 2)
    # two adjacent - tokens are refused
    with pytest.raises(AssertionError):
        deletion_ref.record_runs(["-a", "-c"], [1], 0, idx)
    calls = deletion_ref.call(np.array([[3, 4, 9]] * 5 + [[11, 1, 11]], dtype=np.uint32), np.array([[0, 0, 0, 0, 0, 5, 0]] * 14), E, 4, 512)
    assert (calls["n_distinct"], calls["n_calls"]) == (2, 1)
    assert deletion_ref.tsv(calls, idx) == deletion_ref.HEADER + "\n1\t3\t3\t0\t4\thom\t1280\t5\t5\n"


# ---- the rule
def both(reads, depth, error=E):
    """the reference's rule and the library's export agree; -> (state, qual)"""
    want = deletion_ref.rule(reads, depth, error)
    assert pkg().binding.deletion_state(reads, depth, error) == want, (reads, depth, error)
    return want


def test_rule_ties_go_to_the_first_of_none_het_hom():
    assert both(0, 0) == (NONE, 0)                     # all three cost nothing
    assert both(0, 10) == (NONE, 2560)                 # none 0, het 2560, hom 12800
    assert both(1, 5, 1280) == (NONE, 0)               # none 1280 = het 1280 < hom 5120: none before het
    assert both(5, 10, 512) == (NONE, 0)               # none = het = hom = 2560: none first
    assert both(5, 10, 1280) == (HET, 3840)            # none 6400 = hom 6400 > het 2560
    assert both(4, 5, 1280) == (HET, 0)                # het 1280 = hom 1280 < none 5120: het before hom
    assert both(1, 2, 512) == (NONE, 0)                # none 512 = het 512 = hom 512
    assert both(3, 6, 512) == (NONE, 0)
    assert both(12, 12) == (HOM, 3072)
    assert both(11, 12) == (HOM, 1792) and both(11, 24) == (HET, 7936)   # the planted samples' figures


def test_rule_takes_the_smaller_of_reads_and_depth():
    assert both(9, 4) == both(4, 4) == (HOM, 1024)     # k = 4: none 5120, het 1024, hom 0
    assert both(2**33, 3) == both(3, 3)


def test_rule_saturates_qual():
    assert both(0, 2**24) == (NONE, 2**32 - 1)         # het 2^32 above none
    assert both(0, 2**24 - 1) == (NONE, 2**32 - 256)
    assert both(2**40, 2**40, 8192) == (HOM, 2**32 - 1)
    assert both(6 * 2**40 - 6, 6 * 2**40 - 6, 8192)[0] == HOM   # the largest depth a table can hold


def test_thresholds_of_a_reported_group():
    counts = np.zeros((8, 7), dtype=np.uint64)
    counts[2, :6] = (1, 1, 0, 0, 0, 2)    # depth 4
    counts[3, :6] = (0, 1, 0, 0, 0, 2)    # depth 3
    ev = np.array([[2, 2, 3]] * 4 + [[3, 1, 3]] * 3, dtype=np.uint32)
    assert deletion_ref.rule(4, 4) == (HOM, 1024) and deletion_ref.rule(3, 3) == (HOM, 768)
    got = deletion_ref.call(ev, counts, E, 4, 1024)    # depth at min_depth and one below it; qual at min_qual
    assert got["first"].tolist() == [2] and got["depth"].tolist() == [4] and got["n_distinct"] == 2
    assert deletion_ref.call(ev, counts, E, 4, 1025)["n_calls"] == 0   # qual one below min_qual
    assert deletion_ref.call(ev, counts, E, 3, 768)["first"].tolist() == [2, 3]
    assert deletion_ref.call(ev, counts, E, 3, 769)["first"].tolist() == [2]
    assert deletion_ref.call(ev, counts, E, 5, 0)["n_calls"] == 0
    # a group that is called none is never reported, whatever the thresholds
    assert deletion_ref.call(np.array([[2, 2, 3]], dtype=np.uint32), np.full((8, 7), 10), E, 1, 0)["n_calls"] == 0


# ---- a planted deletion on the oracle's text
PLANTED = deletion_cases.PLANTED


def planted_samples(oracle):
    """-> (oracle index of DRB1, its arrays, node id, graph position of the first deleted base, {sample: [(name, read)]})"""
    ix = oracle.Index(oracle.Graph.from_gfa(DRB1), 11)
    a = oracle_index_arrays(ix)
    nid, site, samples = deletion_cases.planted_reads(a["node_seq_idx"])
    return ix, a, nid, site, samples


@pytest.mark.parametrize("sample,state,depth", [("hom", "hom", 12), ("het", "het", 24)])
def test_planted_deletion_is_called(oracle, sample, state, depth):
    """exactly one event has at least 6 reads: length 12, inside the node, at least 10 reads; hom in the 12-read sample and het in
    the 24-read sample.  The figures are printed (README, "Deletion call")."""
    ix, a, nid, site, samples = planted_samples(oracle)
    reads = samples[sample]
    _, ag, _ = oracle.map_reads(ix, [n for n, _ in reads], [s for _, s in reads])
    text, message, _ = deletion_ref.tsv_gaf(ag, a["node_seq_idx"], a["seq_fwd"])
    everything = deletion_ref.tsv_gaf(ag, a["node_seq_idx"], a["seq_fwd"], deletion_ref.ERROR, 1, 0)[2]
    print(sample, "node", nid, "site", site, message, "\n" + text)
    print("all groups (reads, state, qual):", sorted(zip(everything["reads"].tolist(), everything["state"].tolist(), everything["qual"].tolist()), reverse=True)[:6])
    events = deletion_ref.walk(ag, a["node_seq_idx"])[0]
    groups = {}
    for e in events.tolist():
        groups[tuple(e)] = groups.get(tuple(e), 0) + 1
    big = [(k, v) for k, v in groups.items() if v >= 6]
    assert len(big) == 1, big
    (first, length, last), n = big[0]
    idx = [int(x) for x in a["node_seq_idx"]]
    assert length == PLANTED and last - first == PLANTED - 1 and idx[nid - 1] <= first and last < idx[nid] and n >= 10
    assert first == site
    lines = [ln.split("\t") for ln in text.splitlines()[1:] if int(ln.split("\t")[8]) >= 6]
    assert len(lines) == 1 and lines[0][:6] == [str(nid), str(first - idx[nid - 1]), str(nid), str(last - idx[nid - 1]), str(PLANTED), state], lines
    assert int(lines[0][7]) == depth


# ---- the case module
def test_the_case_sets_hold_what_they_are_run_for(oracle, tmp_path):
    """from the oracle's text alone.  A run directly behind an insertion is not among them: the oracle writes the deletion first
    (deletion_cases.py); the count is printed."""
    cond = {}
    for c in deletion_cases.all_cases(tmp_path):
        gfa = M.gfa_path(c, tmp_path)
        ix = oracle.Index(oracle.Graph.from_gfa(gfa), c.k)
        cond[c.name] = deletion_cases.conditions(M.alignments(oracle, ix, c), M.node_lengths(gfa))
        print(c.name, {k: (sorted(v) if isinstance(v, set) else v) for k, v in cond[c.name].items()})
    lanes, blocks, pairs = cond["drb5-del-lanes"], cond["drb5-del-blocks"], cond["drb5-del-pairs"]
    assert {0, 63} <= lanes["first_lane"] and {0, 63} <= lanes["closing_lane"]
    assert set(deletion_cases.BLOCK_LENGTHS) <= blocks["lengths"]
    assert {(63, 0), (64, 1), (65, 1), (128, 2), (129, 2), (129, 3)} <= blocks["blocks"], "a run inside one block, over two and over three"
    assert {0, 63} <= pairs["pair_lane"], "two runs separated by a single match on lane 63 and on lane 0"
    assert cond["drb1-del-ins"]["before_ins"] >= 4
    for c in ("drb5-del-lanes", "drb5-del-blocks", "drb5-del-pairs"):
        assert cond[c]["leading"] > 0 and cond[c]["trailing"] > 0, "end runs"
    assert max(cond["drb1-del-nodes"]["crossings"]) > 1 and 1 in cond["drb1-del-nodes"]["crossings"]
    assert max(cond["synth-del-nodes"]["crossings"]) > 1 and 1 in cond["synth-del-nodes"]["crossings"]
    print("runs directly behind an insertion:", sum(c["behind_ins"] for c in cond.values()))


# ---- the ABI
def test_abi_lists_and_exports_the_calls(tmp_path):
    p = pkg()
    header = open(os.path.join(ROOT, "include", "vga_hip.h")).read()
    L = p.binding.load_library()
    for name in CALLS:
        assert name in p.binding.ABI_SYMBOLS, name
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*vga_ctx\s*\*", header), name
        assert getattr(L, name) is not None
    assert "vga_deletion_state" in p.binding.ABI_SYMBOLS and L.vga_deletion_state is not None
    assert L.vga_abi_version() == 6
    assert not re.search(r"typedef\s+struct[^;]*deletion", header)   # scalars and parallel arrays: no new struct
    outs = "uint64_t, uint32_t *, uint32_t *, uint32_t *, uint8_t *, uint32_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t *"
    src = tmp_path / "dl.c"
    src.write_text('#include "vga_hip.h"\n'
                   "int (*b)(vga_ctx *) = vga_deletion_begin, (*z)(vga_ctx *) = vga_deletion_reset, (*e)(vga_ctx *) = vga_deletion_end;\n"
                   "int (*r)(vga_ctx *, uint32_t *, uint64_t *, uint64_t *, uint64_t *) = vga_deletion_read;\n"
                   "int (*c)(vga_ctx *, uint32_t, uint64_t, uint64_t, " + outs + ") = vga_deletion_call;\n"
                   "int (*t)(vga_ctx *, uint64_t, const uint32_t *, uint64_t, const uint64_t *, uint32_t, uint64_t, uint64_t, " + outs + ") = vga_deletion_call_table;\n"
                   "uint32_t (*s)(uint64_t, uint64_t, uint32_t, uint32_t *) = vga_deletion_state;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                           str(tmp_path / "dl.o")])
    for name in ("deletion_begin", "deletions", "deletion_reset", "deletion_end", "deletion_call", "deletion_call_table"):
        assert hasattr(p.binding.Context, name), name


def test_null_context_return_codes():
    L = pkg().binding.load_library()
    for name in ("vga_deletion_begin", "vga_deletion_reset", "vga_deletion_end"):
        assert getattr(L, name)(None) == -1
    assert L.vga_deletion_read(None, None, None, None, None) == -1
    assert L.vga_deletion_call(None, 1280, 4, 512, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.vga_deletion_call_table(None, 0, None, 0, None, 1280, 4, 512, 0, None, None, None, None, None, None, None, None, None) == -1
    assert L.vga_deletion_state(3, 3, 1280, None) == HOM   # (qual may be NULL)


def test_the_rule_header_compiles_alone(tmp_path):
    """csrc/vga_deletion.hpp is plain C++ down to its #ifdef: a host compiler builds the rule from it"""
    src = tmp_path / "rule.cpp"
    src.write_text('#include "vga_deletion.hpp"\n#include <cstdio>\nint main() { uint32_t q = 0; const uint32_t s = dl_rule(11, 24, 1280, &q); '
                   'std::printf("%s %u %d\\n", dl_state_name(s), q, (int)dl_reported(s, q, 24, 4, 512)); return 0; }\n')
    exe = tmp_path / "rule"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", CSRC, str(src), "-o", str(exe)])
    assert subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout == "het 7936 1\n"


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


def test_cli_call_deletions_needs_call_variants(tmp_path):
    pkg()
    refused(run_cli(["-D", "-G", "none.gfa", "--call-deletions"], tmp_path), tmp_path, "--call-deletions", "--call-variants")


def test_cli_call_deletions_needs_also_align(tmp_path):
    pkg()
    refused(run_cli(["--call-deletions"], tmp_path), tmp_path, "--call-deletions", "--also-align")
    refused(run_cli(["--call-deletions", "--call-variants"], tmp_path), tmp_path, "--also-align")


def test_usage_names_the_switch():
    pkg()
    usage = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert "--call-deletions" in usage.stderr, usage.stderr


# ---- the kernels, cross-compiled
@pytest.fixture(scope="module")
def dl_remarks():
    pr = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                         "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, "vga_deletion.hip"), "-o", os.devnull], capture_output=True, text=True,
                        timeout=900)
    assert pr.returncode == 0, pr.stderr
    return pr.stderr


@pytest.mark.parametrize("kernel,copies", [("k_dl_events", 1), ("k_dl_keep", 1), ("k_dl_keys", 1), ("k_dl_gather", 1), ("k_dl_heads", 1), ("k_dl_starts", 1),
                                           ("k_dl_group", 2), ("k_dl_emit", 2)])
def test_deletion_kernels_without_scratch(dl_remarks, kernel, copies):
    """the compiler's resource remarks: no scratch, no spill and no LDS for the k_dl_* kernels (the group and emit kernels once per
    counter type: 32-bit for the context's own pileup, 64-bit for the seam).  The register counts are printed."""
    blocks = re.split(r"remark: Function Name: ", dl_remarks)[1:]
    mine = [b for b in blocks if re.match(r"_Z\w*?\d+" + kernel + r"[EI]", b)]
    assert len(mine) == copies, (kernel, [b.split()[0] for b in blocks])
    for b in mine:
        field = lambda f: int(re.search(re.escape(f) + r": (\d+)", b).group(1))
        print(kernel, "vgprs", field("VGPRs"), "sgprs", field("TotalSGPRs"), "occupancy", field("Occupancy [waves/SIMD]"))
        assert field("ScratchSize [bytes/lane]") == 0
        assert field("SGPRs Spill") == 0 and field("VGPRs Spill") == 0
        assert field("LDS Size [bytes/block]") == 0
