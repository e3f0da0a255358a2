"""k_poa_text, k_cov_runs and k_pu_events on the case sets of tests/op_cases.py: events planted on every lane of a 64-operation
block, the closing operation alone in a block, runs that hold whole blocks, run lengths up to five digits
(tests/test_op_cases_cpu.py shows from the oracle alone that the sets hold them).  Per set one map + align call with coverage,
pileup and path support counting; every comparison is exact equality: the records against the oracle's alignments GAF
(helpers.assert_record_equals), the tables against the reference walkers over that GAF.  The block-edge and digit sets run again
on the routes around the kernels' defaults: text on the host, a text arena and lists too small for all problems of the call;
three of the DRB1 and synthetic sets run once more with no room for any list, so that the host's walk builds them all."""
import collections
import re

import numpy as np
import pytest

import coverage_ref
import op_cases as M
import path_support_ref
import pileup_ref
from helpers import assert_record_equals, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

Want = collections.namedtuple("Want", "side lines coverage pileup support")
ACC = ("sum_bases", "sum_edges", "top", "top_alone")


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def wants(oracle, tmp_path_factory):
    """name -> the oracle's side of a case set and the three walkers' tables over its GAF, computed once"""
    out = {}
    for name, s in M.oracle_side(oracle, tmp_path_factory.mktemp("op_cases")).items():
        a = oracle_index_arrays(s.index)
        node_len, paths = path_support_ref.parse_gfa(s.gfa)
        assert paths, name
        out[name] = Want(s, s.gaf.splitlines(), coverage_ref.walk(s.gaf, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"]),
                         pileup_ref.walk(s.gaf, a["node_seq_idx"], a["seq_fwd"]), path_support_ref.walk(s.gaf, node_len, paths))
    return out


def same_table(got, want, what):
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), [int(got[tuple(i)]) for i in bad[:8]], [int(want[tuple(i)]) for i in bad[:8]])


def run(ctx, w, what):
    """one map + align call of the set with the three counters on; every record and every table against the oracle's side"""
    p = pkg()
    case = w.side.case
    upload_oracle_index(ctx, w.side.index)
    g = p.hostlib.gfa_paths(w.side.gfa)
    ctx.coverage_begin()
    ctx.pileup_begin()
    assert ctx.path_support_begin(g["step_off"], g["steps"]) == 0
    b = None
    try:
        mp = p.default_map_params()
        if case.both_strands:
            mp.strands = p.binding.VGA_STRANDS_BOTH
        b = ctx.batch(case.reads)
        mo = b.map(mp)
        al = b.align(mo)
        if case.both_strands:  # (a '-' record carries the forward path and the cs of the reverse complement)
            assert mo.strand.tolist() == [i % 2 for i in range(len(case.reads))], what
        assert len(w.lines) == len(case.reads) and int(al.aligned.sum()) == len(case.reads), what
        for r, line in enumerate(w.lines):
            assert_record_equals(al, r, line)
        base, node, edge, n_cov = ctx.coverage()
        assert n_cov == w.coverage[3], what
        for name, got, want in zip(("base_depth", "node_reads", "edge_reads"), (base, node, edge), w.coverage):
            same_table(got, want, (what, name))
        counts, n_pu, leading = ctx.pileup()
        assert (n_pu, leading) == (w.pileup[1], w.pileup[2]), (what, "pileup totals", n_pu, leading, w.pileup[1:])
        same_table(counts, w.pileup[0], (what, "pileup"))
        acc = ctx.path_support()
        assert (acc["n_alignments"], acc["n_unplaced"]) == (w.support["n_alignments"], w.support["n_unplaced"]), what
        for k in ACC:
            assert acc[k].dtype == np.uint64 and acc[k].tolist() == w.support[k].tolist(), (what, k)
        last = ctx.path_support_last()
        same_table(last[0], w.support["bases"], (what, "path support: bases"))
        same_table(last[1], w.support["edges"], (what, "path support: edges"))
        return al
    finally:
        if b is not None:
            b.close()
        ctx.path_support_end()
        ctx.pileup_end()
        ctx.coverage_end()


SETS = ("drb5-digits", "drb5-edges", "drb1-runs", "drb1-sweep", "drb1-entries", "synth-nodes", "drb1-both-strands")


def built_by_host(trace, what):
    """problems of the traced call whose run list / pileup list found no room in the call's buffer: the host built it"""
    return len(re.findall(r"no room for its " + what, trace))


@pytest.mark.parametrize("name", SETS)
def test_case_set(ctx, wants, monkeypatch, capfd, name):
    """The buffer of pileup lists is sized by the reads of the call, a list by the mismatches and deleted bases: on DRB5, where
    a read of 700 bases deletes 12 000, most pileup lists find no room and the host builds them.  Every other set must keep all
    its lists on the device -- they hold every condition the pileup kernel needs (tests/test_op_cases_cpu.py)."""
    assert tuple(wants) == SETS
    monkeypatch.setenv("VGA_TRACE", "1")
    capfd.readouterr()
    al = run(ctx, wants[name], name)
    trace = capfd.readouterr().err
    assert al.poa_problems == len(wants[name].lines)
    print(name, "run lists built by the host:", built_by_host(trace, "run list"), "pileup lists:", built_by_host(trace, "pileup list"))
    assert built_by_host(trace, "run list") == 0
    if wants[name].side.case.graph != "drb5":
        assert built_by_host(trace, "pileup list") == 0


# ---- the routes, on the block-edge and digit sets
@pytest.mark.parametrize("name", M.BLOCK_EDGE_SETS)
def test_text_on_the_host_is_the_same(ctx, wants, monkeypatch, name):
    monkeypatch.setenv("VGA_POA_TEXT", "host")
    run(ctx, wants[name], name + ", VGA_POA_TEXT=host")
    assert "poa_text" not in [t["name"] for t in ctx.kernel_times()]


def text_bytes(line):
    """what k_poa_text claims in the arena for a record: cs (with its cs:Z:) and CIGAR, padded to four, a word per path node;
    claims are rounded up to 16"""
    f = line.split("\t")
    cs, cg = re.search(r"(cs:Z:[^,\s]*),cg:Z:(\S+)", f[12]).groups()
    return (((len(cs) + len(cg) + 3) & ~3) + 4 * f[5].count(">") + 15) & ~15


@pytest.mark.parametrize("name", M.BLOCK_EDGE_SETS)
def test_text_arena_too_small_for_some_problems(ctx, wants, monkeypatch, capfd, name):
    """an arena that holds the largest text of the set and not all of them: whichever problem of a launch claims first finds
    room, and a launch that holds them all leaves some to the host.  The library's trace counts, launch by launch, the problems
    whose text found no room (a list that finds no room brings the operations back too, under another line)."""
    w = wants[name]
    need = [text_bytes(ln) for ln in w.lines]
    assert max(need) < sum(need) // 2
    monkeypatch.setenv("VGA_POA_TEXT_ARENA", str(max(need)))
    monkeypatch.setenv("VGA_TRACE", "1")
    capfd.readouterr()
    al = run(ctx, w, name + ", small text arena")
    trace = capfd.readouterr().err
    assert al.poa_problems == len(w.lines)
    fell_back = sum(int(x) for x in re.findall(r"the text arena was too small for (\d+) of \d+ problems", trace))
    print("text built by the host:", fell_back, "of", al.poa_problems)
    assert 0 < fell_back < al.poa_problems, "some strings from the device, some encoded by the host"
    assert "poa_text" in [t["name"] for t in ctx.kernel_times()]


def list_words(rec):
    """upper bounds of the words of a record's run list (k_cov_runs) and pileup list (k_pu_events): a run of M operations or of
    matches ends at most at every change of column kind and at every node entry"""
    rr = M.runs(rec)
    breaks = len(rr) + len(rec.entries)
    sparse = sum(n for k, _, n in rr if k in "XD") + sum(k == "I" for k, _, _ in rr)
    return len(rec.path) + 2 * breaks, 2 * breaks + sparse


@pytest.mark.parametrize("name", M.BLOCK_EDGE_SETS)
def test_lists_too_small_for_some_problems(ctx, wants, monkeypatch, capfd, name):
    """list buffers that hold the longest list of the set and not all of them: some lists on the device, some built by the host"""
    w = wants[name]
    cov, pu = zip(*(list_words(r) for r in w.side.records))
    monkeypatch.setenv("VGA_COV_LIST_WORDS", str(max(cov)))
    monkeypatch.setenv("VGA_PILEUP_LIST_WORDS", str(max(pu)))
    monkeypatch.setenv("VGA_TRACE", "1")
    capfd.readouterr()
    al = run(ctx, w, name + ", small lists")
    trace = capfd.readouterr().err
    by_host = {what: built_by_host(trace, what) for what in ("run list", "pileup list")}
    print("built by the host:", by_host, "of", al.poa_problems)
    assert 0 < by_host["run list"] < al.poa_problems
    # (the default buffer of drb5-edges is smaller than its longest pileup list: there every problem takes this route)
    assert 0 < by_host["pileup list"] < al.poa_problems + (name == "drb5-edges")


@pytest.mark.parametrize("name", ("drb1-sweep", "synth-nodes", "drb1-both-strands"))
def test_lists_all_built_by_the_host(ctx, wants, monkeypatch, capfd, name):
    """list buffers of no words at all: the host's walk builds every list of the call.  These sets hold what the DRB5 sets cannot:
    a node entered at lane 0 inside a match run, the leading insertion, I directly behind D, reverse-strand queries"""
    monkeypatch.setenv("VGA_COV_LIST_WORDS", "0")
    monkeypatch.setenv("VGA_PILEUP_LIST_WORDS", "0")
    monkeypatch.setenv("VGA_TRACE", "1")
    capfd.readouterr()
    al = run(ctx, wants[name], name + ", no room for any list")
    trace = capfd.readouterr().err
    assert al.poa_problems == len(wants[name].lines)
    assert built_by_host(trace, "run list") == al.poa_problems
    assert built_by_host(trace, "pileup list") == al.poa_problems
