"""The insertion table and the insertion call on the GPU (vga_insertion_begin / _read / _reset / _end / _call / _call_table,
k_ia_events + k_ia_add + k_ia_call, `vgaligner map --call-variants --call-insertions`).  Every comparison is exact equality of
the uint32 table and of the three totals against the reference walker (tests/insertion_ref.py) run over the ORACLE's alignments
GAF, on every route a problem can take through poa_run, and of the calls against the reference's call rule.  Without the feature
every test here stops at Context.insertion_begin (no such call) or at the unknown --call-insertions flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import insertion_ref
import op_cases as M
import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
COLS = insertion_ref.COLS


@pytest.fixture(scope="module")
def ctx():
    c = pkg().Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def drb1_graph(oracle):
    return oracle.Graph.from_gfa(DRB1)


@pytest.fixture(scope="module")
def drb1(oracle, drb1_graph):
    return oracle.Index(drb1_graph, 11)


def oracle_gaf(oracle, ix, seqs, best_n=1):
    mp = oracle.default_map_params()
    mp.align_best_n = best_n
    return oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)[1]


def walker(oracle, ix, seqs, best_n=1):
    """(counts, n_alignments, n_events, n_leading) from the oracle's alignments GAF of seqs"""
    a = oracle_index_arrays(ix)
    return insertion_ref.walk(oracle_gaf(oracle, ix, seqs, best_n), a["node_seq_idx"], a["seq_fwd"])


def add(x, y):
    return tuple(a + b for a, b in zip(x, y))


def same(got, want, what=""):
    print(what, "alignments", got[1], "/", want[1], "insertions", got[2], "/", want[2], "leading", got[3], "/", want[3])
    assert got[1:] == want[1:], (what, "totals", got[1:], want[1:])
    g, w = got[0], want[0]
    assert g.dtype == np.uint32 and g.shape == w.shape and g.shape[1] == COLS, (what, g.shape, w.shape)
    bad = np.argwhere(g != w)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), [int(g[i, j]) for i, j in bad[:8]], [int(w[i, j]) for i, j in bad[:8]])


def count(c, seqs, best_n=1, map_params=None):
    """one map + align call on a context that is counting"""
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=best_n)
    b.close()
    return al, mo


def fresh(c, ix):
    upload_oracle_index(c, ix)
    c.insertion_begin()


# ---- 1. DRB1, beside the pileup
@pytest.mark.parametrize("k", [11, 19])
def test_drb1(oracle, ctx, drb1_graph, k):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]
    ix = oracle.Index(drb1_graph, k)
    want = walker(oracle, ix, seqs)
    assert want[1] == len(seqs) and want[2] > 1000
    fresh(ctx, ix)
    ctx.pileup_begin()  # (in the same call: the bins of a base add up to the pileup's ins there)
    count(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_ia_events" in names and "k_ia_add" in names and "k_pu_events" in names, names
    got = ctx.insertions()
    same(got, want, "DRB1 k=%d" % k)
    pu, n_pu, leading = ctx.pileup()
    assert n_pu == got[1] and leading == got[3]
    assert np.array_equal(got[0][:, :insertion_ref.BINS].sum(1, dtype=np.uint32), pu[:, pileup_ref.INS])
    insertion_ref.check_rows(got[0])
    ctx.pileup_end()
    ctx.insertion_end()


# ---- 2. block edges
RUN_LANES = (56, 57, 58, 59, 60, 61, 62, 63, 0)
RUN_LENGTHS = (7, 8, 9)


def run_letters(n, before, behind, k=0):
    """n letters that hold at least three different ones, the first none of `behind` (the graph base that follows the run) and
    the last none of `before` (the one that precedes it): the run cannot slide, and no neighbour pair of it is a homopolymer"""
    first = [c for c in "ACGT" if c != behind.upper()][k % 3]
    last = [c for c in "ACGT" if c not in (before.upper(), first)][0]
    mid = [c for c in "ACGT" if c not in (first, last)]
    body = "".join(mid[(i + k) % 2] if i % 3 else (first if i % 2 else last) for i in range(n - 2))
    run = first + body + last
    assert len(run) == n and len(set(run)) >= 3
    return run


def planted_run(e, lane, n, gap=40, k=0, edit=None):
    """an Edit (op_cases) gets a run of n different letters whose first column is on `lane`; edit(run) changes it"""
    p = e.at(lane, gap)
    e.copy_to(p)
    run = run_letters(n, e.h[p - 1], e.h[p], k)
    if edit is not None:
        run = edit(run)
    e.out.append(run)
    e.ins += n
    return run


def distinct_run_case():
    """On the one-node graph DRB5 the column of a graph base is its position plus the bases inserted before it (op_cases.Edit).
    One read per (lane, length): a run of 7, 8 or 9 different letters whose first column is on lane 56 .. 63 or on lane 0, so that
    runs of the lengths around the bin edge end before, at and behind a block edge.  Of these, the run of 8 on lane 0 holds a
    lower-case letter and the run of 9 on lane 60 has N as its eighth letter (position 7, the last that is kept).  Runs stay below
    a dozen bases: the band of a short read cannot hold longer ones.

    A run of different letters directly behind a deletion could not be planted here: wherever a deletion and an insertion meet,
    the two can change places at no cost, and the oracle then writes the insertion first; different letters also find bases of
    the deleted window to match.  behind_deletion_case has the run behind a deleted base."""
    h = M._first_path("drb5")
    reads, plan = [], []
    for i, lane in enumerate(RUN_LANES):
        for n in RUN_LENGTHS:
            e = M.Edit(h, 1000 + 331 * i + 97 * n)
            edit = None
            if (lane, n) == (0, 8):
                edit = lambda run: run[:3] + run[3].lower() + run[4:]
            if (lane, n) == (60, 9):
                edit = lambda run: run[:7] + "N" + run[8:]
            run = planted_run(e, lane, n, gap=300, k=i + n, edit=edit)
            reads.append(e.read(gap=350))
            plan.append((lane, n, run))
    return M.Case("drb5-distinct-runs", "drb5", M.K, reads, False), plan


def behind_deletion_case():
    """four of op_cases' replaced-window reads on DRB1: 36 path bases that lack a letter, replaced by 36 of that letter.  At these
    two windows the oracle writes the deletion first and the insertion directly behind it: the run belongs to a deleted base."""
    reads = M.replaced_window_reads(M._first_path("drb1"))
    n0 = M.REPLACED_WINDOWS[0][1]
    return M.Case("drb1-behind-deletion", "drb1", M.K, [reads[0], reads[1], reads[n0], reads[n0 + 1]], False)


def assert_distinct_runs_planted(gaf, plan, node_len):
    """on the oracle's GAF alone: every planted run is there, with its letters, on its lane (test_op_cases_cpu.py's method)"""
    recs = M.properties(gaf, node_len)
    assert len(recs) == len(plan) and all(r is not None for r in recs)
    seen = set()
    for rec, (lane, n, run) in zip(recs, plan):
        ins = [(f, length) for kind, f, length in M.runs(rec) if kind == "I"]
        assert len(ins) == 1 and ins[0][1] == n, (lane, n, ins)
        f = ins[0][0]
        letters = "".join(c for _, _, c in rec.cols[f:f + n])
        assert letters == run.lower(), (lane, n, letters, run)
        assert f % 64 == lane, (lane, n, f)
        assert rec.cols[f - 1][0] == "E" and rec.cols[f + n][0] == "E"
        seen.add((f % 64, n, (f + n) // 64 - f // 64))
    # the closing lane of a run that starts on lane 56 + i: in the same block (7 letters from lane 56), first of the next (8 from
    # 56, 7 from 57 ..), further into it
    for lane in RUN_LANES:
        for n in RUN_LENGTHS:
            assert (lane, n, (lane + n) // 64) in seen, (lane, n)
    assert any("n" == run[7:8].lower() for _, n, run in plan if n == 9) and any(run != run.upper() for _, _, run in plan)


@pytest.fixture(scope="module")
def edge_sets(oracle, tmp_path_factory):
    """name -> (case, oracle index, the reference's table, the oracle's GAF): the three block-edge sets of op_cases, the set of
    different letters and the runs behind a deletion"""
    tmp = tmp_path_factory.mktemp("ia_cases")
    extra, plan = distinct_run_case()
    behind = behind_deletion_case()
    out = {}
    for c in [c for c in M.all_cases(tmp) if c.name in M.BLOCK_EDGE_SETS] + [extra, behind]:
        gfa = M.gfa_path(c, tmp)
        ix = oracle.Index(oracle.Graph.from_gfa(gfa), c.k)
        gaf = M.alignments(oracle, ix, c)
        if c is extra:
            assert_distinct_runs_planted(gaf, plan, M.node_lengths(gfa))
        if c is behind:
            assert all(len(re.findall(r"-[a-z]{36}\+[a-z]{36}", ln)) == 1 for ln in gaf.splitlines()), "directly behind the deletion"
        a = oracle_index_arrays(ix)
        out[c.name] = (c, ix, insertion_ref.walk(gaf, a["node_seq_idx"], a["seq_fwd"]), gaf)
    return out


def test_the_op_case_sets_hold_what_they_are_run_for(edge_sets):
    """from the oracle's text: insertion runs of 9, 10, 64, 70, 99, 100 and 130, a leading insertion, a run that ends the
    alignment, N inside a run"""
    lengths, ends, n_inside = set(), 0, 0
    for name in M.BLOCK_EDGE_SETS:
        c, ix, want, gaf = edge_sets[name]
        for line in gaf.splitlines():
            cs = re.search(r"cs:Z:([^,\s]*)", line).group(1)
            lengths |= {len(t) - 1 for t in re.findall(r"\+[a-z]+", cs)}
            ends += bool(re.search(r"\+[a-z]+$", cs))
            n_inside += bool(re.search(r"\+[acgt]+n[acgtn]*", cs))
    assert {9, 10, 64, 70, 99, 100, 130} <= lengths, sorted(lengths)
    assert ends > 0 and n_inside > 0
    assert sum(edge_sets[name][2][3] for name in M.BLOCK_EDGE_SETS) >= 2, "leading insertions"


@pytest.mark.parametrize("name", M.BLOCK_EDGE_SETS + ("drb5-distinct-runs", "drb1-behind-deletion"))
@pytest.mark.parametrize("env", [{}, {"VGA_INS_LIST_WORDS": "0"}], ids=["lists on the device", "VGA_INS_LIST_WORDS=0"])
def test_block_edges(ctx, edge_sets, monkeypatch, capfd, name, env):
    """an insertion list is two words per run: with the default buffer every list is k_ia_events' own, with no buffer the host's"""
    c, ix, want, gaf = edge_sets[name]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, ix)
    capfd.readouterr()
    al, _ = count(ctx, c.reads)
    by_host = len(re.findall(r"no room for its insertion list", capfd.readouterr().err))
    # (a record without an insertion behind a base has a list of no words: it finds room in a buffer of no words unless a claim
    # that failed before it has moved the cursor, which depends on the order the waves run in)
    with_events = sum(bool(re.search(r"[0-9a-z]\+[a-z]", re.search(r"cs:Z:([^,\s]*)", ln).group(1))) for ln in gaf.splitlines())
    assert 0 < with_events <= al.poa_problems == len(c.reads)
    if env:
        assert with_events <= by_host <= al.poa_problems, (by_host, with_events, al.poa_problems)
    else:
        assert by_host == 0, by_host
    assert int(al.aligned.sum()) == len(c.reads) == want[1]
    got = ctx.insertions()
    same(got, want, name + str(env))
    # and the call at every base that holds an insertion, against the reference's rule on the reference's rows
    pos = np.flatnonzero(want[0][:, :insertion_ref.BINS].sum(1))
    assert len(pos) > 0
    assert insertion_ref.same(ctx.insertion_call(pos), insertion_ref.call_rows(want[0][pos])) is None
    ctx.insertion_end()


# ---- 3. the routes
@pytest.fixture(scope="module")
def routes(oracle, drb1):
    """the read set of test_routes_count_the_same and its table, computed once"""
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 8, 2500, 0.03, 0.03, 0.04, seed=12)]
    want = walker(oracle, drb1, seqs)
    assert want[1] == len(seqs)
    return seqs, want


@pytest.mark.parametrize("env", [{}, {"VGA_INS_LIST_WORDS": "0"}, {"VGA_INS_LIST_WORDS": "400"}, {"VGA_POA_KERNEL": "t6"}, {"VGA_POA_KERNEL": "t7"},
                                 {"VGA_POA_TEXT": "host"}, {"VGA_INS_LIST_WORDS": "400", "VGA_POA_TEXT": "host"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()) or "defaults")
def test_routes_count_the_same(ctx, drb1, routes, monkeypatch, capfd, env):
    """forced DP kernels (t6 hands wide problems back: a problem that runs twice replaces its record), text on the host, and a
    list buffer too small for all problems or for any: the host builds the lists that found no room.  The library's trace says
    which route a problem took."""
    seqs, want = routes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, drb1)
    capfd.readouterr()
    al, _ = count(ctx, seqs)
    trace = capfd.readouterr().err
    same(ctx.insertions(), want, str(env))
    ctx.insertion_end()
    by_host = len(re.findall(r"no room for its insertion list", trace))
    print("problems", al.poa_problems, "lists built by the host", by_host)
    words = env.get("VGA_INS_LIST_WORDS")
    if words == "0":
        assert by_host == al.poa_problems == len(seqs)
    elif words is not None:
        assert 0 < by_host < al.poa_problems, "some lists on the device, some built by the host"
    else:
        assert by_host == 0


def test_best_of_two_candidates(oracle, ctx, drb1, monkeypatch):
    """only the reported record of a read counts"""
    src = pkg().readsim.simulate_reads(DRB1, 6, 700, 0.02, 0.02, 0.02, seed=23)
    seqs = [r.seq[:500] + r.seq[:500] for r in src] + [src[0].seq[:300] * 3, src[1].seq]
    monkeypatch.setenv("VGA_POA_SUB", "2")  # (two problems per launch: a read's candidates fall into different ones)
    fresh(ctx, drb1)
    al, mo = count(ctx, seqs, best_n=2)
    assert max(len(mo.chains_of(r)) for r in range(len(seqs))) >= 2 and al.poa_problems > len(seqs)
    same(ctx.insertions(), walker(oracle, drb1, seqs, 2), "best_n 2")
    ctx.insertion_end()


@pytest.mark.parametrize("list_words", [None, "0"], ids=["lists on the device", "VGA_INS_LIST_WORDS=0"])
def test_both_strands_with_a_planted_insertion(oracle, ctx, drb1, monkeypatch, list_words):
    """reads given as reverse complements, one of them with four letters planted: a '-' record carries the forward path and the
    cs of the reverse complement, so the letters come out on the graph's forward strand"""
    p = pkg()
    rs = p.readsim
    if list_words is not None:
        monkeypatch.setenv("VGA_INS_LIST_WORDS", list_words)
    segs, paths = rs.parse_gfa_paths(DRB1)
    hap = rs.path_sequence(segs, paths[0][1])
    at = 3000
    run = run_letters(4, hap[at - 1], hap[at])
    forward = [hap[2400:at] + run + hap[at:3700]] + [r.seq for r in rs.simulate_reads(DRB1, 7, 1200, 0.02, 0.02, 0.02, seed=33)]
    seqs = [rs.reverse_complement(s) if i % 2 == 0 else s for i, s in enumerate(forward)]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    fresh(ctx, drb1)
    al, mo = count(ctx, seqs, map_params=mp)
    assert mo.strand.tolist()[0] == 1 and 0 < int(mo.strand.sum()) < len(seqs)
    chosen = [rs.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    a = oracle_index_arrays(drb1)
    gaf = oracle_gaf(oracle, drb1, chosen)
    assert "+" + run.lower() in gaf.splitlines()[0], "the planted run, as the oracle writes it for the forward read"
    want = insertion_ref.walk(gaf, a["node_seq_idx"], a["seq_fwd"])
    assert want[1] == int(al.aligned.sum()) == len(seqs)
    got = ctx.insertions()
    same(got, want, "both strands")
    hit = [i for i in np.flatnonzero(got[0][:, 3]) if insertion_ref.call_row(got[0][i])[2] == run]
    assert len(hit) == 1, "length 4 and the planted letters, forward, at one base"
    ctx.insertion_end()


# ---- 4. life cycle
def test_life_cycle(oracle, drb1_graph, drb1, monkeypatch):
    p = pkg()
    s1 = [r.seq for r in p.readsim.simulate_reads(DRB1, 10, 2000, 0.03, 0.03, 0.04, seed=51)]
    s2 = [r.seq for r in p.readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w1, w2 = walker(oracle, drb1, s1), walker(oracle, drb1, s2)
    assert w2[1] == 7  # (the last read has no chain: a placeholder record adds nothing)
    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.insertion_begin()
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        for call in (c.insertions, c.insertion_reset, lambda: c.insertion_call([0])):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1  # VGA_ERR_ARG: read / reset / call before begin
        count(c, s1)
        assert not any(t["name"].startswith("k_ia") for t in c.kernel_times()), "counting off: no insertion kernel"
        c.insertion_begin()
        count(c, s1)
        same(c.insertions(), w1, "first call")
        same(c.insertions(), w1, "read twice")
        count(c, s2)
        same(c.insertions(), add(w1, w2), "two calls add up")
        c.insertion_reset()
        counts, n, ev, leading = c.insertions()
        assert (n, ev, leading) == (0, 0, 0) and not counts.any()
        count(c, s2)
        same(c.insertions(), w2, "after reset")
        # subgraphs on the host are refused while counting
        monkeypatch.setenv("VGA_SUBGRAPH", "host")
        with pytest.raises(p.VgaError) as e:
            count(c, s2)
        assert e.value.code == -4 and "VGA_SUBGRAPH" in str(e.value)
        monkeypatch.delenv("VGA_SUBGRAPH")
        same(c.insertions(), w2, "a refused call adds nothing")
        # a new index drops the counters and turns counting off
        upload_oracle_index(c, oracle.Index(drb1_graph, 19))
        with pytest.raises(p.VgaError) as e:
            c.insertions()
        assert e.value.code == -1
        count(c, s1)
        assert not any(t["name"].startswith("k_ia") for t in c.kernel_times())
        c.insertion_end()
        c.insertion_end()  # (ending twice is harmless)
    finally:
        c.close()


def _tables(c, which):
    """the tables of the makers named in `which`, each flattened to a tuple of arrays and totals"""
    read = {"cov": c.coverage, "pu": c.pileup, "ia": c.insertions}
    return {m: read[m]() for m in which}


def _same_tables(got, want, what):
    for m, w in want.items():
        assert len(got[m]) == len(w), (what, m)
        for k, (g, x) in enumerate(zip(got[m], w)):
            assert np.array_equal(g, x), (what, m, k)


def test_three_makers_on_one_context(drb1, monkeypatch, capfd):
    """coverage, the pileup and the insertion table counting together: each table equals the one the same reads give with that
    maker alone -- with every list on the device, with one maker on the host walk between two that are not, and with all three on
    it.  Ending them in another order than they began (one of them twice) leaves the others counting, and no kernel of an ended
    maker runs."""
    p = pkg()
    seqs = [r.seq for r in p.readsim.simulate_reads(DRB1, 8, 1800, 0.03, 0.03, 0.04, seed=81)]
    begin = {"cov": lambda c: c.coverage_begin(), "pu": lambda c: c.pileup_begin(), "ia": lambda c: c.insertion_begin()}
    end = {"cov": lambda c: c.coverage_end(), "pu": lambda c: c.pileup_end(), "ia": lambda c: c.insertion_end()}
    reset = {"cov": lambda c: c.coverage_reset(), "pu": lambda c: c.pileup_reset(), "ia": lambda c: c.insertion_reset()}
    prefix = {"cov": "k_cov", "pu": "k_pu", "ia": "k_ia"}
    list_name = {"cov": "run list", "pu": "pileup list", "ia": "insertion list"}
    c = p.Context(0)
    try:
        upload_oracle_index(c, drb1)
        alone = {}
        for m in ("cov", "pu", "ia"):
            begin[m](c)
            al, _ = count(c, seqs)
            assert int(al.aligned.sum()) == len(seqs) == al.poa_problems   # (one list per read and maker)
            alone.update(_tables(c, [m]))
            end[m](c)
        assert alone["cov"][3] == alone["pu"][1] == alone["ia"][1] == len(seqs) and alone["ia"][2] > 100
        for m in ("cov", "pu", "ia"):
            begin[m](c)
        monkeypatch.setenv("VGA_TRACE", "1")
        for env, on_host in (({}, ()), ({"VGA_PILEUP_LIST_WORDS": "0"}, ("pu",)),
                             ({"VGA_COV_LIST_WORDS": "0", "VGA_PILEUP_LIST_WORDS": "0", "VGA_INS_LIST_WORDS": "0"}, ("cov", "pu", "ia"))):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            capfd.readouterr()
            count(c, seqs)
            trace = capfd.readouterr().err
            names = [t["name"] for t in c.kernel_times()]
            _same_tables(_tables(c, alone), alone, str(env))
            for m in alone:
                by_host = len(re.findall("no room for its " + list_name[m], trace))
                assert by_host == (len(seqs) if m in on_host else 0), (env, m, by_host)
            adds = [names.index(k) for k in ("k_cov_add", "k_pu_add", "k_ia_add")]
            assert adds == sorted(adds), names   # the order of the launches
            for k in env:
                monkeypatch.delenv(k)
            for m in alone:
                reset[m](c)
        monkeypatch.delenv("VGA_TRACE")
        # begun as coverage, pileup, insertions: the pileup ends first (twice), then the insertions, then coverage
        left = ["cov", "pu", "ia"]
        for gone in ("pu", "ia", "cov"):
            end[gone](c)
            if gone == "pu":
                end[gone](c)
            left.remove(gone)
            count(c, seqs)
            names = [t["name"] for t in c.kernel_times()]
            for m in alone:
                assert any(n.startswith(prefix[m]) for n in names) == (m in left), (gone, names)
            _same_tables(_tables(c, left), {m: alone[m] for m in left}, "after the end of " + gone)
            for m in left:
                reset[m](c)
    finally:
        c.close()


def test_a_table_call_that_launches_nothing_reports_no_kernel(drb1):
    """the calls over a table, without sites and without bases: kernel_times() holds the kernels of the last call, so none -- not
    those of the call that launched before it"""
    p = pkg()
    rows = random_rows(3, seed=9)
    c = p.Context(0)
    try:
        upload_oracle_index(c, drb1)
        c.pileup_begin()
        c.insertion_begin()
        quiet = [lambda: c.insertion_call([]), lambda: c.insertion_call_table(np.zeros((0, COLS), dtype=np.uint64)),
                 lambda: c.variant_call_table(np.zeros((0, 7), dtype=np.uint64), "")]
        for k, call in enumerate(quiet):
            c.insertion_call_table(rows)   # three rows: it launches
            assert "k_ia_call" in [t["name"] for t in c.kernel_times()]
            call()
            assert not [t["name"] for t in c.kernel_times() if t["name"].startswith("k_")], (k, c.kernel_times())
    finally:
        c.close()


# ---- 5. the seam
def random_rows(n, seed):
    """rows with ties, zeros, rows that `more` dominates, and counters of 2^32 - 1 and just below 2^40"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, 4, size=(n, COLS)).astype(np.uint64)              # small values: ties everywhere
    rows[::7] = rng.integers(0, 1000, size=(len(rows[::7]), COLS))
    rows[::11] = 0                                                            # nothing inserted
    rows[3::13, 8] = 5000                                                     # more wins
    rows[5::17, 8] = rows[5::17, :8].max(1)                                   # more ties with the best bin: the shorter wins
    rows[2::19] = rng.choice(np.array([0, 2**32 - 1, 2**32, 2**40 - 1], dtype=np.uint64), size=(len(rows[2::19]), COLS))
    rows[4::23, :9] = 0                                                       # letters and no bin
    return rows


def test_seam_matches_the_reference(ctx):
    rows = random_rows(2000, seed=5)
    want = insertion_ref.call_rows(rows)
    assert 0 < (want["length"] == 0).sum() < len(rows) and (want["length"] == 9).any() and (want["length_reads"] >= 2**32).any()
    got = ctx.insertion_call_table(rows)
    bad = insertion_ref.same(got, want)
    assert bad is None, (bad, np.asarray(got[bad]).tolist()[:4], np.asarray(want[bad]).tolist()[:4])
    assert "k_ia_call" in [t["name"] for t in ctx.kernel_times()]
    for n in (1, 255, 256, 257):
        assert insertion_ref.same(ctx.insertion_call_table(rows[:n]), insertion_ref.call_rows(rows[:n])) is None, n


def test_seam_limits(ctx):
    p = pkg()
    none = ctx.insertion_call_table(np.zeros((0, COLS), dtype=np.uint64))
    assert len(none["length"]) == 0 and none["rows"].shape == (0, COLS)
    for col in (0, 8, 9, COLS - 1):
        rows = np.ones((300, COLS), dtype=np.uint64)
        rows[299, col] = 2**40
        with pytest.raises(p.VgaError) as e:
            ctx.insertion_call_table(rows)
        assert e.value.code == -4, col  # VGA_ERR_UNSUPPORTED
        rows[299, col] = 2**40 - 1
        assert insertion_ref.same(ctx.insertion_call_table(rows), insertion_ref.call_rows(rows)) is None


def test_call_from_the_context_equals_the_seam(oracle, ctx, drb1):
    p = pkg()
    seqs = [r.seq for r in p.readsim.simulate_reads(DRB1, 12, 2000, 0.03, 0.03, 0.04, seed=71)]
    fresh(ctx, drb1)
    count(ctx, seqs)
    counts = ctx.insertions()[0]
    with_ins = np.flatnonzero(counts[:, :9].sum(1))
    pos = np.concatenate([with_ins[::-1], np.arange(0, 700), [len(counts) - 1, with_ins[0], with_ins[0]]]).astype(np.uint32)  # any order, repeats
    got = ctx.insertion_call(pos)
    assert insertion_ref.same(got, ctx.insertion_call_table(counts[pos])) is None
    assert insertion_ref.same(got, insertion_ref.call_rows(counts[pos])) is None
    assert np.array_equal(ctx.insertions()[0], counts), "the call does not reset or change the counters"
    assert len(ctx.insertion_call([])["length"]) == 0
    for bad in ([len(counts)], [0, 2**32 - 1]):
        with pytest.raises(p.VgaError) as e:
            ctx.insertion_call(bad)
        assert e.value.code == -1  # VGA_ERR_ARG
    ctx.insertion_end()


# ---- 6. the executable
def test_cli(oracle, drb1, tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.simulate_reads(DRB1, 300, 400, 0.02, 0.01, 0.01, seed=61)
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for r in reads:
            f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    a = oracle_index_arrays(drb1)
    _, oag, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    want, sites, n_long = insertion_ref.tsv_gaf(oag, a["node_seq_idx"], a["seq_fwd"])
    assert sites > 0
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain"), "--call-variants"])
    assert not os.path.exists(os.path.join(d, "plain-insertions.tsv"))
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("plain-alignments.gaf") == oag
    for out, extra in (("one", []), ("two", ["--devices", "0,0", "--chunk-reads", "7"])):
        pr = run(common + ["-o", os.path.join(d, out), "--call-variants", "--call-insertions"] + extra)
        assert read(out + "-insertions.tsv") == want, out
        assert "call-insertions: %d sites, %d longer than 8" % (sites, n_long) in pr.stderr, pr.stderr
        # every other file is byte for byte what it is without the switch
        files = {f[len(out):] for f in os.listdir(d) if f.startswith(out + "-")}
        assert files == {f[len("plain"):] for f in os.listdir(d) if f.startswith("plain-")} | {"-insertions.tsv"}
        for suffix in files - {"-insertions.tsv"}:
            assert read(out + suffix) == read("plain" + suffix), (out, suffix)
    pr = subprocess.run([EXE] + common + ["-o", os.path.join(d, "bad"), "--call-insertions"], cwd=d, capture_output=True, text=True, timeout=300)
    assert pr.returncode != 0 and "--call-variants" in pr.stderr and not [f for f in os.listdir(d) if f.startswith("bad")]
