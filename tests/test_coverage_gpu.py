"""Read coverage on the GPU (vga_coverage_begin / _read / _reset / _end, k_cov_runs + k_cov_add, `vgaligner map --coverage`).
Every comparison is exact equality of integer arrays against the reference walker (tests/coverage_ref.py) run over the ORACLE's
alignments GAF -- text the existing parity tests hold equal to the GPU's records -- on every route a problem can take through
poa_run.  Without the feature every test here stops at Context.coverage_begin (no such call) or at the unknown --coverage flag."""
import os
import subprocess

import numpy as np
import pytest

import coverage_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")


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


def walker(oracle, ix, seqs, best_n=1):
    """the four tables from the oracle's alignments GAF of seqs"""
    mp = oracle.default_map_params()
    mp.align_best_n = best_n
    _, ag, _ = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)
    a = oracle_index_arrays(ix)
    return coverage_ref.walk(ag, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])


def add(x, y):
    return x[0] + y[0], x[1] + y[1], x[2] + y[2], x[3] + y[3]


def same(got, want, what=""):
    print(what, "alignments", got[3], "/", want[3], "covered bases", int(got[0].sum()), "/", int(want[0].sum()), "node visits", int(got[1].sum()),
          "/", int(want[1].sum()), "edge visits", int(got[2].sum()), "/", int(want[2].sum()))
    assert got[3] == want[3], (what, "n_alignments")
    for name, g, w in zip(("base_depth", "node_reads", "edge_reads"), got, want):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:8].tolist(), g[bad[:8]].tolist(), w[bad[:8]].tolist())


def count(c, seqs, best_n=1, map_params=None):
    """one map + align call on a context that is counting"""
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=best_n)
    b.close()
    return al, mo


def fresh(c, ix):
    upload_oracle_index(c, ix)
    c.coverage_begin()


# ---- 1. the tables on four graphs, and under a forced kernel
@pytest.mark.parametrize("k", [11, 19])
def test_drb1(oracle, ctx, drb1_graph, k):
    ix = oracle.Index(drb1_graph, k)
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]
    want = walker(oracle, ix, seqs)
    assert want[3] == len(seqs)
    fresh(ctx, ix)
    count(ctx, seqs)
    same(ctx.coverage(), want, "DRB1 k=%d" % k)
    ctx.coverage_end()


def test_test_gfa(oracle, ctx):
    ix = oracle.Index(oracle.Graph.from_gfa(TEST_GFA), 11)
    seqs = [r.seq for r in pkg().readsim.simulate_reads(TEST_GFA, 8, 60, 0, 0, 0, seed=3)]
    want = walker(oracle, ix, seqs)
    fresh(ctx, ix)
    al, _ = count(ctx, seqs)
    assert want[3] == int(al.aligned.sum())
    same(ctx.coverage(), want, "test.gfa")
    ctx.coverage_end()


def test_synthetic_pangenome_narrow_bands(oracle, ctx, tmp_path):
    gfa = str(tmp_path / "syn100k.gfa")
    pkg().readsim.synth_pangenome(gfa, total_bp=100000)
    ix = oracle.Index(oracle.Graph.from_gfa(gfa), 11)
    seqs = [r.seq for r in pkg().readsim.config3_reads(gfa, 12, 3000)] + [r.seq for r in pkg().readsim.config2_reads(gfa, 40)]
    want = walker(oracle, ix, seqs)
    assert want[3] > 12
    fresh(ctx, ix)
    count(ctx, seqs)
    same(ctx.coverage(), want, "synthetic pangenome")
    ctx.coverage_end()


def test_one_long_problem_t7(oracle, ctx, drb1, monkeypatch):
    monkeypatch.setenv("VGA_POA_KERNEL", "t7")
    seqs = [r.seq for r in pkg().readsim.config3_reads(DRB1, 1)]
    want = walker(oracle, drb1, seqs)
    assert want[3] == 1
    fresh(ctx, drb1)
    count(ctx, seqs)
    same(ctx.coverage(), want, "t7")
    ctx.coverage_end()


# ---- 2. both strands
def test_both_strands(oracle, ctx, drb1):
    p = pkg()
    reads = p.readsim.simulate_reads(DRB1, 32, 2500, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5)
    seqs = [r.seq for r in reads]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    fresh(ctx, drb1)
    al, mo = count(ctx, seqs, map_params=mp)
    assert 0 < int(mo.strand.sum()) < len(seqs)
    # a '-' record carries the forward path and the cs of the reverse complement: the oracle on the orientation that was chosen
    chosen = [p.readsim.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    want = walker(oracle, drb1, chosen)
    assert want[3] == int(al.aligned.sum()) == len(seqs)
    same(ctx.coverage(), want, "both strands")
    ctx.coverage_end()


# ---- 3. only the reported record of a read counts
def test_best_of_n_candidates_in_different_sub_batches(oracle, ctx, drb1, monkeypatch):
    p = pkg()
    src = p.readsim.simulate_reads(DRB1, 6, 700, 0.0, 0.0, 0.0, seed=23)
    seqs = [r.seq[:500] + r.seq[:500] for r in src] + [src[0].seq[:300] * 3, src[1].seq]
    monkeypatch.setenv("VGA_POA_SUB", "2")  # (two problems per launch: a read's candidates fall into different ones)
    fresh(ctx, drb1)
    for best_n in (1, 2, 5):
        ctx.coverage_reset()
        al, mo = count(ctx, seqs, best_n=best_n)
        assert max(len(mo.chains_of(r)) for r in range(len(seqs))) >= 2, "the test needs reads with several chains"
        if best_n > 1:
            assert al.poa_problems > len(seqs)
        same(ctx.coverage(), walker(oracle, drb1, seqs, best_n), "best_n %d" % best_n)
    ctx.coverage_end()


# ---- 4. problems that are handed back, and the routes around the defaults
def test_pool_that_starts_far_too_small(oracle, drb1, monkeypatch):
    monkeypatch.setenv("VGA_POOL_FILL", "0.002")
    monkeypatch.setenv("VGA_POOL_SEG", str(32 << 20))
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 320, 2500, 0.03, 0.03, 0.04, seed=41)]
    c = pkg().Context(0)
    try:
        fresh(c, drb1)
        count(c, seqs)
        same(c.coverage(), walker(oracle, drb1, seqs), "starved pool")
    finally:
        c.close()


@pytest.mark.parametrize("env", [{"VGA_POA_ARENAS": "0"}, {"VGA_POA_ARENAS": "0", "VGA_POOL_BYTES": "300000000", "VGA_POA_SUB": "2"},
                                 {"VGA_POA_TEXT": "host"}, {"VGA_POA_TB": "wave"}, {"VGA_POA_KERNEL": "t6"}, {"VGA_POA_KERNEL": "t4"},
                                 {"VGA_POA_SUB": "3", "VGA_POA_SLOTS": "1"}, {"VGA_SG_SPLIT": "2", "VGA_POA_SUB": "2"},
                                 {"VGA_COV_LIST_WORDS": "6000"}, {"VGA_COV_LIST_WORDS": "0"}, {"VGA_COV_LIST_WORDS": "6000", "VGA_POA_TEXT": "host"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_routes_count_the_same(oracle, ctx, drb1, monkeypatch, env):
    """classic pool, re-queued sub-batches, host text, a traceback kernel of its own, forced DP kernels (t6 hands wide problems
    back: POA_ST_RETRY), tiny sub-batches, the store in two parts -- and a run-list buffer too small for all (VGA_COV_LIST_WORDS:
    the host builds the lists of the problems that found no room) or for any"""
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 8, 2500, 0.03, 0.03, 0.04, seed=12)]
    want = walker(oracle, drb1, seqs)
    assert want[3] == len(seqs)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fresh(ctx, drb1)
    count(ctx, seqs)
    same(ctx.coverage(), want, str(env))
    ctx.coverage_end()


def test_subgraphs_on_the_host_are_refused_while_counting(ctx, drb1, monkeypatch):
    p = pkg()
    seqs = [r.seq for r in p.readsim.config2_reads(DRB1, 8)]
    fresh(ctx, drb1)
    monkeypatch.setenv("VGA_SUBGRAPH", "host")
    with pytest.raises(p.VgaError) as e:
        count(ctx, seqs)
    assert e.value.code == -4 and "VGA_SUBGRAPH" in str(e.value)
    base, node, edge, n = ctx.coverage()
    assert n == 0 and not base.any() and not node.any() and not edge.any()
    ctx.coverage_end()
    al, _ = count(ctx, seqs)  # (counting off: the host route is what it was)
    assert int(al.aligned.sum()) > 0


# ---- 5. life cycle
def test_life_cycle(oracle, drb1_graph, drb1):
    p = pkg()
    s1 = [r.seq for r in p.readsim.simulate_reads(DRB1, 10, 2000, 0.03, 0.03, 0.04, seed=51)]
    s2 = [r.seq for r in p.readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w1, w2 = walker(oracle, drb1, s1), walker(oracle, drb1, s2)
    assert w2[3] == 7  # (the last read has no chain: a placeholder record adds nothing)
    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.coverage_begin()
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        for call in (c.coverage, c.coverage_reset):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1  # VGA_ERR_ARG: read / reset before begin
        count(c, s1)
        assert not any(t["name"].startswith("k_cov") for t in c.kernel_times()), "counting off: no coverage kernel"
        c.coverage_begin()
        count(c, s1)
        names = [t["name"] for t in c.kernel_times()]
        assert "k_cov_runs" in names and "k_cov_add" in names, names
        same(c.coverage(), w1, "first call")
        same(c.coverage(), w1, "read twice")
        count(c, s2)
        same(c.coverage(), add(w1, w2), "two calls accumulate")
        c.coverage_reset()
        base, node, edge, n = c.coverage()
        assert n == 0 and not base.any() and not node.any() and not edge.any()
        count(c, s2)
        same(c.coverage(), w2, "after reset")
        # a new index drops the counters and turns counting off
        ix19 = oracle.Index(drb1_graph, 19)
        upload_oracle_index(c, ix19)
        with pytest.raises(p.VgaError) as e:
            c.coverage()
        assert e.value.code == -1
        count(c, s1)
        assert not any(t["name"].startswith("k_cov") for t in c.kernel_times())
        c.coverage_begin()
        count(c, s1)
        same(c.coverage(), walker(oracle, ix19, s1), "counting again on the new index")
        c.coverage_end()
        c.coverage_end()  # (ending twice is harmless)
        with pytest.raises(p.VgaError):
            c.coverage()
    finally:
        c.close()


# ---- 6. the executable
def _tsv(path, header):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == header, (path, lines[0])
    return np.array([[int(x) for x in ln.split("\t")] for ln in lines[1:]], dtype=np.int64).reshape(-1, len(header))


def test_cli(oracle, drb1, tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.config3_reads(DRB1, 32, 3000)
    fa = os.path.join(d, "r.fa")
    with open(fa, "w") as f:
        for r in reads:
            f.write(">%s\n%s\n" % (r.name, r.seq))

    def run(args):
        pr = subprocess.run([EXE] + args, cwd=d, capture_output=True, text=True, timeout=900)
        assert pr.returncode == 0, pr.stderr
        return pr

    run(["index", "-i", DRB1, "-k", "11", "-o", os.path.join(d, "drb1")])
    ocg, oag, _ = oracle.map_reads(drb1, [r.name for r in reads], [r.seq for r in reads])
    a = oracle_index_arrays(drb1)
    idx, eidx, eto, edges = a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"]
    base, node, edge, n_al = coverage_ref.walk(oag, idx, eidx, eto, edges)
    assert n_al == len(reads)
    n_nodes = len(idx) - 1
    # the walker's tables in the layout of the three files
    want_nodes = np.array([[i + 1, idx[i + 1] - idx[i], node[i], base[idx[i]:idx[i + 1]].sum()] for i in range(n_nodes)], dtype=np.int64)
    want_bases = np.array([[i + 1, o, base[idx[i] + o]] for i in range(n_nodes) for o in range(idx[i + 1] - idx[i])], dtype=np.int64)
    want_edges = np.array([[i + 1, edges[s] >> 1, edge[s]] for i in range(n_nodes) for s in range(eidx[i] + eto[i], eidx[i + 1])], dtype=np.int64)
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    for out, extra in (("one", ["--coverage"]), ("two", ["--coverage", "--devices", "0,0", "--chunk-reads", "10"]), ("only", ["--coverage-only"])):
        pr = run(common + ["-o", os.path.join(d, out)] + extra)
        assert "%d alignments counted" % n_al in pr.stderr, pr.stderr
        pre = os.path.join(d, out)
        assert np.array_equal(_tsv(pre + "-coverage-nodes.tsv", ["node", "length", "reads", "bases"]), want_nodes), out
        assert np.array_equal(_tsv(pre + "-coverage-bases.tsv", ["node", "offset", "depth"]), want_bases), out
        assert np.array_equal(_tsv(pre + "-coverage-edges.tsv", ["from", "to", "reads"]), want_edges), out
        assert open(pre + "-chains.gaf").read() == open(os.path.join(d, "plain-chains.gaf")).read() == ocg, out
        if out == "only":
            assert not os.path.exists(pre + "-alignments.gaf")
        else:
            assert open(pre + "-alignments.gaf").read() == open(os.path.join(d, "plain-alignments.gaf")).read() == oag, out
    assert not os.path.exists(os.path.join(d, "plain-coverage-nodes.tsv"))
