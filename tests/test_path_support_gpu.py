"""Path support on the GPU (vga_path_support_begin / _read / _last / _reset / _end / _lists, k_ps_build + k_ps_score,
`vgaligner map --path-support`).  Every comparison is exact equality of integer arrays: against the reference walker
(tests/path_support_ref.py) run over the ORACLE's alignments GAF -- text the existing parity tests hold equal to the GPU's records
-- or, for the kernel seam vga_path_support_lists, against a few lines of Python over the index arrays.  Without the feature
every test here stops at Context.path_support_begin (no such call) or at the unknown --path-support flag."""
import os
import subprocess

import numpy as np
import pytest

import coverage_ref
import path_support_ref
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
def drb1(oracle):
    return oracle.Index(oracle.Graph.from_gfa(DRB1), 11)


# =====================================================================================================================
# 1. the kernel seam on hand-made graphs
# =====================================================================================================================
SPINE, LEAVES = 420, 70
HUB, JOIN = SPINE + 1, SPINE + 1 + LEAVES + 1


def write_seam_gfa(path):
    """nodes 1..420: a spine with edges i -> i+1 and i -> i+2, node lengths 1..5; node 421: a hub with 70 outgoing edges (the slot
    search of its last leaf passes 64 slots), leaves 422..491, all into node 492"""
    rng = np.random.default_rng(5)
    seq = lambda n: "".join("ACGT"[x] for x in rng.integers(0, 4, n))
    with open(path, "w") as f:
        f.write("H\tVN:Z:1.0\n")
        for i in range(1, JOIN + 1):
            f.write("S\t%d\t%s\n" % (i, seq(1 + (i * 7) % 5)))
        for i in range(1, SPINE + 1):
            f.write("L\t%d\t+\t%d\t+\t0M\n" % (i, i + 1))
            if i + 2 <= SPINE:
                f.write("L\t%d\t+\t%d\t+\t0M\n" % (i, i + 2))
        for leaf in range(HUB + 1, JOIN):
            f.write("L\t%d\t+\t%d\t+\t0M\n" % (HUB, leaf))
            f.write("L\t%d\t+\t%d\t+\t0M\n" % (leaf, JOIN))


@pytest.fixture(scope="module")
def seam(oracle, tmp_path_factory):
    gfa = str(tmp_path_factory.mktemp("psseam") / "seam.gfa")
    write_seam_gfa(gfa)
    ix = oracle.Index(oracle.Graph.from_gfa(gfa), 11)
    return ix, oracle_index_arrays(ix)


def spine_walk(rng, start, n):
    out = [start]
    while len(out) < n:
        out.append(out[-1] + int(rng.integers(1, 3)))
    assert out[-1] <= SPINE
    return out


def seam_paths(n_paths, rng):
    """n_paths paths as lists of (node, is_reverse), the special ones shuffled among random walks"""
    fwd = lambda ids: [(i, False) for i in ids]
    special = [
        fwd(list(range(1, HUB + 1)) + [JOIN - 1, JOIN]),                        # the whole spine, the hub's LAST leaf
        fwd([1]) + [(2, True)] + fwd([3, 4]),                                   # a '-' step in the middle: no pair through it
        [(i, True) for i in (9, 8, 7)],                                         # an all-'-' path
        fwd([3, 4, 3, 5]),                                                      # visits node 3 twice; 4+,3+ has no L line
        fwd([1, 5, 6]),                                                         # 1+,5+ has no L line
        fwd([SPINE - 1, SPINE, HUB, HUB + 1, JOIN]),                            # the hub's first leaf
    ]
    paths = special[:n_paths]
    while len(paths) < n_paths:
        if rng.integers(0, 4) == 0:
            paths.append(fwd(list(range(SPINE - int(rng.integers(2, 30)), HUB + 1)) + [int(rng.integers(HUB + 1, JOIN)), JOIN]))
        else:
            paths.append(fwd(spine_walk(rng, int(rng.integers(1, 200)), int(rng.integers(2, 100)))))
    return [paths[i] for i in rng.permutation(n_paths)]


def pack(paths):
    off = np.zeros(len(paths) + 1, dtype=np.uint64)
    steps = []
    for i, st in enumerate(paths):
        steps += [(n << 1) | (1 if rev else 0) for n, rev in st]
        off[i + 1] = len(steps)
    return off, np.asarray(steps, dtype=np.uint64)


def expected(arrays, paths, lists, bases):
    """the meaning of the seam in plain Python -> (bases, edges, pairs without an edge)"""
    eidx, eto, edg = arrays["node_edge_idx"], arrays["node_edges_to"], arrays["edges"]
    is_edge = lambda a, b: 2 * b in [int(x) for x in edg[eidx[a - 1] + eto[a - 1]:eidx[a]]]
    fwd = [{n for n, rev in st if not rev} for st in paths]
    steps = [[(a[0], b[0]) for a, b in zip(st, st[1:]) if not a[1] and not b[1]] for st in paths]
    missing = sum(1 for st in steps for a, b in st if not is_edge(a, b))
    pairs = [{(a, b) for a, b in st if is_edge(a, b)} for st in steps]
    wb = np.array([[sum(c for n, c in zip(l, nb) if n in fwd[p]) for p in range(len(paths))] for l, nb in zip(lists, bases)], dtype=np.int64)
    we = np.array([[sum(1 for ab in zip(l, l[1:]) if ab in pairs[p]) for p in range(len(paths))] for l in lists], dtype=np.int64)
    return wb.reshape(len(lists), len(paths)), we.reshape(len(lists), len(paths)), missing


def same_matrices(got, wb, we, what):
    for name, g, w in (("bases", got[0], wb), ("edges", got[1], we)):
        assert g.dtype == np.uint32 and g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, (what, name, len(bad), bad[:6].tolist(), [int(g[tuple(x)]) for x in bad[:6]], [int(w[tuple(x)]) for x in bad[:6]])


@pytest.mark.parametrize("n_paths", [1, 3, 31, 32, 33, 64, 65, 130])
def test_seam_word_and_wave_boundaries(ctx, seam, n_paths):
    ix, arrays = seam
    rng = np.random.default_rng(100 + n_paths)
    paths = seam_paths(n_paths, rng)
    upload_oracle_index(ctx, ix)
    missing = ctx.path_support_begin(*pack(paths))
    nlen = lambda n: arrays["node_seq_idx"][n] - arrays["node_seq_idx"][n - 1]
    lists = [[7]]                                                            # one node: no pair
    lists += [spine_walk(rng, 1 + k, n) for k, n in enumerate((63, 64, 65, 200))]
    lists += [[SPINE - 1, SPINE, HUB, leaf, JOIN] for leaf in (HUB + 1, HUB + 64, HUB + 65, JOIN - 1)]  # slots 0, 63, 64, 69 of the hub
    lists += [[3, 4, 3, 5], [1, 5, 6]]                                       # pairs of a path that have no L line: they score nothing
    lists += [[5, 3, 300, 2], [JOIN, 1]]                                     # pairs that are no graph edge at all
    lists += [[400, 402, 403]]                                               # (edges that few of the paths hold, or none)
    bases = [[int(rng.integers(0, nlen(n) + 1)) for n in l] for l in lists]
    bases[1] = [nlen(n) for n in lists[1]]                                   # fully covered: the runs of neighbouring nodes touch
    bases[2][5] = 0                                                          # a node that counts for the edges only
    bases[2][6] = 0
    wb, we, want_missing = expected(arrays, paths, lists, bases)
    assert missing == want_missing and (n_paths < 5 or missing >= 2)
    got = ctx.path_support_lists(lists, bases)
    print("n_paths", n_paths, "lists", len(lists), "bases", int(wb.sum()), "edges", int(we.sum()), "pairs without an edge", missing)
    same_matrices(got, wb, we, "n_paths %d" % n_paths)
    if n_paths >= 6:
        assert we.sum() > 0 and wb.sum() > 0 and not we[-3:-1].any()
    # the seam leaves the accumulators alone, and an empty call is fine
    acc = ctx.path_support()
    assert acc["n_alignments"] == 0 and not acc["sum_bases"].any() and not acc["top"].any()
    b0, e0 = ctx.path_support_lists([], [])
    assert b0.shape == (0, n_paths) and e0.shape == (0, n_paths)
    ctx.path_support_end()


def test_seam_refuses_bad_arguments(ctx, seam):
    p = pkg()
    ix, arrays = seam
    upload_oracle_index(ctx, ix)
    for off, steps in (([0], []), ([0, 2, 1], [2, 4]), ([0, 1], [0]), ([0, 1], [(JOIN + 1) << 1])):
        with pytest.raises(p.VgaError) as e:
            ctx.path_support_begin(off, steps)
        assert e.value.code == -1, (off, steps)
    with pytest.raises(p.VgaError) as e:
        ctx.path_support_begin(np.arange(4098), np.full(4097, 2))
    assert e.value.code == -4  # VGA_ERR_UNSUPPORTED: more than 4096 paths
    assert ctx.path_support_begin(np.arange(4097), np.full(4096, 2)) == 0
    b, e = ctx.path_support_lists([[1, 2]], [[1, 0]])
    assert b.shape == (1, 4096) and (b == 1).all() and not e.any()
    for lists, bases in (([[0]], [[0]]), ([[JOIN + 1]], [[0]]), ([[1]], [[99]])):
        with pytest.raises(p.VgaError) as e:
            ctx.path_support_lists(lists, bases)
        assert e.value.code == -1
    ctx.path_support_end()


def test_seam_config4_graph_paths_that_repeat_nodes(oracle, ctx, config4_gfa):
    p = pkg()
    ix = oracle.Index(oracle.Graph.from_gfa(config4_gfa), 11)
    arrays = oracle_index_arrays(ix)
    _, named = path_support_ref.parse_gfa(config4_gfa)
    paths = [st for _, st in named]
    assert len(paths) > 64 and any(len({n for n, _ in st}) < len(st) for st in paths)
    g = p.hostlib.gfa_paths(config4_gfa)
    upload_oracle_index(ctx, ix)
    missing = ctx.path_support_begin(g["step_off"], g["steps"])
    eidx, eto, edg = arrays["node_edge_idx"], arrays["node_edges_to"], arrays["edges"]
    idx = arrays["node_seq_idx"]
    rng = np.random.default_rng(44)
    lists = []
    while len(lists) < 40:
        l = [int(rng.integers(1, len(idx)))]
        for _ in range(int(rng.integers(1, 300))):
            out = [int(h) >> 1 for h in edg[eidx[l[-1] - 1] + eto[l[-1] - 1]:eidx[l[-1]]] if not int(h) & 1]
            if not out:
                break
            l.append(out[int(rng.integers(0, len(out)))])
        lists.append(l)
    bases = [[int(rng.integers(0, idx[n] - idx[n - 1] + 1)) for n in l] for l in lists]
    wb, we, want_missing = expected(arrays, paths, lists, bases)
    assert missing == want_missing
    print("config 4:", len(paths), "paths,", sum(len(l) for l in lists), "list nodes, bases", int(wb.sum()), "edges", int(we.sum()))
    assert we.sum() > 0
    same_matrices(ctx.path_support_lists(lists, bases), wb, we, "config 4")
    ctx.path_support_end()


# =====================================================================================================================
# 2. end to end: the accumulators and the matrices of the last call against the walker over the oracle's GAF
# =====================================================================================================================
def walker(oracle, ix, gfa, seqs, best_n=1):
    mp = oracle.default_map_params()
    mp.align_best_n = best_n
    _, ag, _ = oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)
    node_len, paths = path_support_ref.parse_gfa(gfa)
    return path_support_ref.walk(ag, node_len, paths), ag


def fresh(c, ix, gfa):
    upload_oracle_index(c, ix)
    g = pkg().hostlib.gfa_paths(gfa)
    return c.path_support_begin(g["step_off"], g["steps"])


def score(c, seqs, best_n=1, map_params=None):
    b = c.batch(seqs)
    mo = b.map(map_params) if map_params is not None else b.map()
    al = b.align(mo, best_n=best_n)
    b.close()
    return al, mo


ACC = ("sum_bases", "sum_edges", "top", "top_alone")


def same_acc(got, want, what=""):
    print(what, "alignments", got["n_alignments"], "/", want["n_alignments"], "unplaced", got["n_unplaced"], "/", want["n_unplaced"], "bases",
          int(got["sum_bases"].sum()), "/", int(want["sum_bases"].sum()), "edges", int(got["sum_edges"].sum()), "/", int(want["sum_edges"].sum()))
    assert (got["n_alignments"], got["n_unplaced"]) == (want["n_alignments"], want["n_unplaced"]), what
    for k in ACC:
        assert got[k].dtype == np.uint64 and got[k].tolist() == want[k].tolist(), (what, k, got[k].tolist(), want[k].tolist())


def same(c, want, what=""):
    same_acc(c.path_support(), want, what)
    same_matrices(c.path_support_last(), want["bases"], want["edges"], what)


def add(x, y):
    out = {k: x[k] + y[k] for k in ACC + ("n_alignments", "n_unplaced")}
    return out


@pytest.fixture(scope="module")
def drb1_case(oracle, drb1):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]
    want, ag = walker(oracle, drb1, DRB1, seqs)
    assert want["n_alignments"] == len(seqs)
    return seqs, want, ag


def test_drb1(ctx, drb1, drb1_case):
    seqs, want, _ = drb1_case
    assert fresh(ctx, drb1, DRB1) == 0
    score(ctx, seqs)
    same(ctx, want, "DRB1 k=11")
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_cov_runs" in names and "k_ps_score" in names and "k_cov_add" not in names, names
    ctx.path_support_end()


def test_test_gfa(oracle, ctx):
    ix = oracle.Index(oracle.Graph.from_gfa(TEST_GFA), 11)
    seqs = [r.seq for r in pkg().readsim.simulate_reads(TEST_GFA, 8, 60, 0, 0, 0, seed=3)]
    want, _ = walker(oracle, ix, TEST_GFA, seqs)
    fresh(ctx, ix, TEST_GFA)
    al, _ = score(ctx, seqs)
    assert want["n_alignments"] == int(al.aligned.sum()) > 0
    same(ctx, want, "test.gfa")
    ctx.path_support_end()


def test_synthetic_pangenome_narrow_bands(oracle, ctx, tmp_path, monkeypatch):
    gfa = str(tmp_path / "syn100k.gfa")
    pkg().readsim.synth_pangenome(gfa, total_bp=100000)
    ix = oracle.Index(oracle.Graph.from_gfa(gfa), 11)
    seqs = [r.seq for r in pkg().readsim.config3_reads(gfa, 12, 3000)] + [r.seq for r in pkg().readsim.config2_reads(gfa, 40)]
    want, _ = walker(oracle, ix, gfa, seqs)
    assert want["n_alignments"] > 12 and want["bases"].shape[1] == 16
    fresh(ctx, ix, gfa)
    score(ctx, seqs)
    same(ctx, want, "synthetic pangenome")
    monkeypatch.setenv("VGA_POA_KERNEL", "t6")
    ctx.path_support_reset()
    score(ctx, seqs)
    same(ctx, want, "synthetic pangenome, t6")
    ctx.path_support_end()


def test_both_strands(oracle, ctx, drb1):
    p = pkg()
    reads = p.readsim.simulate_reads(DRB1, 32, 2500, 0.03, 0.03, 0.04, seed=31, reverse_fraction=0.5)
    seqs = [r.seq for r in reads]
    mp = p.default_map_params()
    mp.strands = p.binding.VGA_STRANDS_BOTH
    fresh(ctx, drb1, DRB1)
    al, mo = score(ctx, seqs, map_params=mp)
    assert 0 < int(mo.strand.sum()) < len(seqs)
    # a '-' record carries the forward path and the cs of the reverse complement: the oracle on the orientation that was chosen
    chosen = [p.readsim.reverse_complement(s) if st else s for s, st in zip(seqs, mo.strand.tolist())]
    want, _ = walker(oracle, drb1, DRB1, chosen)
    assert want["n_alignments"] == int(al.aligned.sum()) == len(seqs)
    same(ctx, want, "both strands")
    ctx.path_support_end()


def test_best_of_n_candidates_in_different_sub_batches(oracle, ctx, drb1, monkeypatch):
    p = pkg()
    src = p.readsim.simulate_reads(DRB1, 6, 700, 0.0, 0.0, 0.0, seed=23)
    seqs = [r.seq[:500] + r.seq[:500] for r in src] + [src[0].seq[:300] * 3, src[1].seq]
    monkeypatch.setenv("VGA_POA_SUB", "2")  # (two problems per launch: a read's candidates fall into different ones)
    fresh(ctx, drb1, DRB1)
    for best_n in (1, 2, 5):
        ctx.path_support_reset()
        al, mo = score(ctx, seqs, best_n=best_n)
        assert max(len(mo.chains_of(r)) for r in range(len(seqs))) >= 2, "the test needs reads with several chains"
        if best_n > 1:
            assert al.poa_problems > len(seqs)
        same(ctx, walker(oracle, drb1, DRB1, seqs, best_n)[0], "best_n %d" % best_n)
    ctx.path_support_end()


@pytest.fixture(scope="module")
def routes_case(oracle, drb1):
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 8, 2500, 0.03, 0.03, 0.04, seed=12)]
    want, _ = walker(oracle, drb1, DRB1, seqs)
    assert want["n_alignments"] == len(seqs)
    return seqs, want


@pytest.mark.parametrize("env", [{"VGA_COV_LIST_WORDS": "0"}, {"VGA_COV_LIST_WORDS": "6000"}, {"VGA_POA_TEXT": "host"}, {"VGA_POA_KERNEL": "t6"},
                                 {"VGA_COV_LIST_WORDS": "6000", "VGA_POA_TEXT": "host"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_routes_score_the_same(ctx, drb1, routes_case, monkeypatch, env):
    """a run-list buffer too small for any problem or for some (the host builds those lists), host text, a forced DP kernel that
    hands wide problems back"""
    seqs, want = routes_case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fresh(ctx, drb1, DRB1)
    score(ctx, seqs)
    same(ctx, want, str(env))
    ctx.path_support_end()


def test_with_coverage_at_the_same_time(ctx, drb1, drb1_case):
    seqs, want, ag = drb1_case
    a = oracle_index_arrays(drb1)
    cov_want = coverage_ref.walk(ag, a["node_seq_idx"], a["node_edge_idx"], a["node_edges_to"], a["edges"])

    def same_cov(what):
        got = ctx.coverage()
        assert got[3] == cov_want[3], what
        for g, w in zip(got[:3], cov_want[:3]):
            assert np.array_equal(g, w), what

    fresh(ctx, drb1, DRB1)
    ctx.coverage_begin()
    score(ctx, seqs)
    names = [t["name"] for t in ctx.kernel_times()]
    assert "k_cov_add" in names and "k_ps_score" in names, names
    same(ctx, want, "beside coverage")
    same_cov("beside path support")
    # either ends without disturbing the other
    ctx.coverage_end()
    ctx.path_support_reset()
    score(ctx, seqs)
    same(ctx, want, "coverage ended")
    ctx.coverage_begin()
    ctx.path_support_end()
    score(ctx, seqs)
    same_cov("path support ended")
    assert not any(t["name"].startswith("k_ps") for t in ctx.kernel_times())
    ctx.coverage_end()


# =====================================================================================================================
# 3. life cycle
# =====================================================================================================================
def test_life_cycle(oracle, drb1, monkeypatch):
    p = pkg()
    s1 = [r.seq for r in p.readsim.simulate_reads(DRB1, 10, 2000, 0.03, 0.03, 0.04, seed=51)]
    s2 = [r.seq for r in p.readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w1, w2 = walker(oracle, drb1, DRB1, s1)[0], walker(oracle, drb1, DRB1, s2)[0]
    assert w2["n_alignments"] == 7 and not w2["bases"][7].any()  # (the last read has no chain: a placeholder record, a zero row)
    g = p.hostlib.gfa_paths(DRB1)
    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.path_support_begin(g["step_off"], g["steps"])
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        for call in (c.path_support, c.path_support_last, c.path_support_reset, lambda: c.path_support_lists([[1]], [[0]])):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1  # VGA_ERR_ARG: read / last / reset / lists before begin
        score(c, s1)
        assert not any(t["name"].startswith(("k_ps", "k_cov")) for t in c.kernel_times()), "off: no kernel of its own, no run lists"
        c.path_support_begin(g["step_off"], g["steps"])
        assert [t["name"] for t in c.kernel_times()] == ["k_ps_build"]
        with pytest.raises(p.VgaError) as e:
            c.path_support_last(len(s1))  # (nothing scored since begin)
        assert e.value.code == -1
        score(c, s1)
        same(c, w1, "first call")
        same(c, w1, "read twice")
        with pytest.raises(p.VgaError) as e:
            c.path_support_last(len(s1) + 1)
        assert e.value.code == -1
        score(c, s2)
        same_acc(c.path_support(), add(w1, w2), "two calls accumulate")
        same_matrices(c.path_support_last(), w2["bases"], w2["edges"], "the last call's rows, a zero row for the placeholder")
        c.path_support_reset()
        acc = c.path_support()
        assert acc["n_alignments"] == 0 and acc["n_unplaced"] == 0 and not any(acc[k].any() for k in ACC)
        score(c, s2)
        same(c, w2, "after reset")
        # VGA_SUBGRAPH=host is refused while it is on, and what it was once it is off
        monkeypatch.setenv("VGA_SUBGRAPH", "host")
        with pytest.raises(p.VgaError) as e:
            score(c, s2)
        assert e.value.code == -4 and "VGA_SUBGRAPH" in str(e.value) and "path support" in str(e.value)
        same_acc(c.path_support(), w2, "the refused call added nothing")
        monkeypatch.delenv("VGA_SUBGRAPH")
        # a new index drops the state and turns it off
        upload_oracle_index(c, drb1)
        with pytest.raises(p.VgaError) as e:
            c.path_support()
        assert e.value.code == -1
        score(c, s1)
        assert not any(t["name"].startswith(("k_ps", "k_cov")) for t in c.kernel_times())
        c.path_support_begin(g["step_off"], g["steps"])
        score(c, s1)
        same(c, w1, "on again on the new index")
        c.path_support_end()
        c.path_support_end()  # (ending twice is harmless)
        with pytest.raises(p.VgaError):
            c.path_support()
        monkeypatch.setenv("VGA_SUBGRAPH", "host")
        al, _ = score(c, s1)  # (off: the host route is what it was)
        assert int(al.aligned.sum()) > 0
    finally:
        c.close()


CHILDREN = {  # the stages that live in path support's state: how each begins, reads its table and says that it is off
    "genotype": ("genotype_begin", "genotype", "vga_genotype_read: genotyping is off (vga_genotype_begin)"),
    "likelihood": ("genotype_likelihood_begin", "genotype_likelihood", "vga_genotype_lik_read: the likelihood is off (vga_genotype_lik_begin)"),
    "edit": ("path_edit_begin", "path_edit", "vga_path_edit_read: the edit distance is off (vga_path_edit_begin)"),
}


def same_table(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def children_case(drb1):
    """six reads, and the table of path support and of each child when it alone is on"""
    p = pkg()
    seqs = [r.seq for r in p.readsim.simulate_reads(DRB1, 6, 2000, 0.03, 0.03, 0.04, seed=61)]
    alone = {}
    for name in [None] + list(CHILDREN):
        c = p.Context(0)
        try:
            fresh(c, drb1, DRB1)
            if name:
                getattr(c, CHILDREN[name][0])()
            score(c, seqs)
            alone[name or "support"] = getattr(c, CHILDREN[name][1])() if name else c.path_support()
        finally:
            c.close()
    assert alone["support"]["n_alignments"] == len(seqs) and alone["genotype"]["sum_bases"].any() and alone["likelihood"]["n_scored"] == len(seqs)
    assert alone["edit"]["n_alignments"] == len(seqs) and alone["edit"]["n_scored"].any()
    return seqs, alone


@pytest.mark.parametrize("ending", ["path_support_end", "new index", "close"])
def test_children_end_with_path_support(drb1, children_case, ending):
    """genotyping, the likelihood and the edit distance all on over one path support: each table is what the stage gives alone, and
    the three end with path support, with its index, and with the context"""
    p = pkg()
    seqs, alone = children_case
    c = p.Context(0)
    try:
        fresh(c, drb1, DRB1)
        for begin, _, _ in CHILDREN.values():
            getattr(c, begin)()
        score(c, seqs)
        names = [t["name"] for t in c.kernel_times()]
        assert all(k in names for k in ("k_ps_score", "k_gt_pairs", "k_gl_pairs", "k_pe_rows")), names
        same_table(c.path_support(), alone["support"], "path support beside its three children")
        for name, (_, read, _) in CHILDREN.items():
            same_table(getattr(c, read)(), alone[name], name + " beside the others")
        if ending == "close":
            c.close()  # (everything still on)
            return
        if ending == "path_support_end":
            c.path_support_end()
        else:
            upload_oracle_index(c, drb1)
        for name, (_, read, off) in CHILDREN.items():
            with pytest.raises(p.VgaError) as e:
                getattr(c, read)()
            assert e.value.code == -1 and off in str(e.value), (name, str(e.value))
        with pytest.raises(p.VgaError) as e:
            c.path_support()
        assert e.value.code == -1
        score(c, seqs)
        names = [t["name"] for t in c.kernel_times()]
        assert names and not any(n.startswith(("k_ps", "k_gt", "k_gl", "k_pe")) for n in names), names
    finally:
        c.close()


# =====================================================================================================================
# 4. the executable
# =====================================================================================================================
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
    node_len, paths = path_support_ref.parse_gfa(DRB1)
    w = path_support_ref.walk(oag, node_len, paths)
    assert w["n_alignments"] == len(reads)
    want_paths = "path\tsteps\tlength\tsum_bases\tsum_edges\ttop\ttop_alone\n" + "".join(
        "%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (name, len(st), sum(node_len[n] for n, rev in st if not rev), w["sum_bases"][i], w["sum_edges"][i], w["top"][i],
                                          w["top_alone"][i]) for i, (name, st) in enumerate(paths))
    want_reads = "read\tpath\tbases\tedges\n" + "".join(
        "%d\t%d\t%d\t%d\n" % (r, i, w["bases"][r, i], w["edges"][r, i]) for r in range(len(reads)) for i in range(len(paths))
        if w["bases"][r, i] or w["edges"][r, i])
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    for out, extra in (("one", ["--path-support"]), ("two", ["--path-support", "--devices", "0,0", "--chunk-reads", "10"]),
                       ("cov", ["--path-support", "--coverage"])):
        pr = run(common + ["-o", os.path.join(d, out)] + extra)
        assert "%d alignments scored, %d unplaced" % (w["n_alignments"], w["n_unplaced"]) in pr.stderr, pr.stderr
        pre = os.path.join(d, out)
        assert open(pre + "-path-support.tsv").read() == want_paths, out
        assert open(pre + "-path-support-reads.tsv").read() == want_reads, out
        assert open(pre + "-chains.gaf").read() == open(os.path.join(d, "plain-chains.gaf")).read() == ocg, out
        assert open(pre + "-alignments.gaf").read() == open(os.path.join(d, "plain-alignments.gaf")).read() == oag, out
        assert os.path.exists(pre + "-coverage-nodes.tsv") == (out == "cov")
    assert not os.path.exists(os.path.join(d, "plain-path-support.tsv")) and not os.path.exists(os.path.join(d, "plain-path-support-reads.tsv"))
