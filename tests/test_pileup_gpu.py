"""The pileup on the GPU (vga_pileup_begin / _read / _reset / _end, k_pu_events + k_pu_add + k_pu_finish, `vgaligner map
--pileup`).  Every comparison is exact equality of the integer table and of both totals against the reference walker
(tests/pileup_ref.py) run over the ORACLE's alignments GAF -- text the existing parity tests hold equal to the GPU's records --
on every route a problem can take through poa_run.  Without the feature every test here stops at Context.pileup_begin (no such
call) or at the unknown --pileup flag."""
import os
import re
import subprocess

import numpy as np
import pytest

import pileup_ref
from helpers import DATA, ROOT, oracle_index_arrays, pkg, upload_oracle_index

pytestmark = pytest.mark.gpu

DRB1 = os.path.join(DATA, "DRB1-3123.gfa")
TEST_GFA = os.path.join(DATA, "test.gfa")
EXE = os.path.join(ROOT, "rs-vgaligner_amd", "vgaligner")
A, C, G, T, N, DEL, INS = range(7)


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


@pytest.fixture(scope="module")
def seqs24():
    return [r.seq for r in pkg().readsim.simulate_reads(DRB1, 24, 3000, 0.03, 0.03, 0.04, seed=7)]


@pytest.fixture(scope="module")
def routes(oracle, drb1):
    """the read set of test_routes_count_the_same and its table, computed once"""
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 8, 2500, 0.03, 0.03, 0.04, seed=12)]
    want = walker(oracle, drb1, seqs)
    assert want[1] == len(seqs)
    return seqs, want


def oracle_gaf(oracle, ix, seqs, best_n=1):
    mp = oracle.default_map_params()
    mp.align_best_n = best_n
    return oracle.map_reads(ix, ["r%d" % i for i in range(len(seqs))], seqs, mp)[1]


def walker(oracle, ix, seqs, best_n=1):
    """(counts, n_alignments, leading_ins) from the oracle's alignments GAF of seqs"""
    a = oracle_index_arrays(ix)
    return pileup_ref.walk(oracle_gaf(oracle, ix, seqs, best_n), a["node_seq_idx"], a["seq_fwd"])


def add(x, y):
    return x[0] + y[0], x[1] + y[1], x[2] + y[2]


def same(got, want, what=""):
    print(what, "alignments", got[1], "/", want[1], "leading insertions", got[2], "/", want[2], "column sums", got[0].sum(0).tolist(), "/",
          want[0].sum(0).tolist())
    assert got[1] == want[1], (what, "n_alignments")
    assert got[2] == want[2], (what, "leading_ins")
    g, w = got[0], want[0]
    assert g.dtype == np.uint32 and g.shape == w.shape and g.shape[1] == 7, (what, g.shape, w.shape)
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
    c.pileup_begin()


# ---- 1. the table on four graphs, and under a forced kernel
@pytest.mark.parametrize("k", [11, 19])
def test_drb1(oracle, ctx, drb1_graph, seqs24, k):
    ix = oracle.Index(drb1_graph, k)
    want = walker(oracle, ix, seqs24)
    assert want[1] == len(seqs24)
    fresh(ctx, ix)
    ctx.coverage_begin()  # (in the same call: A + C + G + T + N is the depth)
    count(ctx, seqs24)
    got = ctx.pileup()
    same(got, want, "DRB1 k=%d" % k)
    base, _, _, n_cov = ctx.coverage()
    assert n_cov == got[1] and np.array_equal(got[0][:, :5].sum(1, dtype=np.uint32), base)
    ctx.coverage_end()
    ctx.pileup_end()


def test_test_gfa(oracle, ctx):
    ix = oracle.Index(oracle.Graph.from_gfa(TEST_GFA), 11)
    seqs = [r.seq for r in pkg().readsim.simulate_reads(TEST_GFA, 8, 60, 0, 0, 0, seed=3)]
    want = walker(oracle, ix, seqs)
    fresh(ctx, ix)
    al, _ = count(ctx, seqs)
    assert want[1] == int(al.aligned.sum())
    got = ctx.pileup()
    same(got, want, "test.gfa")
    assert not got[0][:, [N, DEL, INS]].any() and got[2] == 0, "error-free reads delete, insert and mismatch nothing"
    ctx.pileup_end()


def test_synthetic_pangenome_narrow_bands(oracle, ctx, tmp_path):
    gfa = str(tmp_path / "syn100k.gfa")
    pkg().readsim.synth_pangenome(gfa, total_bp=100000)
    ix = oracle.Index(oracle.Graph.from_gfa(gfa), 11)
    seqs = [r.seq for r in pkg().readsim.config3_reads(gfa, 12, 3000)] + [r.seq for r in pkg().readsim.config2_reads(gfa, 40)]
    want = walker(oracle, ix, seqs)
    assert want[1] > 12
    fresh(ctx, ix)
    count(ctx, seqs)
    same(ctx.pileup(), want, "synthetic pangenome")
    ctx.pileup_end()


def test_one_long_problem_t7(oracle, ctx, drb1, monkeypatch):
    monkeypatch.setenv("VGA_POA_KERNEL", "t7")
    seqs = [r.seq for r in pkg().readsim.config3_reads(DRB1, 1)]
    want = walker(oracle, drb1, seqs)
    assert want[1] == 1
    fresh(ctx, drb1)
    count(ctx, seqs)
    same(ctx.pileup(), want, "t7")
    ctx.pileup_end()


# ---- 2. the rare tokens
RARE_SEED = 3


def rare_reads(seed):
    """DRB1 reads that carry what simulated reads seldom do: a few N in place of read bases, and 5-10 foreign bases in front of
    and behind them; reads that start at the first base of a haplotype path have nothing of the graph before them, so there the
    foreign bases can only be a leading insertion.  An optimal alignment never puts an insertion beside a deletion where
    mismatches are cheaper, so the last two reads replace a window of 36 haplotype bases that lacks one letter by 36 of that
    letter: nothing there can match, and a deletion plus an insertion cost less than 36 mismatches."""
    rs = pkg().readsim
    rng = np.random.default_rng(seed)
    foreign = lambda: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, int(rng.integers(5, 11))))
    seqs = []
    for r in rs.simulate_reads(DRB1, 10, 1500, 0.03, 0.03, 0.04, seed=100 + seed):
        s = list(r.seq)
        for i in rng.choice(len(s), 4, replace=False):
            s[int(i)] = "N"
        seqs.append(foreign() + "".join(s) + foreign())
    segs, paths = rs.parse_gfa_paths(DRB1)
    for _, steps in paths[:3]:
        seqs.append(foreign() + rs.path_sequence(segs, steps)[:1500])
    hap = rs.path_sequence(segs, paths[0][1])
    windows = [(i, b) for i in range(800, len(hap) - 836, 7) for b in "ACGT" if b not in hap[i:i + 36]]
    for w in rng.choice(len(windows), 2, replace=False):
        i, b = windows[int(w)]
        seqs.append(hap[i - 700:i] + b * 36 + hap[i + 36:i + 736])
    return seqs


def rare_properties(oracle, ix, seqs):
    """(table, leading insertions, N counts, insertions directly behind a deletion) of the reference on seqs"""
    ag = oracle_gaf(oracle, ix, seqs)
    a = oracle_index_arrays(ix)
    want = pileup_ref.walk(ag, a["node_seq_idx"], a["seq_fwd"])
    ins_after_del = sum(len(re.findall(r"-[a-z]+\+", ln)) for ln in ag.splitlines() if ln.split("\t")[5] != "*")
    return want, want[2], int(want[0][:, N].sum()), ins_after_del


def test_rare_tokens(oracle, ctx, drb1):
    seqs = rare_reads(RARE_SEED)
    want, leading, n_count, ins_after_del = rare_properties(oracle, drb1, seqs)
    # (on the reference alone, so that the case cannot silently vanish)
    assert leading > 0 and n_count > 0 and ins_after_del > 0, (leading, n_count, ins_after_del)
    fresh(ctx, drb1)
    count(ctx, seqs)
    same(ctx.pileup(), want, "rare tokens")
    ctx.pileup_end()


# ---- 3. both strands
@pytest.mark.parametrize("list_words", [None, "0"], ids=["lists on the device", "VGA_PILEUP_LIST_WORDS=0"])
def test_both_strands(oracle, ctx, drb1, monkeypatch, list_words):
    """... and with every list built by the host, which reads the reverse complement from the batch's host copy"""
    p = pkg()
    if list_words is not None:
        monkeypatch.setenv("VGA_PILEUP_LIST_WORDS", list_words)
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
    assert want[1] == int(al.aligned.sum()) == len(seqs)
    same(ctx.pileup(), want, "both strands")
    ctx.pileup_end()


# ---- 4. only the reported record of a read counts
def test_best_of_n_candidates_in_different_sub_batches(oracle, ctx, drb1, monkeypatch):
    p = pkg()
    src = p.readsim.simulate_reads(DRB1, 6, 700, 0.0, 0.0, 0.0, seed=23)
    seqs = [r.seq[:500] + r.seq[:500] for r in src] + [src[0].seq[:300] * 3, src[1].seq]
    monkeypatch.setenv("VGA_POA_SUB", "2")  # (two problems per launch: a read's candidates fall into different ones)
    fresh(ctx, drb1)
    for best_n in (1, 2, 5):
        ctx.pileup_reset()
        al, mo = count(ctx, seqs, best_n=best_n)
        assert max(len(mo.chains_of(r)) for r in range(len(seqs))) >= 2, "the test needs reads with several chains"
        if best_n > 1:
            assert al.poa_problems > len(seqs)
        same(ctx.pileup(), walker(oracle, drb1, seqs, best_n), "best_n %d" % best_n)
    ctx.pileup_end()


# ---- 5. problems that are handed back, and the routes around the defaults
def test_pool_that_starts_far_too_small(oracle, drb1, monkeypatch):
    monkeypatch.setenv("VGA_POOL_FILL", "0.002")
    monkeypatch.setenv("VGA_POOL_SEG", str(32 << 20))
    seqs = [r.seq for r in pkg().readsim.simulate_reads(DRB1, 320, 2500, 0.03, 0.03, 0.04, seed=41)]
    c = pkg().Context(0)
    try:
        fresh(c, drb1)
        count(c, seqs)
        same(c.pileup(), walker(oracle, drb1, seqs), "starved pool")
    finally:
        c.close()


@pytest.mark.parametrize("env", [{"VGA_POA_ARENAS": "0"}, {"VGA_POA_ARENAS": "0", "VGA_POOL_BYTES": "300000000", "VGA_POA_SUB": "2"},
                                 {"VGA_POA_TEXT": "host"}, {"VGA_POA_TB": "wave"}, {"VGA_POA_KERNEL": "t6"}, {"VGA_POA_KERNEL": "t4"},
                                 {"VGA_SG_SPLIT": "2", "VGA_POA_SUB": "2"},
                                 {"VGA_PILEUP_LIST_WORDS": "3000"}, {"VGA_PILEUP_LIST_WORDS": "0"}, {"VGA_PILEUP_LIST_WORDS": "3000", "VGA_POA_TEXT": "host"}],
                         ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_routes_count_the_same(ctx, drb1, routes, monkeypatch, capfd, env):
    """classic pool, re-queued sub-batches, host text, a traceback kernel of its own, forced DP kernels (t6 hands wide problems
    back: POA_ST_RETRY), the store in two parts -- and a list buffer too small for all (VGA_PILEUP_LIST_WORDS: the host builds the
    lists of the problems that found no room) or for any.  The library's trace (VGA_TRACE, stderr) says which route a problem
    took, so that a case cannot turn into another one unnoticed."""
    seqs, want = routes
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("VGA_TRACE", "1")
    fresh(ctx, drb1)
    capfd.readouterr()
    al, _ = count(ctx, seqs)
    trace = capfd.readouterr().err
    same(ctx.pileup(), want, str(env))
    ctx.pileup_end()
    by_host = len(re.findall(r"no room for its pileup list", trace))
    handed_back = sum(int(x) for x in re.findall(r"(\d+) problems handed back by the specialised DP kernel", trace))
    print("problems", al.poa_problems, "lists built by the host", by_host, "problems handed back", handed_back)
    words = env.get("VGA_PILEUP_LIST_WORDS")
    if words == "0":
        assert by_host == al.poa_problems == len(seqs)
    elif words is not None:
        assert 0 < by_host < al.poa_problems, "some lists on the device, some built by the host"
    else:
        assert by_host == 0
    if env.get("VGA_POA_KERNEL") == "t6":
        assert handed_back > 0, "a problem that runs twice replaces its record"


def test_subgraphs_on_the_host_are_refused_while_counting(ctx, drb1, monkeypatch):
    p = pkg()
    seqs = [r.seq for r in p.readsim.config2_reads(DRB1, 8)]
    fresh(ctx, drb1)
    monkeypatch.setenv("VGA_SUBGRAPH", "host")
    with pytest.raises(p.VgaError) as e:
        count(ctx, seqs)
    assert e.value.code == -4 and "VGA_SUBGRAPH" in str(e.value)
    counts, n, leading = ctx.pileup()
    assert n == 0 and leading == 0 and not counts.any()
    ctx.pileup_end()
    al, _ = count(ctx, seqs)  # (counting off: the host route is what it was)
    assert int(al.aligned.sum()) > 0


# ---- 6. life cycle
def _records(al):
    return (al.aligned.tolist(), al.cs, al.cigar, al.path_handles.tolist(), al.path_off.tolist(), al.path_start.tolist(), al.path_end.tolist(),
            al.block_length.tolist(), al.best_score.tolist())


def test_life_cycle(oracle, drb1_graph, drb1):
    p = pkg()
    s1 = [r.seq for r in p.readsim.simulate_reads(DRB1, 10, 2000, 0.03, 0.03, 0.04, seed=51)]
    s2 = [r.seq for r in p.readsim.simulate_reads(DRB1, 7, 1500, 0.03, 0.03, 0.04, seed=52)] + ["ACGT" * 30]
    w1, w2 = walker(oracle, drb1, s1), walker(oracle, drb1, s2)
    assert w2[1] == 7  # (the last read has no chain: a placeholder record adds nothing)
    c = p.Context(0)
    try:
        with pytest.raises(p.VgaError) as e:
            c.pileup_begin()
        assert e.value.code == -5  # VGA_ERR_NO_INDEX
        upload_oracle_index(c, drb1)
        for call in (c.pileup, c.pileup_reset):
            with pytest.raises(p.VgaError) as e:
                call()
            assert e.value.code == -1  # VGA_ERR_ARG: read / reset before begin
        al_off, _ = count(c, s1)
        assert not any(t["name"].startswith("k_pu") for t in c.kernel_times()), "counting off: no pileup kernel"
        c.pileup_begin()
        al_on, _ = count(c, s1)
        names = [t["name"] for t in c.kernel_times()]
        assert "k_pu_events" in names and "k_pu_add" in names, names
        assert _records(al_on) == _records(al_off), "counting changes no record"
        same(c.pileup(), w1, "first call")
        same(c.pileup(), w1, "read twice")
        count(c, s2)
        same(c.pileup(), add(w1, w2), "two calls accumulate")
        c.pileup_reset()
        counts, n, leading = c.pileup()
        assert n == 0 and leading == 0 and not counts.any()
        count(c, s2)
        same(c.pileup(), w2, "after reset")
        # a new index drops the counters and turns counting off
        ix19 = oracle.Index(drb1_graph, 19)
        upload_oracle_index(c, ix19)
        with pytest.raises(p.VgaError) as e:
            c.pileup()
        assert e.value.code == -1
        count(c, s1)
        assert not any(t["name"].startswith("k_pu") for t in c.kernel_times())
        c.pileup_begin()
        count(c, s1)
        same(c.pileup(), walker(oracle, ix19, s1), "counting again on the new index")
        c.pileup_end()
        c.pileup_end()  # (ending twice is harmless)
        with pytest.raises(p.VgaError):
            c.pileup()
    finally:
        c.close()


# ---- 7. the executable
HEADER = ["node", "offset", "ref", "A", "C", "G", "T", "N", "del", "ins"]


def _pileup_tsv(path):
    lines = open(path).read().splitlines()
    assert lines[0].split("\t") == HEADER, (path, lines[0])
    rows = [ln.split("\t") for ln in lines[1:]]
    return ([(int(r[0]), int(r[1]), r[2]) for r in rows], np.array([[int(x) for x in r[3:]] for r in rows], dtype=np.int64).reshape(-1, 7))


def test_cli(oracle, drb1, tmp_path):
    p = pkg()
    d = str(tmp_path)
    reads = p.readsim.config3_reads(DRB1, 40, 3000)
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
    idx, seq = a["node_seq_idx"], a["seq_fwd"].decode()
    counts, n_al, leading = pileup_ref.walk(oag, idx, seq)
    assert n_al == len(reads)
    want_keys = [(i + 1, o, seq[idx[i] + o]) for i in range(len(idx) - 1) for o in range(idx[i + 1] - idx[i])]
    common = ["map", "-i", os.path.join(d, "drb1"), "-f", fa, "-p", "abpoa", "--also-align", "-G", DRB1]
    run(common + ["-o", os.path.join(d, "plain")])
    assert not os.path.exists(os.path.join(d, "plain-pileup.tsv"))
    texts = {}
    for out, extra in (("one", ["--pileup"]), ("two", ["--pileup", "--devices", "0,0", "--chunk-reads", "10"]), ("both", ["--pileup", "--coverage"]),
                       ("only", ["--pileup", "--coverage-only"])):
        pr = run(common + ["-o", os.path.join(d, out)] + extra)
        assert "%d alignments piled up, %d leading insertions" % (n_al, leading) in pr.stderr, pr.stderr
        pre = os.path.join(d, out)
        texts[out] = open(pre + "-pileup.tsv").read()
        assert open(pre + "-chains.gaf").read() == open(os.path.join(d, "plain-chains.gaf")).read() == ocg, out
        if out == "only":
            assert not os.path.exists(pre + "-alignments.gaf")
        else:
            assert open(pre + "-alignments.gaf").read() == open(os.path.join(d, "plain-alignments.gaf")).read() == oag, out
    keys, table = _pileup_tsv(os.path.join(d, "one-pileup.tsv"))
    assert keys == want_keys
    assert np.array_equal(table, counts.astype(np.int64))
    assert texts["two"] == texts["one"] and texts["both"] == texts["one"] and texts["only"] == texts["one"]
    # beside --coverage: the five allele columns add up to the depth, line by line
    depth = [int(ln.split("\t")[2]) for ln in open(os.path.join(d, "both-coverage-bases.tsv")).read().splitlines()[1:]]
    assert table[:, :5].sum(1).tolist() == depth
